// A long FIR over long rows: the second half of the reference's preprocess_mne (bm/studies/api.py:334-363),
// `data -= julius.lowpass_filter(data, highpass / sample_rate)`, over a whole recording.  With half = (ntaps - 1) / 2:
//     s[r][t] = sum_{k < ntaps} taps[k] * x[r][clamp(t + k - half, 0, T - 1)],     y[r][t] = subtract ? x[r][t] - s : s.
// bm_lowpass's replicate-padding semantics, but rows are TILED in time and the taps are walked in chunks, so neither T
// nor half is bounded by LDS (a 0.1 Hz highpass at 120 Hz is half = 4800 over rows of 432 000 samples).
//
// Grid (time tile, row); a workgroup (256 threads, 4 wavefronts) owns FIR_NT = 4096 consecutive outputs of one row, a
// wavefront 1024 of them as FIR_NB = 4 accumulator blocks of 16 x 16.  The arithmetic is the exact-fp32 MFMA
// v_mfma_f32_16x16x4_f32 in every compute mode, in the Toeplitz form that resample_mfma_kernel is for old = new = 16:
// with xs[i] = x[clamp(t0 - half + i)], output t0 + 16 f + p is row f, column p of
//     A[f][j] = xs[16 f + j],     B[j][p] = taps[j - p]  (zero outside [0, ntaps)),     j in [0, ntaps + 15).
// ONE accumulator chain per output, j ascending from 0.f, carried in registers across the tap chunks; the MFMA is a
// k-ordered fmaf chain, and the zero entries of B add nothing to a finite sum.  So an output's bits depend on its own
// window alone -- not on the tile, the grid, the chunking or the other rows -- and for finite input the outputs equal
// bm_lowpass's (fp32 fmaf, taps ascending from 0.f) as numbers wherever that kernel applies.
//
// The tap walk: chunks of FIR_CH = 2048 values of j.  Per chunk a workgroup stages the FIR_NT + FIR_CH samples the chunk
// touches (replicate-indexed while staging, bm_wave_replicate: no load leaves its row) and the FIR_CH + 16 taps around
// them (zero outside the filter: no padded tap vector, no Toeplitz table), 33.5 KiB of LDS in all, so four workgroups
// share a CU and one's staging hides behind the others' MFMAs.  A lane's B value is tp[j0 + (lane >> 4) - (lane & 15) +
// 15]: 19 consecutive words per wavefront, conflict-free, and it feeds all four blocks of the wavefront (the resampler
// fetches a B fragment per MFMA).  The samples are staged de-interleaved by s mod 16, sample s at [s & 15][s >> 4] with
// a pitch of FIR_PITCH = 400 words (16 mod 32): the A read of a step is 16 consecutive words per k, the four k a pitch
// apart on distinct banks, where the resampler's (16 m + lr) * 16 + lk puts four lanes on one bank; the blocks and the
// four steps of a group of 16 j are constant offsets from one address.  The operands of the next group are read before
// this group's 16 MFMAs.  A values at j >= ntaps + 15 enter as 0.f, so a sample beyond that never reaches an output.
//
// Non-finite samples: in the Toeplitz form 0 * NaN reaches the up to 15 outputs on either side of a window.  The
// contract: a non-finite sample makes non-finite every output within `half` of it, may do so up to 15 samples further,
// and nothing beyond.
//
// No flags, no atomics: every output is stored exactly once.  Row offsets are 64-bit.  72 VGPRs + 16 AGPRs, 54 SGPRs,
// ScratchSize 0, no spills.
//
// Measured (profiles/preprocess_vs_torch.txt; HIP events around the call): 273 rows x 216 000 samples, 9601 taps, 1132
// GFLOP in 11.3 ms = 100 TFLOP/s, 64 % of the 157 TF exact-fp32 matrix peak (the resampler's loop: 17 %); torch's direct
// F.conv1d takes 445 ms for the same sum (no element differs), an rfft product 1.9 ms -- the FFT form does a hundredth of the
// arithmetic and is FASTER; the direct form is kept for its fixed order and its per-sample bound.  Not tried: staging
// the next chunk into registers under the MFMAs (a workgroup's staging is hidden by the three others on its CU only).
#include "bm_wave.h"

#define FIR_THREADS 256
#define FIR_WAVES (FIR_THREADS / 64)
#define FIR_NB 4                                    // accumulator blocks (16 x 16 outputs) of a wavefront
#define FIR_NT (FIR_WAVES * FIR_NB * 256)           // outputs of a workgroup: 4096
#define FIR_CH 2048                                 // values of j (taps + 15) per chunk, a multiple of 16
#define FIR_PITCH 400                               // >= (FIR_NT + FIR_CH) / 16 = 384, and 16 mod 32
#define FIR_MAX_HALF 16384
#define FIR_MAX_ROWS 65535                          // gridDim.y

static_assert(FIR_CH % 16 == 0 && FIR_PITCH >= (FIR_NT + FIR_CH) / 16 && FIR_PITCH % 32 == 16, "the staging layout");
static_assert((16 * FIR_PITCH + FIR_CH + 16) * sizeof(float) <= 65536, "at most 64 KiB of LDS");

extern "C" int bm_fir_tile(void) { return FIR_NT; }
extern "C" int bm_fir_chunk(void) { return FIR_CH; }
extern "C" int bm_fir_max_half(void) { return FIR_MAX_HALF; }

__global__ __launch_bounds__(FIR_THREADS) void fir_rows_kernel(const float* __restrict__ x, long row_stride,
                                                               float* __restrict__ y, int T,
                                                               const float* __restrict__ taps, int ntaps, int subtract) {
    __shared__ float smp[16 * FIR_PITCH];           // sample jc + i of the tile's span at [i & 15][i >> 4]
    __shared__ float tp[FIR_CH + 16];               // tp[i] = taps[jc + i - 15], zero outside the filter
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
    const int half = (ntaps - 1) >> 1, J = ntaps + 15;
    const long t0 = (long)blockIdx.x * FIR_NT;
    const float* __restrict__ xr = x + (long)blockIdx.y * row_stride;
    const long tw = t0 + wave * (FIR_NB * 256);     // the wavefront's first output
    const bool live = tw < T;                       // uniform over the wavefront; every wavefront stages and syncs

    f32x4 acc[FIR_NB];
#pragma unroll
    for (int b = 0; b < FIR_NB; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int jc = 0; jc < J; jc += FIR_CH) {
        if (jc) __syncthreads();                    // the previous chunk has been read
        const long g0 = t0 - half + jc;
        for (int i = threadIdx.x; i < FIR_NT + FIR_CH; i += FIR_THREADS)
            smp[(i & 15) * FIR_PITCH + (i >> 4)] = xr[bm_wave_replicate(g0 + i, T)];
        for (int i = threadIdx.x; i < FIR_CH + 16; i += FIR_THREADS) {
            const int k = jc + i - 15;
            tp[i] = k >= 0 && k < ntaps ? taps[k] : 0.f;
        }
        __syncthreads();
        if (!live) continue;
        const int jn = min(FIR_CH, J - jc);         // values of j in this chunk
        const int groups = (jn + 15) >> 4;
        // group q, step u: j0 = 16 q + 4 u;  A of block b: sample 256 (4 wave + b) + 16 lr + j0 + lk
        const float* ap = smp + lk * FIR_PITCH + wave * (FIR_NB * 16) + lr;
        const float* bp = tp + lk - lr + 15;
        float a[4][FIR_NB], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            bv[u] = bp[4 * u];
#pragma unroll
            for (int b = 0; b < FIR_NB; ++b) a[u][b] = 4 * u + lk < jn ? ap[4 * u * FIR_PITCH + 16 * b] : 0.f;
        }
        for (int q = 0; q < groups; ++q) {
            const int qn = min(q + 1, groups - 1);
            float an[4][FIR_NB], bn[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bn[u] = bp[16 * qn + 4 * u];
#pragma unroll
                for (int b = 0; b < FIR_NB; ++b) {
                    const float v = ap[qn + 4 * u * FIR_PITCH + 16 * b];
                    an[u][b] = 16 * qn + 4 * u + lk < jn ? v : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int b = 0; b < FIR_NB; ++b)
                    acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][b], bv[u], acc[b], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bv[u] = bn[u];
#pragma unroll
                for (int b = 0; b < FIR_NB; ++b) a[u][b] = an[u][b];
            }
        }
    }
    if (!live) return;
    float* __restrict__ yr = y + (long)blockIdx.y * T;
#pragma unroll
    for (int b = 0; b < FIR_NB; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j) {               // column = lane & 15, row = 4 (lane >> 4) + j
            const long t = tw + 256 * b + 16 * (4 * lk + j) + lr;
            if (t < T) yr[t] = subtract ? xr[t] - acc[b][j] : acc[b][j];
        }
}

extern "C" int bm_fir_rows(const float* x, long row_stride, float* y, int rows, long T, const float* taps, int ntaps,
                           int subtract, void* stream) {
    BM_REQUIRE(rows >= 0 && rows <= FIR_MAX_ROWS, "fir_rows: %d rows, the limit is %d", rows, FIR_MAX_ROWS);
    BM_REQUIRE(T >= 1 && T < (1L << 31), "fir_rows: rows of %ld samples (1 <= T < 2^31)", T);
    BM_REQUIRE(ntaps >= 1 && (ntaps & 1), "fir_rows: %d taps (an odd number: 2 half + 1)", ntaps);
    BM_REQUIRE((ntaps - 1) / 2 <= FIR_MAX_HALF, "fir_rows: half = %d, the limit is %d", (ntaps - 1) / 2, FIR_MAX_HALF);
    BM_REQUIRE(row_stride >= T, "fir_rows: row_stride %ld is below T = %ld", row_stride, T);
    if (rows == 0) return BM_OK;
    BM_REQUIRE(x && y && taps, "fir_rows: null pointer");
    BM_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)taps) & 3) == 0, "fir_rows: a pointer is not 4-byte aligned");
    const unsigned tiles = (unsigned)((T + FIR_NT - 1) / FIR_NT);
    hipLaunchKernelGGL(fir_rows_kernel, dim3(tiles, rows), dim3(FIR_THREADS), 0, (hipStream_t)stream, x, row_stride, y,
                       (int)T, taps, ntaps, subtract);
    return bm_check_launch("fir_rows");
}
