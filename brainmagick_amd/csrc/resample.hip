// julius.resample.ResampleFrac(old_sr, new_sr, zeros, rolloff) over waveforms that are resident on the device, the step
// in front of every audio feature of the reference (bm/features/audio.py:66, 113, 186), as ONE launch for all the
// waveforms of one reduced ratio old / new.  julius is restated from its published definition: a polyphase filter of
// `new` phases, each a Hann-windowed sinc of ntaps = 2 width + old taps normalised to a DC gain of 1 (the table is
// computed on the host, hip_ops.resample_taps), over the waveform replicate-padded by `width` samples on the left and
// `width + old` on the right:
//     out[f new + i] = sum_k taps[i][k] * padded[f old + k],   f < L / old + 1,  f new + i < floor(new L / old).
//
// The waveforms come in a wave table (bm_wave.h), `out` the outputs of a waveform.  Grid (tile of FT julius frames,
// waveform); a workgroup (256 threads)
//   1. stages the (FT - 1) old + ntp padded samples its frames cover in LDS once, replicate-indexed (no padded copy of
//      the waveform exists), normalised as (float)(((double)x - shift) * scale) when moments are given (the reference
//      normalises at the source rate, before it resamples);
//   2. new >= 16: a wavefront takes 16 frames x 16 phases at a time, v_mfma_f32_16x16x4_f32: the A operand (16 frames x
//      4 samples) is read in place from LDS with a row stride of `old`, the B operand (4 samples x 16 phases) from the
//      tap table [ntp][newp] in L2 (k padded with zero taps to ntp, a multiple of 4; phases padded to newp, a multiple
//      of 16).  ONE accumulator chain over k ascending from 0.f: an output's bits do not depend on its tile, the grid or
//      the other waveforms.  A samples at k >= ntaps enter as 0.f, so that a NaN next to a window stays out of it;
//      new < 16: one thread per output, fmaf over k ascending from 0.f (the same staging, the same table).
// A ratio always takes the same variant and the same FT (bm_resample_frames_tile).  Every output element is stored exactly
// once, no atomics.
#include "bm_wave.h"

#define RS_THREADS 256
#define RS_WAVES (RS_THREADS / 64)
#define RS_MAX_SPAN 16384               // floats of LDS (64 KiB) that 16 frames may cover: 15 old + ntp
#define RS_MAX_NEW 4096
#define RS_FMA_SPAN 8192                // floats that a tile of the few-phase variant stages at most
#define RS_FMA_MAX_FT 1024

struct RsArgs {
    const BmWave* table;
    const double* mom;                  // [W][2] (bm_wave_norm), or null: the samples as they are
    const float* taps;                  // [ntp][newp]
    int old_, new_, newp, width, ntaps, ntp, ft;
    BmFastDiv div_new;
};

static inline int rs_ntp(int old_, int width) { return (2 * width + old_ + 3) & ~3; }

// Frames per workgroup of a ratio, 0 outside the limits: a function of (old, new, width) alone.
static inline int rs_frames_tile(long old_, long new_, long width) {
    if (old_ < 1 || new_ < 1 || new_ > RS_MAX_NEW || width < 1 || old_ > RS_MAX_SPAN || width > RS_MAX_SPAN) return 0;
    const long ntp = rs_ntp((int)old_, (int)width);
    if (15 * old_ + ntp > RS_MAX_SPAN) return 0;
    if (new_ >= 16) return 16;                                  // one MFMA row block: 29 KiB of LDS at 441 / 160, five workgroups per CU
    long ft = ((RS_FMA_SPAN - ntp) / old_ + 1) & ~15L;
    return (int)(ft < 16 ? 16 : ft > RS_FMA_MAX_FT ? RS_FMA_MAX_FT : ft);
}

extern "C" int bm_resample_frames_tile(int old_rate, int new_rate, int width) {
    return rs_frames_tile(old_rate, new_rate, width);
}

__device__ __forceinline__ void rs_stage(const RsArgs& g, const BmWave& e, int f0, float* span) {
    const long L = e.L;
    const BmWaveNorm norm = bm_wave_norm(g.mom, blockIdx.y);
    const long g0 = (long)f0 * g.old_ - g.width;                // local sample i is sample g0 + i, replicate-indexed
    const int nspan = (g.ft - 1) * g.old_ + g.ntp;
    const float* __restrict__ x = e.x;
    for (int i = threadIdx.x; i < nspan; i += RS_THREADS) {
        const long s = bm_wave_replicate(g0 + i, L);
        span[i] = g.mom ? bm_wave_normed(x[s], norm) : x[s];
    }
    __syncthreads();
}

__global__ __launch_bounds__(RS_THREADS) void resample_mfma_kernel(const RsArgs g) {
    extern __shared__ __attribute__((aligned(16))) float span[];
    const BmWave e = g.table[blockIdx.y];
    const long out_len = (long)g.new_ * e.L / g.old_;
    const int f0 = blockIdx.x * g.ft;
    if ((long)f0 * g.new_ >= out_len) return;                   // uniform: a shorter waveform of the table
    rs_stage(g, e, f0, span);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
    const int ptiles = g.newp >> 4, jobs = (g.ft >> 4) * ptiles, nsteps = g.ntp >> 2;
    float* __restrict__ out = e.out;
    for (int job = wave; job < jobs; job += RS_WAVES) {
        const int m = job / ptiles, pt = job - m * ptiles;
        const long fm = (long)f0 + 16 * m;
        if (fm * g.new_ >= out_len) continue;                   // uniform over the wavefront
        const float* ap = span + (16 * m + lr) * g.old_ + lk;
        const float* __restrict__ bp = g.taps + (long)lk * g.newp + pt * 16 + lr;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float a = lk < g.ntaps ? ap[0] : 0.f, b = bp[0];
        for (int s = 0; s < nsteps; ++s) {                      // the operands of the next step before this step's MFMA
            const int sn = min(s + 1, nsteps - 1);
            const float av = ap[4 * sn];
            const float bn = bp[(long)4 * sn * g.newp];
            const float an = 4 * sn + lk < g.ntaps ? av : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
            a = an;
            b = bn;
        }
        const int phase = pt * 16 + lr;                         // column = phase, row = frame
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long n = (fm + lk * 4 + j) * g.new_ + phase;
            if (phase < g.new_ && n < out_len) out[n] = acc[j];
        }
    }
}

__global__ __launch_bounds__(RS_THREADS) void resample_fma_kernel(const RsArgs g) {
    extern __shared__ __attribute__((aligned(16))) float span[];
    const BmWave e = g.table[blockIdx.y];
    const long out_len = (long)g.new_ * e.L / g.old_;
    const int f0 = blockIdx.x * g.ft;
    const long n0 = (long)f0 * g.new_;
    if (n0 >= out_len) return;                                  // uniform
    rs_stage(g, e, f0, span);
    float* __restrict__ out = e.out;
    const float* __restrict__ taps = g.taps;
    for (int o = threadIdx.x; o < g.ft * g.new_; o += RS_THREADS) {
        if (n0 + o >= out_len) break;
        const int f = (int)bm_div((unsigned)o, g.div_new), i = o - f * g.new_;
        const float* sp = span + f * g.old_;
        float acc = 0.f;
        for (int k = 0; k < g.ntaps; ++k) acc = fmaf(sp[k], taps[k * g.newp + i], acc);
        out[n0 + o] = acc;
    }
}

extern "C" int bm_resample_frac(const void* table, const long* lengths, int n_waves, const double* mom, const float* taps,
                                int old_rate, int new_rate, int width, void* stream) {
    const int ft = rs_frames_tile(old_rate, new_rate, width);
    BM_REQUIRE(ft > 0, "resample_frac: ratio %d / %d with width %d (new <= %d; 15 old + 2 width + old <= %d floats of LDS)",
               old_rate, new_rate, width, RS_MAX_NEW, RS_MAX_SPAN);
    const long tiles = bm_wave_tiles("resample_frac", table, lengths, n_waves, 0, "",
                                     [=](long L) { return (L / old_rate + 1 + ft - 1) / ft; });
    if (tiles <= 0) return (int)-tiles;                         // no waveform, or the error
    for (int w = 0; w < n_waves; ++w)
        BM_REQUIRE(new_rate * lengths[w] / old_rate < (1L << 31),
                   "resample_frac: waveform %d has %ld samples (fewer than 2^31 outputs)", w, lengths[w]);
    BM_REQUIRE(taps, "resample_frac: null pointer");
    BM_REQUIRE(((uintptr_t)mom & 7) == 0 && ((uintptr_t)taps & 3) == 0, "resample_frac: a table is not aligned");
    RsArgs g;
    g.table = (const BmWave*)table;
    g.mom = mom;
    g.taps = taps;
    g.old_ = old_rate;
    g.new_ = new_rate;
    g.newp = (new_rate + 15) & ~15;
    g.width = width;
    g.ntaps = 2 * width + old_rate;
    g.ntp = rs_ntp(old_rate, width);
    g.ft = ft;
    g.div_new = bm_fastdiv((unsigned)new_rate);
    const size_t lds = ((size_t)(ft - 1) * old_rate + g.ntp) * sizeof(float);
    if (new_rate >= 16)
        hipLaunchKernelGGL(resample_mfma_kernel, dim3((unsigned)tiles, n_waves), dim3(RS_THREADS), lds, (hipStream_t)stream, g);
    else
        hipLaunchKernelGGL(resample_fma_kernel, dim3((unsigned)tiles, n_waves), dim3(RS_THREADS), lds, (hipStream_t)stream, g);
    return bm_check_launch("resample_frac");
}
