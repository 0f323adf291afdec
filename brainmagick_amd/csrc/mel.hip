// The MelSpectrum targets from waveforms that are resident on the device: MelSpectrum._compute (bm/features/audio.py:61-76)
// behind the channel mean -- `(wav - wav.mean()) / (1e-8 + wav.std())`, torchaudio.transforms.MelSpectrogram(n_fft, hop =
// n_fft / 4, normalized) and `log10(mel + eps)` -- as TWO launches for any number of waveforms.  torchaudio is restated
// from its documentation: torch.stft(center=True, pad_mode="reflect", periodic Hann window of n_fft, onesided), divided
// by sqrt(sum w^2) when normalized, |.|^2, times melscale_fbanks(htk, norm=None, f_min 0, f_max sr / 2).
//
// The waveforms come in a wave table (bm_wave.h; this unit holds its two host entry points), `out` the [n_mels][frames]
// output of a waveform; they are read with scalar loads, ONE summation order whatever the alignment.
//
// bm_wave_moments    grid (split, waveform), ONE launch.  A waveform of L samples is cut into ns(L) = at most MM_SPLITS
//     splits of at least MM_MIN_SPLIT samples (a function of L alone: the bits of a waveform's moments do not depend on
//     the other waveforms of the table).  Workgroup (k, w) walks its split twice in fp64: the sum -> the split's own
//     mean m_k, then the sum of (x - m_k)^2 (centred: a constant waveform gives exactly 0).  The workgroup of a waveform
//     that finishes last (bm_block.h's ticket, one counter per waveform) folds the partials in split order:
//     mean = (sum_k s_k) / L,  M2 = sum_k [q_k + n_k (m_k - mean)^2]  (the pairwise update of Chan, Golub & LeVeque),
//     std = sqrt(M2 / (L - 1)) (unbiased, torch's default), and stores (shift, scale) = (mean, 1 / (1e-8 + std)).
//
// bm_mel_spectrogram grid (frame tile, waveform), ONE launch.  A workgroup (256 threads) owns FT = 16 MT frames:
//   1. the (FT + 3) hop samples its frames cover go to LDS once, reflect-indexed at both ends of the waveform,
//      normalised as (float)(((double)x - shift) * scale): no padded or normalised copy of the waveform exists.  LDS
//      holds them in chunks of `hop` samples at a pitch of hop + 4 floats, so that the 16 frames x 4 samples of one A
//      fragment (frame stride = one chunk) fall into 64 different banks when hop is a multiple of 64;
//   2. frame j is the window [j hop, j hop + n_fft) of that span: the A operand (16 frames x 4 samples) is read from it
//      in place.  A wavefront takes 16 bins at a time: B fragments (4 samples x 16 bins) of the `re` and of the `im`
//      half of the basis [n_fft][2 nbp] (window and 1 / sqrt(sum w^2) folded in; from L2), v_mfma_f32_16x16x4_f32.
//      Every frame's re / im is a blocked sum in ONE fixed order, whatever the frame's tile, the grid or the table: per
//      quarter of the window, fmaf chains over 8 samples (k ascending, from 0.f), their sums added in ascending order;
//      the four quarters folded as (q0 + q1) + (q2 + q3).  (A single chain over all n_fft samples measured up to 4.7
//      times the deviation of torch's fp32 FFT from the fp64 truth, where the tests allow 4.)
//   3. power = fmaf(im, im, re re) into LDS [bin][frame];
//   4. one thread per output (mel row m, frame): fmaf over the bins [lo_m, hi_m) of row m ascending, from 0.f (an empty
//      row gives 0), then log10(mel + eps) when asked -- the sum in fp32, its logarithm rounded once; frames run along
//      the lanes, so a wavefront stores runs of a row.
// No atomics, every output element is stored exactly once.
#include "bm_block.h"
#include "bm_wave.h"

#define ML_THREADS 256
#define ML_WAVES (ML_THREADS / 64)
#define ML_PAD 4                        // floats between two chunks of `hop` samples in LDS
#define ML_BLOCK_STEPS 2                // MFMA steps (of 4 samples) that are one fmaf chain, a power of two
#define ML_MIN_NFFT 8
#define ML_MAX_NFFT 2048
#define ML_MAX_MELS 256
#define ML_WIDE_NFFT 1024               // up to here a workgroup owns 32 frames, beyond it 16 (LDS)
#define MM_SPLITS 256
#define MM_MIN_SPLIT 16384

extern "C" long bm_wave_table_entry_bytes(void) { return (long)sizeof(BmWave); }

extern "C" int bm_wave_table_fill(void* entry, const float* x, long L, float* out) {
    BM_REQUIRE(entry && x && L >= 1 && L < (1L << 31), "wave table: bad waveform (%ld samples; 1 <= L < 2^31)", L);
    BM_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 3) == 0, "wave table: a waveform or an output is not 4-byte aligned");
    BmWave* e = (BmWave*)entry;
    e->x = x;
    e->out = out;
    e->L = L;
    return BM_OK;
}

extern "C" int bm_mel_frame_tile(int n_fft) { return n_fft <= ML_WIDE_NFFT ? 32 : 16; }

// ---- moments ---------------------------------------------------------------------------------------------------------
// (samples per split, splits) of a waveform of L samples: no split is empty.
__host__ __device__ __forceinline__ int mm_per_split(int L) {
    int ns = (L + MM_MIN_SPLIT - 1) / MM_MIN_SPLIT;
    ns = ns < 1 ? 1 : ns > MM_SPLITS ? MM_SPLITS : ns;
    return (L + ns - 1) / ns;
}
__host__ __device__ __forceinline__ int mm_splits(int L) {
    const int per = mm_per_split(L);
    return (L + per - 1) / per;
}

extern "C" int bm_wave_moments_splits(long L) { return L >= 1 && L < (1L << 31) ? mm_splits((int)L) : 0; }

__global__ __launch_bounds__(ML_THREADS) void wave_moments_kernel(const BmWave* __restrict__ table, int max_splits,
                                                                  unsigned* tickets, double* part /* [W][max_splits][2] */,
                                                                  double* __restrict__ mom /* [W][2] */) {
    __shared__ BmFoldLds<double, ML_WAVES> sh;
    const int w = blockIdx.y, split = blockIdx.x;
    const BmWave e = table[w];
    const int L = (int)e.L;
    const int per = mm_per_split(L), ns = mm_splits(L);
    if (split >= ns || ns > max_splits) return;                 // uniform over the workgroup (the second: never, on a checked table)
    const int i0 = split * per, i1 = min(L, i0 + per);
    const float* __restrict__ x = e.x;
    double s = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += ML_THREADS) s += (double)x[i];
    s = bm_block_sum<ML_WAVES>(s, sh.wave[0]);
    const double mk = s / (double)(i1 - i0);
    double q = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += ML_THREADS) {
        const double d = (double)x[i] - mk;
        q = fma(d, d, q);
    }
    q = bm_block_sum<ML_WAVES>(q, sh.wave[0]);
    double* mine = part + ((long)w * max_splits + split) * 2;
    if (threadIdx.x == 0) {
        bm_store_partial(mine, s);
        bm_store_partial(mine + 1, q);
    }
    if (!bm_last_arriver(tickets + w, (unsigned)ns, &sh.last)) return;
    if (threadIdx.x == 0) {
        const double* p = part + (long)w * max_splits * 2;
        double tot = 0.0;
        for (int k = 0; k < ns; ++k) tot += p[2 * k];
        const double mean = tot / (double)L;
        double m2 = 0.0;
        for (int k = 0; k < ns; ++k) {
            const double nk = (double)(min(L, (k + 1) * per) - k * per);
            const double d = p[2 * k] / nk - mean;
            m2 += p[2 * k + 1] + nk * d * d;
        }
        const double sd = L < 2 ? __longlong_as_double(0x7ff8000000000000LL) : sqrt(m2 / (double)(L - 1));
        mom[2 * w] = mean;
        mom[2 * w + 1] = 1.0 / (1e-8 + sd);
    }
}

extern "C" int bm_wave_moments(const void* table, const long* lengths, int n_waves, unsigned* tickets, double* part,
                               int max_splits, double* mom, void* stream) {
    const long need = bm_wave_tiles("wave_moments", table, lengths, n_waves, 0, "", [](long L) { return mm_splits((int)L); });
    if (need <= 0) return (int)-need;                           // no waveform, or the error
    BM_REQUIRE(tickets && part && mom, "wave_moments: null pointer");
    BM_REQUIRE((((uintptr_t)part | (uintptr_t)mom) & 7) == 0, "wave_moments: the partials or the result are not 8-byte aligned");
    if (max_splits < need)
        return bm_set_error(BM_ERR_WORKSPACE, "wave_moments: room for %d splits per waveform, %ld needed", max_splits, need);
    hipLaunchKernelGGL(wave_moments_kernel, dim3((unsigned)need, n_waves), dim3(ML_THREADS), 0, (hipStream_t)stream,
                       (const BmWave*)table, max_splits, tickets, part, mom);
    return bm_check_launch("wave_moments");
}

// ---- the mel spectrogram ---------------------------------------------------------------------------------------------
struct MelArgs {
    const BmWave* table;
    const double* mom;                  // [W][2]: bm_wave_norm
    const float* basis;                 // [n_fft][2 nbp]: columns [0, nbp) re, [nbp, 2 nbp) im; bins >= nb are zero
    const float* fbw;                   // [n_mels][nb]
    const int* range;                   // [n_mels][2]: lo, hi
    int n_fft, nb, nbp, n_mels, use_log;
    float eps;
    BmFastDiv div_hop;
};

static inline size_t ml_span_floats(int n_fft, int FT) { return ((size_t)(FT + 3) * (n_fft / 4 + ML_PAD) + 3) & ~(size_t)3; }

template <int MT>
__global__ __launch_bounds__(ML_THREADS) void mel_spectrogram_kernel(const MelArgs g) {
    constexpr int FT = 16 * MT, FTP = FT + 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int N = g.n_fft, hop = N >> 2, pitch = hop + ML_PAD;
    float* span = smem;
    float* pw = smem + (((FT + 3) * pitch + 3) & ~3);           // [nbp][FTP]
    const BmWave e = g.table[blockIdx.y];
    const int L = (int)e.L;
    const int frames = 1 + L / hop;
    const int f0 = blockIdx.x * FT;
    if (f0 >= frames) return;                                   // uniform: a shorter waveform of the table
    const int nf = min(FT, frames - f0);
    const int tid = threadIdx.x;
    const BmWaveNorm norm = bm_wave_norm(g.mom, blockIdx.y);

    // 1: local sample i is sample g0 + i of the waveform padded by n_fft / 2 reflected samples on both sides (with
    // L > n_fft / 2 one reflection lands inside [0, L)).
    const long g0 = (long)f0 * hop - (N >> 1);
    const int nvalid = (nf + 3) * hop;
    const float* __restrict__ x = e.x;
    for (int i = tid; i < (FT + 3) * hop; i += ML_THREADS) {
        const int c = (int)bm_div((unsigned)i, g.div_hop);
        float v = 0.f;
        if (i < nvalid) v = bm_wave_normed(x[bm_wave_reflect(g0 + i, L)], norm);
        span[c * pitch + (i - c * hop)] = v;
    }
    __syncthreads();

    // 2 + 3
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
    const int ldb = 2 * g.nbp;
    for (int bt = wave; bt < (g.nbp >> 4); bt += ML_WAVES) {
        // One sum per quarter of the window (quarter q is chunk q of the frame's span), blocked: ML_BLOCK_STEPS steps of
        // 4 samples are one fmaf chain from 0.f with k ascending (re / im), the block sums are added to the quarter's
        // total (tre / tim) in ascending order, the quarters fold as (q0 + q1) + (q2 + q3).  ONE chain of n_fft terms
        // measured up to 4.7 times the deviation of torch's fp32 FFT from the fp64 truth and one chain per quarter up to
        // 4.05, where the tests allow 4; blocks of 8 samples stay near 1.5 in an emulation of this order on the CPU.
        // hop need not be a multiple of 4: the lanes past the quarter's end contribute 0 * 0.  The operands of the
        // next step are loaded before the MFMAs of the current one.
        f32x4 re[4][MT], im[4][MT], tre[4][MT], tim[4][MT];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                re[q][m] = f32x4{0.f, 0.f, 0.f, 0.f};
                im[q][m] = f32x4{0.f, 0.f, 0.f, 0.f};
                tre[q][m] = f32x4{0.f, 0.f, 0.f, 0.f};
                tim[q][m] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        const float* __restrict__ bp = g.basis + bt * 16 + lr;
        struct Ops {
            float b_re[4], b_im[4], a[4][MT];
        };
        auto load = [&](int s, Ops& o) {
            const int kl = 4 * s + lk;
            const bool in = kl < hop;
            const int kc = in ? kl : hop - 1;                   // every address stays inside the quarter
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long k = (long)q * hop + kc;
                const float br = bp[k * ldb], bi = bp[k * ldb + g.nbp];
                o.b_re[q] = in ? br : 0.f;
                o.b_im[q] = in ? bi : 0.f;
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const float av = span[(lr + q + 16 * m) * pitch + kc];
                    o.a[q][m] = in ? av : 0.f;
                }
            }
        };
        const int nsteps = (hop + 3) >> 2;
        Ops cur, nxt;
        load(0, cur);
        for (int s = 0; s < nsteps; ++s) {
            load(min(s + 1, nsteps - 1), nxt);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    re[q][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[q][m], cur.b_re[q], re[q][m], 0, 0, 0);
                    im[q][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a[q][m], cur.b_im[q], im[q][m], 0, 0, 0);
                }
            cur = nxt;
            if ((s & (ML_BLOCK_STEPS - 1)) == ML_BLOCK_STEPS - 1 || s == nsteps - 1) {      // uniform: a block ends
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        tre[q][m] += re[q][m];
                        tim[q][m] += im[q][m];
                        re[q][m] = f32x4{0.f, 0.f, 0.f, 0.f};
                        im[q][m] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
            }
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            f32x4 p;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float r = (tre[0][m][j] + tre[1][m][j]) + (tre[2][m][j] + tre[3][m][j]);
                const float i = (tim[0][m][j] + tim[1][m][j]) + (tim[2][m][j] + tim[3][m][j]);
                p[j] = fmaf(i, i, r * r);
            }
            *(f32x4*)(pw + (bt * 16 + lr) * FTP + m * 16 + lk * 4) = p;        // bin = column, frame = row
        }
    }
    __syncthreads();

    // 4
    float* __restrict__ out = e.out;
    for (int o = tid; o < g.n_mels * FT; o += ML_THREADS) {
        const int m = o / FT, fr = o % FT;
        if (fr >= nf) continue;
        const int lo = g.range[2 * m], hi = g.range[2 * m + 1];
        const float* __restrict__ wr = g.fbw + (long)m * g.nb;
        float acc = 0.f;
        for (int b = lo; b < hi; ++b) acc = fmaf(pw[b * FTP + fr], wr[b], acc);
        // the sum in fp32 as the reference's, its logarithm rounded once (log10f is good to 2 ulp, which at |log| >= 4 is
        // a quarter of the tolerance)
        out[(long)m * frames + f0 + fr] = g.use_log ? (float)log10((double)(acc + g.eps)) : acc;
    }
}

template <int MT>
static int ml_launch(const MelArgs& g, unsigned tiles, int n_waves, hipStream_t stream) {
    constexpr int FT = 16 * MT;
    const size_t lds = (ml_span_floats(g.n_fft, FT) + (size_t)g.nbp * (FT + 4)) * sizeof(float);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mel_spectrogram_kernel<MT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return bm_set_error((int)e, "mel_spectrogram: hipFuncSetAttribute: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL((mel_spectrogram_kernel<MT>), dim3(tiles, n_waves), dim3(ML_THREADS), lds, stream, g);
    return bm_check_launch("mel_spectrogram");
}

extern "C" int bm_mel_spectrogram(const void* table, const long* lengths, int n_waves, const double* mom,
                                  const float* basis, int n_fft, int nbp, const float* fbw, const int* range,
                                  const int* range_host, int n_mels, int use_log, float eps, void* stream) {
    BM_REQUIRE(n_fft >= ML_MIN_NFFT && n_fft <= ML_MAX_NFFT && n_fft % 4 == 0,
               "mel_spectrogram: n_fft = %d (%d <= n_fft <= %d, a multiple of 4)", n_fft, ML_MIN_NFFT, ML_MAX_NFFT);
    BM_REQUIRE(n_mels >= 1 && n_mels <= ML_MAX_MELS, "mel_spectrogram: n_mels = %d (1 <= n_mels <= %d)", n_mels, ML_MAX_MELS);
    const int nb = n_fft / 2 + 1, hop = n_fft / 4, FT = bm_mel_frame_tile(n_fft);
    BM_REQUIRE(nbp == ((nb + 15) & ~15), "mel_spectrogram: the basis has %d bin columns, expected %d", nbp, (nb + 15) & ~15);
    const long tiles = bm_wave_tiles("mel_spectrogram", table, lengths, n_waves, n_fft / 2, "the reflect padding: n_fft / 2 = ",
                                     [=](long L) { return (1 + L / hop + FT - 1) / FT; });
    if (tiles <= 0) return (int)-tiles;                         // no waveform, or the error
    BM_REQUIRE(basis && fbw && range && range_host, "mel_spectrogram: null pointer");
    BM_REQUIRE(((uintptr_t)mom & 7) == 0 && (((uintptr_t)basis | (uintptr_t)fbw | (uintptr_t)range) & 3) == 0,
               "mel_spectrogram: a table is not aligned");
    for (int m = 0; m < n_mels; ++m)                            // range_host (HOST memory): the same rows as `range`
        BM_REQUIRE(range_host[2 * m] >= 0 && range_host[2 * m] <= range_host[2 * m + 1] && range_host[2 * m + 1] <= nb,
                   "mel_spectrogram: filter %d covers the bins [%d, %d) of %d", m, range_host[2 * m], range_host[2 * m + 1], nb);
    MelArgs g;
    g.table = (const BmWave*)table;
    g.mom = mom;
    g.basis = basis;
    g.fbw = fbw;
    g.range = range;
    g.n_fft = n_fft;
    g.nb = nb;
    g.nbp = nbp;
    g.n_mels = n_mels;
    g.use_log = use_log;
    g.eps = eps;
    g.div_hop = bm_fastdiv((unsigned)hop);
    return FT == 32 ? ml_launch<2>(g, (unsigned)tiles, n_waves, (hipStream_t)stream)
                    : ml_launch<1>(g, (unsigned)tiles, n_waves, (hipStream_t)stream);
}
