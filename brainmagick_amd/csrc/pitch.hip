// The Pitch feature from waveforms that are resident on the device: what compute_yin(sig, sr, w_len, w_step, f0_min,
// f0_max, harmo_thresh)[0] (bm/lib/pitch_calc/yin.py, called by Pitch._compute, bm/features/audio.py:110-124) returns,
// as ONE launch for any number of waveforms.  Frame t starts at sample t w_step, t < ceil((L - w_len) / w_step), and
//     d(tau) = sum_{j = 0}^{w_len - tau - 1} (x_j - x_{j + tau})^2              (the reference's FFT expression, as a sum)
//     c(0) = 0,  c(tau) = d(tau) tau / sum_{1 .. tau} d                         for tau < tau_max
// the first tau in [tau_min, tau_max) with c(tau) < thresh is walked down while c(tau + 1) < c(tau) and tau + 1 < tau_max;
// the pitch is (float)(sr / tau), or 0 when there is none.  A silent frame gives 0 / 0 = NaN, every comparison is false
// and the pitch is 0; a frame that holds a NaN or an Inf has a running sum that is not finite from tau = 1 on (d(1) covers
// every sample), its c is NaN throughout -- what the reference's FFT makes of it -- and its pitch is 0.
//
// A wave table (bm_wave.h), `out` the frames of a waveform.  Grid (tile of YN_FT frames, waveform); a workgroup (256
// threads) stages the (YN_FT - 1) w_step + w_len samples of its frames in LDS once, as doubles; ONE wavefront per frame:
//   1. lanes over tau, 64 at a time: d(tau) in fp64 by fma with j ascending;
//   2. the running sum over the 64 lanes one after the other (tau ascending, the order of numpy's cumsum), carried from
//      one group of 64 to the next; c(tau) into the wavefront's row of LDS;
//   3. the first tau under the threshold by ballot, the walk down by reading c.
// No atomics, every output element is stored exactly once.
#include "bm_wave.h"

#define YN_THREADS 256
#define YN_FT (YN_THREADS / 64)         // frames per workgroup: one per wavefront
#define YN_MAX_WLEN 1024
#define YN_MAX_WSTEP 512

struct YnArgs {
    const BmWave* table;
    double sr, thresh;
    int w_len, w_step, tau_min, tau_max;
};

extern "C" int bm_yin_frames_tile(void) { return YN_FT; }

__device__ __forceinline__ double yn_readlane(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ __launch_bounds__(YN_THREADS) void yin_pitch_kernel(const YnArgs g) {
    extern __shared__ __attribute__((aligned(16))) double ysm[];
    const BmWave e = g.table[blockIdx.y];
    const long L = e.L;
    const long frames = (L - g.w_len + g.w_step - 1) / g.w_step;
    const long f0 = (long)blockIdx.x * YN_FT;
    if (f0 >= frames) return;                                   // uniform: a shorter waveform of the table
    const int nspan = (YN_FT - 1) * g.w_step + g.w_len;
    double* span = ysm;
    const long g0 = f0 * g.w_step;
    const float* __restrict__ x = e.x;
    for (int i = threadIdx.x; i < nspan; i += YN_THREADS) span[i] = g0 + i < L ? (double)x[g0 + i] : 0.0;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long f = f0 + wave;
    if (f >= frames) return;                                    // uniform over the wavefront; no barrier follows
    const double* xs = span + wave * g.w_step;
    double* c = ysm + nspan + wave * g.tau_max;                 // the wavefront's own row
    const int W = g.w_len;
    double run = 0.0;
    for (int base = 0; base < g.tau_max; base += 64) {
        const int tau = base + lane;
        double d = 0.0;
        if (tau >= 1 && tau < g.tau_max)
            for (int j = 0; j < W - tau; ++j) {
                const double v = xs[j] - xs[j + tau];
                d = fma(v, v, d);
            }
        double cs = 0.0;
#pragma unroll 4
        for (int i = 0; i < 64; ++i) {                          // lanes past tau_max and tau = 0 add +0.0
            run += yn_readlane(d, i);
            cs = lane == i ? run : cs;
        }
        if (tau < g.tau_max) {
            double v = 0.0;
            if (tau >= 1) v = isfinite(cs) ? d * (double)tau / cs : __longlong_as_double(0x7ff8000000000000LL);
            c[tau] = v;
        }
    }
    // 3: the row was written and is read by this wavefront alone
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    int found = 0;
    for (int base = 0; base < g.tau_max && !found; base += 64) {
        const int tau = base + lane;
        const bool under = tau >= g.tau_min && tau < g.tau_max && c[tau] < g.thresh;
        const unsigned long long mask = __ballot(under);
        if (mask) found = base + __builtin_ctzll(mask);
    }
    if (found)
        while (found + 1 < g.tau_max && c[found + 1] < c[found]) ++found;
    if (lane == 0) e.out[f] = found ? (float)(g.sr / (double)found) : 0.f;
}

extern "C" int bm_yin_pitch(const void* table, const long* lengths, int n_waves, double sr, int w_len, int w_step,
                            int tau_min, int tau_max, double thresh, void* stream) {
    BM_REQUIRE(w_len >= 2 && w_len <= YN_MAX_WLEN && w_step >= 1 && w_step <= YN_MAX_WSTEP,
               "yin_pitch: w_len = %d, w_step = %d (2 <= w_len <= %d, 1 <= w_step <= %d)", w_len, w_step, YN_MAX_WLEN,
               YN_MAX_WSTEP);
    BM_REQUIRE(tau_min >= 1 && tau_max <= w_len, "yin_pitch: tau_min = %d, tau_max = %d (1 <= tau_min, tau_max <= w_len = %d)",
               tau_min, tau_max, w_len);
    BM_REQUIRE(sr > 0, "yin_pitch: sr = %g", sr);
    const long tiles = bm_wave_tiles("yin_pitch", table, lengths, n_waves, w_len, "w_len = ",
                                     [=](long L) { return ((L - w_len + w_step - 1) / w_step + YN_FT - 1) / YN_FT; });
    if (tiles <= 0) return (int)-tiles;                         // no waveform, or the error
    YnArgs g;
    g.table = (const BmWave*)table;
    g.sr = sr;
    g.thresh = thresh;
    g.w_len = w_len;
    g.w_step = w_step;
    g.tau_min = tau_min;
    g.tau_max = tau_max < 0 ? 0 : tau_max;
    const size_t lds = ((size_t)(YN_FT - 1) * w_step + w_len + (size_t)YN_FT * g.tau_max) * sizeof(double);
    hipLaunchKernelGGL(yin_pitch_kernel, dim3((unsigned)tiles, n_waves), dim3(YN_THREADS), lds, (hipStream_t)stream, g);
    return bm_check_launch("yin_pitch");
}
