// Fitting the scalers of bm/norm.py on the device (the one-off job in front of the first training step).
//   bm/norm.py:58-80    RobustScaler.fit: per channel, sort the column and read the values at int(q * n), q = .25, .5, .75
//   bm/norm.py:96-105   StandardScaler.fit: masked mean / unbiased std, per channel or over the whole slice
//   bm/norm.py:136-142  NoOpCategoryCountScaler.fit: assert on all of X, histogram of the selected values
//   bm/norm.py:85-86, 110-111  inverse_transform: (X * scale_) + center_
// The reference sorts one channel at a time and reads every quantile back with `.item()`.  Fitting needs three order
// statistics per column, not a sorted column: bm_quantile_select is an MSD radix select (four 8-bit digits) over the
// [N][C][T] layout the batches already have, all ranks of a channel resolved in the same passes.  Counting is integer
// only (LDS histograms, integer global adds): order-independent, two runs are bit-identical.  A column is split over
// several workgroups; they never wait for each other inside a launch -- every digit is one counting launch and one
// small per-channel scan launch, ordered by the stream.
#include "bm_block.h"

#define SF_THREADS 256
#define SF_MAXQ 8
#define SF_BINS 256
#define SF_PASSES 4
#define SF_MASK_NONE 0
#define SF_MASK_ROW 1       // [N][1][T]
#define SF_MASK_FULL 2      // [N][F][T]
#define SF_MAX_CARDINALITY 16384
#define SF_MOMENT_SPLITS 64

struct SfRanks {
    unsigned r[SF_MAXQ];
};

// Order-preserving key of torch.sort's ascending order: negatives with all bits flipped, the others with the sign bit
// set; EVERY NaN (either sign bit) is the largest key, as torch.sort puts all NaNs last.  (-0 sorts below +0 here;
// torch calls them equal.)
__device__ __forceinline__ unsigned sf_key(float v) {
    const unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sf_unkey(unsigned k) {
    if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);      // no other value has this key
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// ++hist[bin] in LDS for every lane with bin >= 0; called by whole wavefronts (converged).  Raw MEG puts nearly every
// sample of a column into two or three bins of the leading digit: the two most common bins of a wavefront are added
// once each with the number of their lanes, the rest with one LDS atomic per lane (few lanes per address).
__device__ __forceinline__ void sf_lds_count(unsigned* hist, int bin) {
    const int lane = threadIdx.x & (BM_WAVE - 1);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long act = __ballot(bin >= 0);
        if (act == 0ull) return;                                    // wave-uniform
        const int leader = __ffsll((long long)act) - 1;
        const int b0 = __shfl(bin, leader);
        const unsigned long long same = __ballot(bin == b0);
        if (lane == leader) atomicAdd(&hist[b0], (unsigned)__popcll(same));
        if (bin == b0) bin = -1;
    }
    if (bin >= 0) atomicAdd(&hist[bin], 1u);
}

template <int V>
__device__ __forceinline__ void sf_load(const float* __restrict__ p, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void sf_load_mask(const unsigned char* __restrict__ p, unsigned char (&m)[V]) {
    if constexpr (V == 4) {
        const uchar4 t = *reinterpret_cast<const uchar4*>(p);
        m[0] = t.x; m[1] = t.y; m[2] = t.z; m[3] = t.w;
    } else {
        m[0] = *p;
    }
}

// ---- (a) quantile select -------------------------------------------------------------------------------------------
// State of rank q of channel c after `pass` digits: prefix[c][q] = the leading 8 * pass key bits of the wanted element,
// rank[c][q] = its index among the column's elements with that prefix.  Ranks that share a prefix share one histogram,
// filed under the first of them.
//
// Counting launch of one digit: workgroup (split, c) walks the segments [split * nper, ...) of column c.
template <int V>
__global__ __launch_bounds__(SF_THREADS) void sf_count_kernel(const float* __restrict__ x, int N, int C, int T, int Q,
                                                             int pass, int nper, BmFastDiv div_tv,
                                                             const unsigned* __restrict__ prefix,
                                                             unsigned* __restrict__ hist /* this digit: [C][Q][256] */) {
    __shared__ unsigned sh_hist[SF_MAXQ * SF_BINS];
    __shared__ unsigned sh_pref[SF_MAXQ];
    __shared__ int sh_owner[SF_MAXQ];
    __shared__ int sh_nu;
    const int split = blockIdx.x, c = blockIdx.y;
    for (int i = threadIdx.x; i < Q * SF_BINS; i += SF_THREADS) sh_hist[i] = 0u;
    if (threadIdx.x == 0) {
        int nu = 0;
        if (pass == 0) {
            sh_pref[0] = 0u;
            sh_owner[0] = 0;
            nu = 1;
        } else {
            for (int q = 0; q < Q; ++q) {
                const unsigned p = prefix[c * Q + q];
                bool seen = false;
                for (int u = 0; u < nu; ++u) seen |= sh_pref[u] == p;
                if (!seen) {
                    sh_pref[nu] = p;
                    sh_owner[nu] = q;
                    ++nu;
                }
            }
        }
        sh_nu = nu;
    }
    __syncthreads();
    const int nu = sh_nu;
    unsigned up[SF_MAXQ];
#pragma unroll
    for (int u = 0; u < SF_MAXQ; ++u) up[u] = u < nu ? sh_pref[u] : 0u;
    const int n0 = split * nper;
    const int nn = min(N, n0 + nper) - n0;
    const unsigned Tv = (unsigned)(T / V);
    const unsigned nvec = nn > 0 ? (unsigned)nn * Tv : 0u;
    const int dshift = 24 - 8 * pass;            // this digit
    const int pshift = 32 - 8 * pass;            // what is above it (pass > 0)
    for (unsigned base = 0; base < nvec; base += SF_THREADS) {        // block-uniform trip count (sf_lds_count)
        const unsigned j = base + threadIdx.x;
        const bool valid = j < nvec;
        float v[V];
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = 0.f;
        if (valid) {
            const unsigned nl = bm_div(j, div_tv);
            const unsigned tv = j - nl * Tv;
            sf_load<V>(x + ((size_t)(n0 + nl) * C + c) * T + (size_t)tv * V, v);
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const unsigned key = sf_key(v[i]);
            const int digit = (int)((key >> dshift) & 255u);
            int bin = -1;
            if (pass == 0) {
                bin = digit;
            } else {
                const unsigned head = key >> pshift;
#pragma unroll
                for (int u = 0; u < SF_MAXQ; ++u)
                    if (u < nu && head == up[u]) bin = u * SF_BINS + digit;
            }
            sf_lds_count(sh_hist, valid ? bin : -1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nu * SF_BINS; i += SF_THREADS) {
        const unsigned cnt = sh_hist[i];
        if (cnt) atomicAdd(&hist[((size_t)c * Q + sh_owner[i >> 8]) * SF_BINS + (i & 255)], cnt);
    }
}

// Scan launch of one digit: workgroup c, one wavefront per rank; the digit of rank q is the bin in which the running
// count passes rank[c][q].  The last digit writes the value.
__global__ __launch_bounds__(SF_THREADS) void sf_scan_kernel(int Q, int pass, SfRanks ranks,
                                                            const unsigned* __restrict__ hist,
                                                            unsigned* __restrict__ prefix, unsigned* __restrict__ rank,
                                                            float* __restrict__ out) {
    __shared__ unsigned sh_pref[SF_MAXQ], sh_rank[SF_MAXQ];
    const int c = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < Q) {
        unsigned r0 = 0u;
#pragma unroll
        for (int k = 0; k < SF_MAXQ; ++k)
            if (k == (int)threadIdx.x) r0 = ranks.r[k];
        sh_pref[threadIdx.x] = pass ? prefix[c * Q + threadIdx.x] : 0u;
        sh_rank[threadIdx.x] = pass ? rank[c * Q + threadIdx.x] : r0;
    }
    __syncthreads();                              // every old state is read before any new one is written
    for (int q = wave; q < Q; q += SF_THREADS / 64) {
        const unsigned pq = sh_pref[q];
        int owner = q;
        for (int k = q - 1; k >= 0; --k)
            if (sh_pref[k] == pq) owner = k;
        const uint4 hv = reinterpret_cast<const uint4*>(hist + ((size_t)c * Q + owner) * SF_BINS)[lane];
        const unsigned s = hv.x + hv.y + hv.z + hv.w;
        unsigned incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        const unsigned r = sh_rank[q];
        unsigned e = incl - s;
        if (r >= e && r < incl) {                 // exactly one lane: r < the number of elements under the prefix
            int d = 3;
            if (r < e + hv.x) d = 0;
            else if (r < e + hv.x + hv.y) d = 1, e += hv.x;
            else if (r < e + hv.x + hv.y + hv.z) d = 2, e += hv.x + hv.y;
            else e += hv.x + hv.y + hv.z;
            const unsigned np = (pq << 8) | (unsigned)(4 * lane + d);
            if (pass == SF_PASSES - 1) {
                out[c * Q + q] = sf_unkey(np);
            } else {
                prefix[c * Q + q] = np;
                rank[c * Q + q] = r - e;
            }
        }
    }
}

// workspace: the four digits' histogram tables [4][C][Q][256] (ZEROED by the caller before every call), then the state
static long sf_select_hist_words(int C, int Q) { return (long)SF_PASSES * C * Q * SF_BINS; }
extern "C" long bm_quantile_select_workspace_bytes(int C, int Q) {
    if (C < 0 || Q < 0) return 0;
    return (sf_select_hist_words(C, Q) + 2L * C * Q) * 4;
}

extern "C" int bm_quantile_select(const float* x, const long* ranks, float* out, int N, int C, int T, int Q,
                                  void* workspace, long workspace_bytes, void* stream) {
    BM_REQUIRE(N >= 0 && C >= 0 && T >= 0 && C <= 65535, "quantile_select: bad shape");
    BM_REQUIRE(Q >= 1 && Q <= SF_MAXQ, "quantile_select: 1 <= Q <= %d ranks, got %d", SF_MAXQ, Q);
    const long n = (long)N * T;
    BM_REQUIRE(n < (1L << 31), "quantile_select: %ld elements per column: counts are 32-bit", n);
    if (n * C == 0) return BM_OK;
    BM_REQUIRE(x && ranks && out, "quantile_select: null pointer");
    SfRanks rk;
    for (int q = 0; q < SF_MAXQ; ++q) rk.r[q] = 0u;
    for (int q = 0; q < Q; ++q) {
        BM_REQUIRE(ranks[q] >= 0 && ranks[q] < n && (q == 0 || ranks[q] >= ranks[q - 1]),
                   "quantile_select: ranks must ascend within [0, %ld)", n);
        rk.r[q] = (unsigned)ranks[q];
    }
    if (!workspace || workspace_bytes < bm_quantile_select_workspace_bytes(C, Q))
        return bm_set_error(BM_ERR_WORKSPACE, "quantile_select: workspace");
    // ~2 048 workgroups of at least 4 096 elements: (split, channel)
    long nsplit = cdiv(2048, C);
    if (nsplit > cdiv(n, 4096)) nsplit = cdiv(n, 4096);
    if (nsplit > N) nsplit = N;
    if (nsplit < 1) nsplit = 1;
    const int nper = cdiv(N, nsplit);
    nsplit = cdiv(N, nper);
    const bool vec = T % 4 == 0 && ((uintptr_t)x & 15) == 0;
    unsigned* hist = (unsigned*)workspace;
    unsigned* prefix = hist + sf_select_hist_words(C, Q);
    unsigned* rank = prefix + (long)C * Q;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nsplit, C);
    for (int pass = 0; pass < SF_PASSES; ++pass) {
        unsigned* h = hist + (long)pass * C * Q * SF_BINS;
        if (vec)
            hipLaunchKernelGGL(sf_count_kernel<4>, grid, dim3(SF_THREADS), 0, s, x, N, C, T, Q, pass, nper,
                               bm_fastdiv((unsigned)(T / 4)), prefix, h);
        else
            hipLaunchKernelGGL(sf_count_kernel<1>, grid, dim3(SF_THREADS), 0, s, x, N, C, T, Q, pass, nper,
                               bm_fastdiv((unsigned)T), prefix, h);
        hipLaunchKernelGGL(sf_scan_kernel, dim3(C), dim3(SF_THREADS), 0, s, Q, pass, rk, h, prefix, rank, out);
    }
    return bm_check_launch("quantile_select");
}

// ---- (b) masked moments --------------------------------------------------------------------------------------------
// Two walks of the slice, each followed by a one-workgroup fold of the per-workgroup fp64 partials in a fixed order:
// sum and count -> mean, then sum (x - mean)^2 -> unbiased std.  (Centred, not sum x^2 - n mean^2: a constant feature
// gives exactly 0, which the "could not be normalized" assert of bm/norm.py:234-237 relies on.)
template <int V>
__global__ __launch_bounds__(SF_THREADS) void sf_moments_kernel(const float* __restrict__ x,
                                                               const unsigned char* __restrict__ mask, int mask_mode,
                                                               int N, int F, int T, int f0, int nper, BmFastDiv div_tv,
                                                               const double* __restrict__ center /* null: first walk */,
                                                               double* __restrict__ part_sum,
                                                               double* __restrict__ part_cnt /* [channels][nsplit] */) {
    __shared__ double sh[8];
    const int split = blockIdx.x, ch = blockIdx.y, f = f0 + ch, nsplit = gridDim.x;
    const int n0 = split * nper;
    const int nn = min(N, n0 + nper) - n0;
    const unsigned Tv = (unsigned)(T / V);
    const unsigned nvec = nn > 0 ? (unsigned)nn * Tv : 0u;
    const double ce = center ? center[ch] : 0.0;
    double s = 0.0, cnt = 0.0;
    for (unsigned j = threadIdx.x; j < nvec; j += SF_THREADS) {
        const unsigned nl = bm_div(j, div_tv);
        const unsigned tv = j - nl * Tv;
        const size_t n = (size_t)(n0 + nl);
        float v[V];
        unsigned char m[V];
        sf_load<V>(x + (n * F + f) * T + (size_t)tv * V, v);
#pragma unroll
        for (int i = 0; i < V; ++i) m[i] = 1;
        if (mask_mode == SF_MASK_FULL) sf_load_mask<V>(mask + (n * F + f) * T + (size_t)tv * V, m);
        else if (mask_mode == SF_MASK_ROW) sf_load_mask<V>(mask + n * T + (size_t)tv * V, m);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const double d = (double)v[i] - ce;
            const double w = center ? d * d : d;
            s += m[i] ? w : 0.0;
            cnt += m[i] ? 1.0 : 0.0;
        }
    }
    s = bm_block_sum<SF_THREADS / 64>(s, sh);
    cnt = bm_block_sum<SF_THREADS / 64>(cnt, sh + 4);
    if (threadIdx.x == 0) {
        part_sum[ch * nsplit + split] = s;
        part_cnt[ch * nsplit + split] = cnt;
    }
}

// stage 0: center[ch] = mean (fp64, for the second walk); stage 1: count, mean and std, rounded to fp32 once.
__global__ __launch_bounds__(SF_THREADS) void sf_moments_fold_kernel(const double* __restrict__ part_sum,
                                                                    const double* __restrict__ part_cnt, int nch,
                                                                    int nsplit, int per_channel, int stage,
                                                                    double* __restrict__ center, float* __restrict__ mean,
                                                                    float* __restrict__ std, double* __restrict__ count) {
    __shared__ double sh[8];
    double gs = 0.0, gc = 0.0;
    if (!per_channel) {                           // one statistic over the whole slice
        for (int k = threadIdx.x; k < nch * nsplit; k += SF_THREADS) {
            gs += part_sum[k];
            gc += part_cnt[k];
        }
        gs = bm_block_sum<SF_THREADS / 64>(gs, sh);
        gc = bm_block_sum<SF_THREADS / 64>(gc, sh + 4);
    }
    for (int ch = threadIdx.x; ch < nch; ch += SF_THREADS) {
        double s = gs, c = gc;
        if (per_channel) {
            s = 0.0;
            c = 0.0;
            for (int k = 0; k < nsplit; ++k) {
                s += part_sum[ch * nsplit + k];
                c += part_cnt[ch * nsplit + k];
            }
        }
        if (stage == 0) {
            center[ch] = s / c;                   // nothing selected: 0 / 0 = NaN, like torch's mean of nothing
        } else {
            count[ch] = c;
            mean[ch] = (float)center[ch];
            std[ch] = c < 2.0 ? __uint_as_float(0x7fc00000u) : (float)sqrt(s / (c - 1.0));      // torch.std of one value: NaN
        }
    }
}

// workspace: partial sums and counts [channels][SF_MOMENT_SPLITS] each, then the fp64 means [channels]
extern "C" long bm_masked_moments_workspace_bytes(int channels) {
    return channels < 0 ? 0 : (2L * SF_MOMENT_SPLITS + 1) * channels * 8;
}

extern "C" int bm_masked_moments(const float* x, const unsigned char* mask, int mask_mode, int N, int F, int T, int f0,
                                 int f1, int per_channel, float* mean, float* std, double* count, void* workspace,
                                 long workspace_bytes, void* stream) {
    BM_REQUIRE(N >= 0 && F > 0 && T >= 0 && (long)N * F * T < (1L << 31), "masked_moments: bad shape");
    BM_REQUIRE(f0 >= 0 && f0 < f1 && f1 <= F && f1 - f0 <= 65535, "masked_moments: bad channel range [%d, %d) of %d",
               f0, f1, F);
    BM_REQUIRE(mask_mode >= SF_MASK_NONE && mask_mode <= SF_MASK_FULL && (mask_mode == SF_MASK_NONE || mask),
               "masked_moments: bad mask");
    BM_REQUIRE(mean && std && count && (x || (long)N * T == 0), "masked_moments: null pointer");
    const int nch = f1 - f0;
    if (!workspace || workspace_bytes < bm_masked_moments_workspace_bytes(nch))
        return bm_set_error(BM_ERR_WORKSPACE, "masked_moments: workspace");
    long nsplit = cdiv((long)N * T, 4096);
    if (nsplit > cdiv(1024, nch)) nsplit = cdiv(1024, nch);
    if (nsplit > SF_MOMENT_SPLITS) nsplit = SF_MOMENT_SPLITS;
    if (nsplit > N) nsplit = N;
    if (nsplit < 1) nsplit = 1;
    const int nper = cdiv(N, nsplit);
    nsplit = N > 0 ? cdiv(N, nper) : 1;
    const bool vec = T > 0 && T % 4 == 0 && ((uintptr_t)x & 15) == 0 && (mask_mode == SF_MASK_NONE || ((uintptr_t)mask & 3) == 0);
    double* part_sum = (double*)workspace;
    double* part_cnt = part_sum + (long)nch * SF_MOMENT_SPLITS;
    double* center = part_cnt + (long)nch * SF_MOMENT_SPLITS;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)nsplit, nch);
    for (int stage = 0; stage < 2; ++stage) {     // an empty input walks nothing: count 0, NaN mean and std
        const double* ce = stage ? center : nullptr;
        if (vec)
            hipLaunchKernelGGL(sf_moments_kernel<4>, grid, dim3(SF_THREADS), 0, s, x, mask, mask_mode, N, F, T, f0, nper,
                               bm_fastdiv((unsigned)(T / 4)), ce, part_sum, part_cnt);
        else
            hipLaunchKernelGGL(sf_moments_kernel<1>, grid, dim3(SF_THREADS), 0, s, x, mask, mask_mode, N, F, T, f0, nper,
                               bm_fastdiv((unsigned)(T > 0 ? T : 1)), ce, part_sum, part_cnt);
        hipLaunchKernelGGL(sf_moments_fold_kernel, dim3(1), dim3(SF_THREADS), 0, s, part_sum, part_cnt, nch, (int)nsplit,
                           per_channel, stage, center, mean, std, count);
    }
    return bm_check_launch("masked_moments");
}

// ---- (c) category counts -------------------------------------------------------------------------------------------
#define SF_FLAG_NOT_INTEGER 1       // some value of X is not an integer (NaN and +-inf included)
#define SF_FLAG_MAX 2               // some value of X is >= cardinality
#define SF_FLAG_MIN 4               // min(X) != 0: a negative value, or no zero at all
#define SF_RAW_NEGATIVE 4           // (raw word of the counting launch)
#define SF_RAW_SAW_ZERO 8
template <int V>
__global__ __launch_bounds__(SF_THREADS) void sf_category_kernel(const float* __restrict__ x,
                                                                const unsigned char* __restrict__ mask, int mask_mode,
                                                                int N, int F, int T, int f, int K, int nper,
                                                                BmFastDiv div_tv, unsigned* __restrict__ counts,
                                                                unsigned* __restrict__ raw_flags) {
    extern __shared__ unsigned sh_cnt[];          // K bins
    for (int i = threadIdx.x; i < K; i += SF_THREADS) sh_cnt[i] = 0u;
    __syncthreads();
    const int n0 = blockIdx.x * nper;
    const int nn = min(N, n0 + nper) - n0;
    const unsigned Tv = (unsigned)(T / V);
    const unsigned nvec = nn > 0 ? (unsigned)nn * Tv : 0u;
    const float fK = (float)K;
    unsigned fl = 0u;
    for (unsigned base = 0; base < nvec; base += SF_THREADS) {        // block-uniform trip count (sf_lds_count)
        const unsigned j = base + threadIdx.x;
        const bool valid = j < nvec;
        float v[V];
        unsigned char m[V];
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = 0.f, m[i] = 0;
        if (valid) {
            const unsigned nl = bm_div(j, div_tv);
            const unsigned tv = j - nl * Tv;
            const size_t n = (size_t)(n0 + nl);
            sf_load<V>(x + (n * F + f) * T + (size_t)tv * V, v);
#pragma unroll
            for (int i = 0; i < V; ++i) m[i] = 1;
            if (mask_mode == SF_MASK_FULL) sf_load_mask<V>(mask + (n * F + f) * T + (size_t)tv * V, m);
            else if (mask_mode == SF_MASK_ROW) sf_load_mask<V>(mask + n * T + (size_t)tv * V, m);
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float a = v[i];
            const bool integral = a == truncf(a) && fabsf(a) < 2147483648.f;      // false for a NaN
            const bool inside = integral && a >= 0.f && a < fK;
            if (valid) {                          // the assert looks at all of X, selected or not
                fl |= integral ? 0u : SF_FLAG_NOT_INTEGER;
                fl |= a >= fK ? SF_FLAG_MAX : 0u;
                fl |= a < 0.f ? SF_RAW_NEGATIVE : 0u;
                fl |= a == 0.f ? SF_RAW_SAW_ZERO : 0u;
            }
            sf_lds_count(sh_cnt, valid && m[i] && inside ? (int)a : -1);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fl |= (unsigned)__shfl_xor((int)fl, o);
    if ((threadIdx.x & 63) == 0 && fl) atomicOr(raw_flags, fl);
    __syncthreads();
    for (int i = threadIdx.x; i < K; i += SF_THREADS) {
        const unsigned cnt = sh_cnt[i];
        if (cnt) atomicAdd(&counts[i], cnt);
    }
}

__global__ __launch_bounds__(SF_THREADS) void sf_category_fold_kernel(const unsigned* __restrict__ counts,
                                                                     const unsigned* __restrict__ raw_flags, int K,
                                                                     float* __restrict__ out, int* __restrict__ flags) {
    const int i = blockIdx.x * SF_THREADS + threadIdx.x;
    if (i < K) out[i] = (float)counts[i];         // fp32 like torch.histc
    if (i == 0) {
        const unsigned r = *raw_flags;
        const bool bad_min = (r & SF_RAW_NEGATIVE) || !(r & SF_RAW_SAW_ZERO);
        *flags = (int)((r & (SF_FLAG_NOT_INTEGER | SF_FLAG_MAX)) | (bad_min ? SF_FLAG_MIN : 0));
    }
}

// workspace (ZEROED by the caller before every call): integer counts [cardinality], then the raw flag word
extern "C" long bm_category_counts_workspace_bytes(int cardinality) {
    return cardinality < 0 ? 0 : ((long)cardinality + 4) * 4;
}

extern "C" int bm_category_counts(const float* x, const unsigned char* mask, int mask_mode, int N, int F, int T, int f,
                                  int cardinality, float* counts, int* flags, void* workspace, long workspace_bytes,
                                  void* stream) {
    BM_REQUIRE(N >= 0 && F > 0 && T >= 0 && (long)N * F * T < (1L << 31) && f >= 0 && f < F, "category_counts: bad shape");
    BM_REQUIRE(cardinality >= 1 && cardinality <= SF_MAX_CARDINALITY,
               "category_counts: cardinality %d outside [1, %d] (the histogram lives in LDS)", cardinality,
               SF_MAX_CARDINALITY);
    BM_REQUIRE(mask_mode >= SF_MASK_NONE && mask_mode <= SF_MASK_FULL && (mask_mode == SF_MASK_NONE || mask),
               "category_counts: bad mask");
    BM_REQUIRE(counts && flags, "category_counts: null pointer");
    if ((long)N * T == 0) return BM_OK;
    BM_REQUIRE(x, "category_counts: null pointer");
    if (!workspace || workspace_bytes < bm_category_counts_workspace_bytes(cardinality))
        return bm_set_error(BM_ERR_WORKSPACE, "category_counts: workspace");
    long nsplit = cdiv((long)N * T, 8192);
    if (nsplit > 512) nsplit = 512;
    if (nsplit > N) nsplit = N;
    const int nper = cdiv(N, nsplit);
    nsplit = cdiv(N, nper);
    const bool vec = T % 4 == 0 && ((uintptr_t)x & 15) == 0 && (mask_mode == SF_MASK_NONE || ((uintptr_t)mask & 3) == 0);
    unsigned* cnt = (unsigned*)workspace;
    unsigned* raw = cnt + cardinality;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)cardinality * sizeof(unsigned);
    if (vec)
        hipLaunchKernelGGL(sf_category_kernel<4>, dim3((unsigned)nsplit), dim3(SF_THREADS), lds, s, x, mask, mask_mode, N,
                           F, T, f, cardinality, nper, bm_fastdiv((unsigned)(T / 4)), cnt, raw);
    else
        hipLaunchKernelGGL(sf_category_kernel<1>, dim3((unsigned)nsplit), dim3(SF_THREADS), lds, s, x, mask, mask_mode, N,
                           F, T, f, cardinality, nper, bm_fastdiv((unsigned)T), cnt, raw);
    hipLaunchKernelGGL(sf_category_fold_kernel, dim3(cdiv(cardinality, SF_THREADS)), dim3(SF_THREADS), 0, s, cnt, raw,
                       cardinality, counts, flags);
    return bm_check_launch("category_counts");
}

// ---- (d) inverse transform -----------------------------------------------------------------------------------------
// out[b][c][t] = (x[b][c][t] * scale[group[b]][c]) + center[group[b]][c]: the multiply and the add stay two roundings,
// as the reference's two torch ops.  Same grid and grouping as center_scale_kernel (scale.hip).
template <int VEC>
__global__ void center_scale_inverse_kernel(const float* __restrict__ x, float* __restrict__ out,
                                            const long* __restrict__ group, const float* __restrict__ center,
                                            const float* __restrict__ scale, int B, int C, int T) {
    const int b = blockIdx.y;
    const long g = group ? group[b] : 0;
    const int TV = T / VEC;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < C * TV; e += gridDim.x * blockDim.x) {
        const int c = e / TV;
        const int tv = e - c * TV;
        const float ce = center[g * C + c], sc = scale[g * C + c];
        const long off = ((long)b * C + c) * T + (long)tv * VEC;
        float v[VEC];
        sf_load<VEC>(x + off, v);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
#pragma clang fp contract(off)                    // (hipcc contracts __fadd_rn(__fmul_rn(..)) into an FMA: they are plain operators in its headers)
            const float p = v[i] * sc;
            v[i] = p + ce;
        }
        if constexpr (VEC == 4) {
            *reinterpret_cast<float4*>(out + off) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            out[off] = v[0];
        }
    }
}

extern "C" int bm_center_scale_inverse(const float* x, float* out, const long* group, const float* center,
                                       const float* scale, int B, int C, int T, void* stream) {
    BM_REQUIRE(x && out && center && scale, "center_scale_inverse: null pointer");
    if ((long)B * C * T == 0) return BM_OK;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = (T % 4 == 0) && (((uintptr_t)x | (uintptr_t)out) % 16 == 0);
    const int per = vec ? C * (T / 4) : C * T;
    int bx = (per + 255) / 256;
    if (bx > 64) bx = 64;
    if (vec)
        hipLaunchKernelGGL(center_scale_inverse_kernel<4>, dim3(bx, B), dim3(256), 0, s, x, out, group, center, scale,
                           B, C, T);
    else
        hipLaunchKernelGGL(center_scale_inverse_kernel<1>, dim3(bx, B), dim3(256), 0, s, x, out, group, center, scale,
                           B, C, T);
    return bm_check_launch("center_scale_inverse");
}
