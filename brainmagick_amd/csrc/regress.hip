// Regression objective and its test metrics (bm/losses.py:11-26, bm/metrics.py:37-170).
//
//   forward   loss = sum_{selected} w(e - o) / count       w = |.| (L1) or (.)^2 (MSE)
//   backward  dEst = g * w'(e - o) * m / count, dOut = -dEst
//   metrics   per (f, t) column, over the batch: sum l r m, sum l m, sum r m, sum (l m)^2, sum (r m)^2, sum m,
//             sum ((l - r) m)^2, sum |(l - r) m|   (OnlineCorrelation, L2Reg, L1Reg with dim = 0)
//
// The mask is null (all true), [B][1][T] (broadcast over F: SegmentBatch.features_mask) or [B][F][T]; one byte per
// element, nonzero = selected.  The forward and the backward are ONE launch each: the loss' per-workgroup fp64
// partials, and the backward's per-(channel, split) maxima, are folded by the workgroup that finishes last (ticket
// counter in the caller's workspace; partials stored write-through, an agent-scope acquire in the last workgroup).  Every sum has a fixed order for a given shape: the results are bit-reproducible.
#include "bm_common.h"

#define RG_THREADS 256
#define RG_FWD_MAX_BLOCKS 1024
#define RG_BWD_MAX_PARTIALS 16384
#define RG_MASK_NONE 0
#define RG_MASK_ROW 1       // [B][1][T]
#define RG_MASK_FULL 2      // [B][F][T]
#define RG_L1 0
#define RG_MSE 1

// Workspace layout (bm_regress_workspace_bytes): two ticket counters (zero between launches: the last workgroup of a
// launch resets its counter), the forward partials (sum, count) and the backward's partial maxima.
struct RgWs {
    unsigned* tickets;      // [0]: forward, [1]: backward
    double* part_sum;       // [RG_FWD_MAX_BLOCKS]
    double* part_cnt;       // [RG_FWD_MAX_BLOCKS]
    float* part_max;        // [RG_BWD_MAX_PARTIALS], [F][nsplit]
};
static RgWs rg_ws(void* base) {
    char* p = (char*)base;
    RgWs w;
    w.tickets = (unsigned*)p;
    w.part_sum = (double*)(p + 64);
    w.part_cnt = w.part_sum + RG_FWD_MAX_BLOCKS;
    w.part_max = (float*)(w.part_cnt + RG_FWD_MAX_BLOCKS);
    return w;
}
static const long RG_WS_BYTES = 64 + 2L * RG_FWD_MAX_BLOCKS * 8 + RG_BWD_MAX_PARTIALS * 4L;

extern "C" long bm_regress_workspace_bytes(void) { return RG_WS_BYTES; }

template <int V> struct RgVec;
template <> struct RgVec<1> {
    typedef float F;
    typedef unsigned char M;
};
template <> struct RgVec<4> {
    typedef f32x4 F;
    typedef uchar4 M;
};
__device__ __forceinline__ float rg_get(const float& v, int) { return v; }
__device__ __forceinline__ float rg_get(const f32x4& v, int i) { return v[i]; }
__device__ __forceinline__ unsigned char rg_get(const unsigned char& v, int) { return v; }
__device__ __forceinline__ unsigned char rg_get(const uchar4& v, int i) {
    return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}
__device__ __forceinline__ void rg_set(float& v, int, float x) { v = x; }
__device__ __forceinline__ void rg_set(f32x4& v, int i, float x) { v[i] = x; }

// Thread 0 stores its workgroup's partial write-through (sc1: no agent-scope release needed -- a release would write
// back the whole XCD L2, which the backward has just filled with dEst), waits for the store, draws a ticket; returns
// true in every thread of the workgroup that finished last, after the acquire that makes the other workgroups'
// partials visible to it.  `sh_flag` lives in the kernel's one LDS array.
template <typename P>
__device__ __forceinline__ void rg_store_partial(P* dst, P v) {
    __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool rg_last_arriver(unsigned* ticket, unsigned nblocks, double* sh_flag) {
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = prev == nblocks - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        }
        *sh_flag = last ? 1.0 : 0.0;
    }
    __syncthreads();
    return *sh_flag != 0.0;
}

// fixed-order block sum of a double (4 wavefronts); sh: >= 4 doubles; returns the sum in every thread
__device__ __forceinline__ double rg_block_sum(double v, double* sh) {
    v = bm_wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return v;
}

// ---- forward: one launch, grid-stride over vectors of V elements (V = 4 when T % 4 == 0) ----------------------------
template <int V>
__global__ __launch_bounds__(RG_THREADS) void regress_fwd_kernel(const float* __restrict__ est,
                                                                 const float* __restrict__ out,
                                                                 const unsigned char* __restrict__ mask, int mask_mode,
                                                                 unsigned nvec, unsigned Tv, BmFastDiv div_tv,
                                                                 BmFastDiv div_f, int kind, RgWs ws,
                                                                 float* __restrict__ loss, double* __restrict__ count,
                                                                 int* __restrict__ flag) {
    typedef typename RgVec<V>::F FV;
    typedef typename RgVec<V>::M MV;
    __shared__ double sh[9];
    double s = 0.0, c = 0.0;
    for (unsigned j = blockIdx.x * RG_THREADS + threadIdx.x; j < nvec; j += gridDim.x * RG_THREADS) {
        const FV e = ((const FV*)est)[j];
        const FV o = ((const FV*)out)[j];
        MV m;
        if (mask_mode == RG_MASK_FULL) {
            m = ((const MV*)mask)[j];
        } else if (mask_mode == RG_MASK_ROW) {
            const unsigned row = bm_div(j, div_tv);            // b * F + f
            const unsigned b = bm_div(row, div_f);
            m = ((const MV*)mask)[b * Tv + (j - row * Tv)];
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const bool sel = mask_mode == RG_MASK_NONE || rg_get(m, i) != 0;
            const double d = (double)(rg_get(e, i) - rg_get(o, i));      // the fp32 difference, as torch forms it
            const double w = kind == RG_L1 ? fabs(d) : d * d;
            s += sel ? w : 0.0;
            c += sel ? 1.0 : 0.0;
        }
    }
    s = rg_block_sum(s, sh);
    c = rg_block_sum(c, sh + 4);
    if (threadIdx.x == 0) {
        rg_store_partial(ws.part_sum + blockIdx.x, s);
        rg_store_partial(ws.part_cnt + blockIdx.x, c);
    }
    if (!rg_last_arriver(ws.tickets + 0, gridDim.x, sh + 8)) return;
    // the last workgroup folds the partials in block order
    s = 0.0;
    c = 0.0;
    for (unsigned k = threadIdx.x; k < gridDim.x; k += RG_THREADS) {
        s += ws.part_sum[k];
        c += ws.part_cnt[k];
    }
    s = rg_block_sum(s, sh);
    c = rg_block_sum(c, sh + 4);
    if (threadIdx.x == 0) {
        *loss = (float)(s / c);                       // count == 0: 0 / 0 = NaN, like torch's mean of nothing
        *count = c;
        if (c == 0.0 && flag) atomicOr(flag, 2);      // bm/solver.py:354-356 "no mask!"
    }
}

extern "C" int bm_regress_loss_fwd(const float* est, const float* out, const unsigned char* mask, int mask_mode,
                                   int B, int F, int T, int kind, float* loss, double* count, void* workspace,
                                   long workspace_bytes, int* flag, void* stream) {
    BM_REQUIRE(B >= 0 && F > 0 && T > 0 && (long)B * F * T < (1L << 31), "regress_loss_fwd: bad shape");
    BM_REQUIRE(mask_mode >= RG_MASK_NONE && mask_mode <= RG_MASK_FULL && (mask_mode == RG_MASK_NONE || mask),
               "regress_loss_fwd: bad mask");
    BM_REQUIRE(kind == RG_L1 || kind == RG_MSE, "regress_loss_fwd: kind must be 0 (L1) or 1 (MSE)");
    BM_REQUIRE(loss && count && (est && out || B == 0), "regress_loss_fwd: null pointer");
    if (!workspace || workspace_bytes < RG_WS_BYTES) return bm_set_error(BM_ERR_WORKSPACE, "regress_loss_fwd: workspace");
    const long n = (long)B * F * T;
    const bool vec = T % 4 == 0 && (((uintptr_t)est | (uintptr_t)out) & 15) == 0 &&
                     (mask_mode == RG_MASK_NONE || ((uintptr_t)mask & 3) == 0);
    const int V = vec ? 4 : 1;
    const unsigned nvec = (unsigned)(n / V), Tv = (unsigned)(T / V);
    int blocks = cdiv(nvec, RG_THREADS * 8);
    blocks = blocks < 1 ? 1 : blocks > RG_FWD_MAX_BLOCKS ? RG_FWD_MAX_BLOCKS : blocks;
    const RgWs ws = rg_ws(workspace);
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(regress_fwd_kernel<4>, dim3(blocks), dim3(RG_THREADS), 0, s, est, out, mask, mask_mode, nvec,
                           Tv, bm_fastdiv(Tv), bm_fastdiv((unsigned)F), kind, ws, loss, count, flag);
    else
        hipLaunchKernelGGL(regress_fwd_kernel<1>, dim3(blocks), dim3(RG_THREADS), 0, s, est, out, mask, mask_mode, nvec,
                           Tv, bm_fastdiv(Tv), bm_fastdiv((unsigned)F), kind, ws, loss, count, flag);
    return bm_check_launch("regress_loss_fwd");
}

// ---- backward: workgroup (split, f) walks the rows (b, f) of its batch range -----------------------------------------
// With amax_out (compute mode f16x2) the workgroup stores max |dEst| of its rows; the last workgroup folds the
// [F][nsplit] maxima into amax_rows_out[f] and the tensor's amax slot: the consumers of dEst need no bm_amax pass.
template <int V>
__global__ __launch_bounds__(RG_THREADS) void regress_bwd_kernel(const float* __restrict__ est,
                                                                 const float* __restrict__ out,
                                                                 const unsigned char* __restrict__ mask, int mask_mode,
                                                                 int B, int F, int T, int bper, BmFastDiv div_tv,
                                                                 int kind, const float* __restrict__ grad_out,
                                                                 const double* __restrict__ count,
                                                                 float* __restrict__ d_est, float* __restrict__ d_out,
                                                                 float* __restrict__ amax_out,
                                                                 float* __restrict__ amax_rows_out, RgWs ws) {
    typedef typename RgVec<V>::F FV;
    typedef typename RgVec<V>::M MV;
    __shared__ double sh[9];
    const int split = blockIdx.x, f = blockIdx.y, nsplit = gridDim.x;
    const int b0 = split * bper;
    const int nb = min(B, b0 + bper) - b0;
    const unsigned Tv = (unsigned)(T / V);
    const float g = *grad_out;
    const double cnt = *count;
    // torch: L1 = mean(|d|) -> sign(d) * (g / N); MSE -> d * (2 / N) * g
    const float scale = kind == RG_L1 ? g / (float)cnt : (float)(2.0 / cnt);
    float mx = 0.f;
    const unsigned nvec = nb > 0 ? (unsigned)nb * Tv : 0u;
    for (unsigned j = threadIdx.x; j < nvec; j += RG_THREADS) {
        const unsigned bl = bm_div(j, div_tv);
        const unsigned tv = j - bl * Tv;
        const unsigned b = (unsigned)b0 + bl;
        const size_t idx = ((size_t)b * F + f) * Tv + tv;           // in vectors
        const FV e = ((const FV*)est)[idx];
        const FV o = ((const FV*)out)[idx];
        MV m;
        if (mask_mode == RG_MASK_FULL) m = ((const MV*)mask)[idx];
        else if (mask_mode == RG_MASK_ROW) m = ((const MV*)mask)[(size_t)b * Tv + tv];
        FV r;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const bool sel = mask_mode == RG_MASK_NONE || rg_get(m, i) != 0;
            const float d = rg_get(e, i) - rg_get(o, i);
            float v;
            if (kind == RG_L1) v = d > 0.f ? scale : d < 0.f ? -scale : 0.f;   // torch's sign: (0 < d) - (d < 0), 0 for 0 AND for NaN
            else v = d * scale * g;
            v = sel ? v : 0.f;
            rg_set(r, i, v);
            mx = fmaxf(mx, fabsf(v));
        }
        ((FV*)d_est)[idx] = r;
        if (d_out) ((FV*)d_out)[idx] = -r;
    }
    if (!amax_out) return;                            // kernel argument: uniform
    float* shf = (float*)sh;
    mx = bm_wave_max(mx);
    if ((threadIdx.x & 63) == 0) shf[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) rg_store_partial(ws.part_max + f * nsplit + split, fmaxf(fmaxf(shf[0], shf[1]), fmaxf(shf[2], shf[3])));
    __syncthreads();
    if (!rg_last_arriver(ws.tickets + 1, gridDim.x * gridDim.y, sh + 8)) return;
    float all = 0.f;
    for (int c = threadIdx.x; c < F; c += RG_THREADS) {
        float v = 0.f;
        for (int k = 0; k < nsplit; ++k) v = fmaxf(v, ws.part_max[c * nsplit + k]);
        if (amax_rows_out) amax_rows_out[c] = v;
        all = fmaxf(all, v);
    }
    all = bm_wave_max(all);
    if ((threadIdx.x & 63) == 0) shf[threadIdx.x >> 6] = all;
    __syncthreads();
    if (threadIdx.x < BM_AMAX_SHARDS)
        amax_out[threadIdx.x] = threadIdx.x == 0 ? fmaxf(fmaxf(shf[0], shf[1]), fmaxf(shf[2], shf[3])) : 0.f;
}

extern "C" int bm_regress_loss_bwd(const float* est, const float* out, const unsigned char* mask, int mask_mode,
                                   int B, int F, int T, int kind, const float* grad_out, const double* count,
                                   float* d_est, float* d_out, float* amax_out, float* amax_rows_out, void* workspace,
                                   long workspace_bytes, void* stream) {
    BM_REQUIRE(B >= 0 && F > 0 && T > 0 && (long)B * F * T < (1L << 31), "regress_loss_bwd: bad shape");
    BM_REQUIRE(mask_mode >= RG_MASK_NONE && mask_mode <= RG_MASK_FULL && (mask_mode == RG_MASK_NONE || mask),
               "regress_loss_bwd: bad mask");
    BM_REQUIRE(kind == RG_L1 || kind == RG_MSE, "regress_loss_bwd: kind must be 0 (L1) or 1 (MSE)");
    BM_REQUIRE(grad_out && count && (B == 0 || (est && out && d_est)), "regress_loss_bwd: null pointer");
    BM_REQUIRE(!amax_rows_out || amax_out, "regress_loss_bwd: amax_rows_out needs amax_out");
    if (amax_out && (!workspace || workspace_bytes < RG_WS_BYTES))
        return bm_set_error(BM_ERR_WORKSPACE, "regress_loss_bwd: workspace");
    if (B == 0) return BM_OK;
    // ~2 048 workgroups: nsplit batch ranges per channel (F * nsplit partial maxima fit the workspace)
    int nsplit = cdiv(2048, F);
    nsplit = nsplit > B ? B : nsplit;
    if (amax_out && F * nsplit > RG_BWD_MAX_PARTIALS) nsplit = RG_BWD_MAX_PARTIALS / F;
    if (nsplit < 1) return bm_set_error(BM_ERR_UNSUPPORTED, "regress_loss_bwd: F = %d exceeds %d with amax_out", F,
                                        RG_BWD_MAX_PARTIALS);
    const int bper = cdiv(B, nsplit);
    nsplit = cdiv(B, bper);
    const bool vec = T % 4 == 0 && (((uintptr_t)est | (uintptr_t)out | (uintptr_t)d_est | (uintptr_t)d_out) & 15) == 0 &&
                     (mask_mode == RG_MASK_NONE || ((uintptr_t)mask & 3) == 0);
    const RgWs ws = amax_out ? rg_ws(workspace) : RgWs{nullptr, nullptr, nullptr, nullptr};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(nsplit, F);
    if (vec)
        hipLaunchKernelGGL(regress_bwd_kernel<4>, grid, dim3(RG_THREADS), 0, s, est, out, mask, mask_mode, B, F, T, bper,
                           bm_fastdiv((unsigned)(T / 4)), kind, grad_out, count, d_est, d_out, amax_out, amax_rows_out, ws);
    else
        hipLaunchKernelGGL(regress_bwd_kernel<1>, grid, dim3(RG_THREADS), 0, s, est, out, mask, mask_mode, B, F, T, bper,
                           bm_fastdiv((unsigned)T), kind, grad_out, count, d_est, d_out, amax_out, amax_rows_out, ws);
    return bm_check_launch("regress_loss_bwd");
}

// ---- test metrics: one thread per (f, t) column of the window [t0, T), walking b in order ----------------------------
// acc: 8 planes of [F][T - t0] doubles, accumulated in place (sum l r m, sum l m, sum r m, sum (l m)^2, sum (r m)^2,
// sum m, sum ((l - r) m)^2, sum |(l - r) m|).  Rows of est / out are T floats apart, segments *_bstride floats; the
// mask is [B][1][T] (mask_full = 0) or [B][F][T] (mask_full = 1), segments mask_bstride bytes apart, or null.
#define RG_METRIC_UNROLL 8
__global__ __launch_bounds__(RG_THREADS) void regress_metric_kernel(const float* __restrict__ est, long est_bstride,
                                                                    const float* __restrict__ out, long out_bstride,
                                                                    const unsigned char* __restrict__ mask,
                                                                    long mask_bstride, int mask_full, int B, int F,
                                                                    int T, int t0, double* __restrict__ acc) {
    const int Tw = T - t0;
    const long ncol = (long)F * Tw;
    const long col = (long)blockIdx.x * RG_THREADS + threadIdx.x;
    if (col >= ncol) return;
    const int f = (int)(col / Tw), t = t0 + (int)(col - (long)f * Tw);
    const long off = (long)f * T + t;
    const long moff = mask_full ? off : t;
    double sdot = 0.0, sl = 0.0, sr = 0.0, sll = 0.0, srr = 0.0, sm = 0.0, sl2 = 0.0, sl1 = 0.0;
    for (int b0 = 0; b0 < B; b0 += RG_METRIC_UNROLL) {
        float lv[RG_METRIC_UNROLL], rv[RG_METRIC_UNROLL];
        unsigned char mv[RG_METRIC_UNROLL];
#pragma unroll
        for (int i = 0; i < RG_METRIC_UNROLL; ++i) {          // loads first: eight segments in flight
            const int b = b0 + i < B ? b0 + i : B - 1;
            lv[i] = est[b * est_bstride + off];
            rv[i] = out[b * out_bstride + off];
            mv[i] = mask ? mask[b * mask_bstride + moff] : 1;
        }
#pragma unroll
        for (int i = 0; i < RG_METRIC_UNROLL; ++i) {          // then the sums, in segment order
            if (b0 + i >= B) break;
            const double m = mv[i] ? 1.0 : 0.0;
            const double l = lv[i], r = rv[i];
            const double lm = l * m, rm = r * m, dm = (l - r) * m;
            sdot += l * r * m;
            sl += lm;
            sr += rm;
            sll += lm * lm;
            srr += rm * rm;
            sm += m;
            sl2 += dm * dm;
            sl1 += fabs(dm);
        }
    }
    acc[0 * ncol + col] += sdot;
    acc[1 * ncol + col] += sl;
    acc[2 * ncol + col] += sr;
    acc[3 * ncol + col] += sll;
    acc[4 * ncol + col] += srr;
    acc[5 * ncol + col] += sm;
    acc[6 * ncol + col] += sl2;
    acc[7 * ncol + col] += sl1;
}

extern "C" int bm_regress_metric_update(const float* est, long est_bstride, const float* out, long out_bstride,
                                        const unsigned char* mask, long mask_bstride, int mask_full, int B, int F,
                                        int T, int t0, double* acc, void* stream) {
    BM_REQUIRE(B >= 0 && F > 0 && T > 0 && t0 >= 0 && t0 < T && acc, "regress_metric_update: bad arguments");
    BM_REQUIRE(B == 0 || (est && out), "regress_metric_update: null pointer");
    if (B == 0) return BM_OK;
    const long ncol = (long)F * (T - t0);
    hipLaunchKernelGGL(regress_metric_kernel, dim3(cdiv(ncol, RG_THREADS)), dim3(RG_THREADS), 0, (hipStream_t)stream,
                       est, est_bstride, out, out_bstride, mask, mask_bstride, mask_full, B, F, T, t0, acc);
    return bm_check_launch("regress_metric_update");
}
