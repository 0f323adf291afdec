// Regression objective and its test metrics (bm/losses.py:11-26, bm/metrics.py:37-170); further down FeatureDecodingLoss
// (bm/losses.py:117-173) and ClassificationAcc (bm/metrics.py:173-180) on the same helpers and workspace.
//
//   forward   loss = sum_{selected} w(e - o) / count       w = |.| (L1) or (.)^2 (MSE)
//   backward  dEst = g * w'(e - o) * m / count, dOut = -dEst
//   metrics   per (f, t) column, over the batch: sum l r m, sum l m, sum r m, sum (l m)^2, sum (r m)^2, sum m,
//             sum ((l - r) m)^2, sum |(l - r) m|   (OnlineCorrelation, L2Reg, L1Reg with dim = 0)
//
// The mask is null (all true), [B][1][T] (broadcast over F: SegmentBatch.features_mask) or [B][F][T]; one byte per
// element, nonzero = selected.  The forward and the backward are ONE launch each: the loss' per-workgroup fp64
// partials, and the backward's per-(channel, split) maxima, are folded by the workgroup that finishes last (bm_block.h:
// ticket counter in the caller's workspace; partials stored write-through, an agent-scope acquire in the last
// workgroup).  Every sum has a fixed order for a given shape: the results are bit-reproducible.
#include "bm_block.h"

#define RG_THREADS 256
#define RG_FWD_MAX_BLOCKS 1024
#define RG_BWD_MAX_PARTIALS 16384
#define RG_MASK_NONE 0
#define RG_MASK_ROW 1       // [B][1][T]
#define RG_MASK_FULL 2      // [B][F][T]
#define RG_L1 0
#define RG_MSE 1
#define FD_MAX_FEATURES 16
#define FD_MAX_K 16384
#define FD_MAX_BLOCKS 2048
#define FD_SLOTS (FD_MAX_FEATURES + 1)      // one (numerator, denominator) pair per feature + the selected positions

// Workspace layout (bm_regress_workspace_bytes): three ticket counters (zero between launches: the last workgroup of a
// launch resets its counter), the forward partials (sum, count), the backward's partial maxima and the per-feature
// partials of the feature-decoding forward.
struct RgWs {
    unsigned* tickets;      // [0]: forward, [1]: backward, [2]: feature-decoding forward
    double* part_sum;       // [RG_FWD_MAX_BLOCKS]
    double* part_cnt;       // [RG_FWD_MAX_BLOCKS]
    float* part_max;        // [RG_BWD_MAX_PARTIALS], [F][nsplit]
    double* part_fd;        // [FD_SLOTS][2][FD_MAX_BLOCKS]
};
static RgWs rg_ws(void* base) {
    const BmFoldWs<double> head = BmFoldWs<double>::at(base);
    RgWs w;
    w.tickets = head.tickets;
    w.part_sum = head.part;
    w.part_cnt = w.part_sum + RG_FWD_MAX_BLOCKS;
    w.part_max = (float*)(w.part_cnt + RG_FWD_MAX_BLOCKS);
    w.part_fd = (double*)(w.part_max + RG_BWD_MAX_PARTIALS);
    return w;
}
static const long RG_WS_BYTES = BmFoldWs<double>::bytes(2L * RG_FWD_MAX_BLOCKS) + RG_BWD_MAX_PARTIALS * 4L +
                                2L * FD_SLOTS * FD_MAX_BLOCKS * 8;

extern "C" long bm_regress_workspace_bytes(void) { return RG_WS_BYTES; }

#define RG_WAVES (RG_THREADS / 64)
typedef BmFoldLds<double, RG_WAVES, 2> RgSumLds;          // two sums at a time: (numerator, denominator)

// ---- forward: one launch, grid-stride over vectors of V elements (V = 4 when T % 4 == 0) ----------------------------
template <int V>
__global__ __launch_bounds__(RG_THREADS) void regress_fwd_kernel(const float* __restrict__ est,
                                                                 const float* __restrict__ out,
                                                                 const unsigned char* __restrict__ mask, int mask_mode,
                                                                 unsigned nvec, unsigned Tv, BmFastDiv div_tv,
                                                                 BmFastDiv div_f, int kind, RgWs ws,
                                                                 float* __restrict__ loss, double* __restrict__ count,
                                                                 int* __restrict__ flag) {
    typedef typename BmVec<V>::F FV;
    typedef typename BmVec<V>::M MV;
    __shared__ RgSumLds sh;
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
            const bool sel = mask_mode == RG_MASK_NONE || bm_get(m, i) != 0;
            const double d = (double)(bm_get(e, i) - bm_get(o, i));      // the fp32 difference, as torch forms it
            const double w = kind == RG_L1 ? fabs(d) : d * d;
            s += sel ? w : 0.0;
            c += sel ? 1.0 : 0.0;
        }
    }
    s = bm_block_sum<RG_WAVES>(s, sh.wave[0]);
    c = bm_block_sum<RG_WAVES>(c, sh.wave[1]);
    if (threadIdx.x == 0) {
        bm_store_partial(ws.part_sum + blockIdx.x, s);
        bm_store_partial(ws.part_cnt + blockIdx.x, c);
    }
    if (!bm_last_arriver(ws.tickets + 0, gridDim.x, &sh.last)) return;
    // the last workgroup folds the partials in block order
    s = 0.0;
    c = 0.0;
    for (unsigned k = threadIdx.x; k < gridDim.x; k += RG_THREADS) {
        s += ws.part_sum[k];
        c += ws.part_cnt[k];
    }
    s = bm_block_sum<RG_WAVES>(s, sh.wave[0]);
    c = bm_block_sum<RG_WAVES>(c, sh.wave[1]);
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
    typedef typename BmVec<V>::F FV;
    typedef typename BmVec<V>::M MV;
    __shared__ BmFoldLds<float, RG_WAVES> sh;
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
            const bool sel = mask_mode == RG_MASK_NONE || bm_get(m, i) != 0;
            const float d = bm_get(e, i) - bm_get(o, i);
            float v;
            if (kind == RG_L1) v = d > 0.f ? scale : d < 0.f ? -scale : 0.f;   // torch's sign: (0 < d) - (d < 0), 0 for 0 AND for NaN
            else v = d * scale * g;
            v = sel ? v : 0.f;
            bm_set(r, i, v);
            mx = fmaxf(mx, fabsf(v));
        }
        ((FV*)d_est)[idx] = r;
        if (d_out) ((FV*)d_out)[idx] = -r;
    }
    if (!amax_out) return;                            // kernel argument: uniform
    if (!bm_amax_arrive(mx, ws.part_max + f * nsplit + split, ws.tickets + 1, gridDim.x * gridDim.y, sh)) return;
    bm_amax_fold_rows<RG_WAVES>(ws.part_max, F, nsplit, nsplit, 1, amax_out, amax_rows_out, sh.wave[0]);
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
    const RgWs ws = amax_out ? rg_ws(workspace) : RgWs{nullptr, nullptr, nullptr, nullptr, nullptr};
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

// ---- FeatureDecodingLoss (bm/losses.py:117-173): MSE on the continuous features, weighted cross-entropy on the
// categorical ones, all features in ONE forward and ONE backward launch ------------------------------------------------
// A workgroup owns tiles of 64 consecutive positions (b, t) of the flat [B][T] axis; its four wavefronts share the
// channels of a feature (wavefront w takes the channels w, w + 4, ...), so every load is 64 consecutive floats of one
// channel row.  The feature loop is the outer one: a thread carries the numerator / denominator of one feature at a
// time (no per-thread table).  A categorical feature's logits are read once: every wavefront keeps a running maximum
// and an fp64 sum of exponentials over its share of the K classes, the four pairs are merged through LDS.
#define FD_CONTINUOUS 0
#define FD_CATEGORICAL 1
#define FD_RANGE_BIT 4          // flag word: a category outside [0, K)  (the assert of bm/losses.py:150)
#define FD_NO_MASK_BIT 2
#define FD_TILE 64
#define FD_UNROLL 8
#define FD_BWD_MAX_TILES 16384
struct FdFeature {
    int kind, est_start, width, out_start, weight_off;
};
struct FdTable {
    int n;
    FdFeature f[FD_MAX_FEATURES];
};

struct FdPos {
    unsigned idx, b, t;     // flat position (clamped into range), segment, sample
    bool in, sel;           // inside [0, B T); selected by the mask
};
__device__ __forceinline__ FdPos fd_pos(unsigned tile, unsigned npos, unsigned T, const BmFastDiv& div_t,
                                        const unsigned char* __restrict__ mask) {
    FdPos p;
    const unsigned i = tile * FD_TILE + (threadIdx.x & 63);
    p.in = i < npos;
    p.idx = p.in ? i : npos - 1;        // lanes past the end read the last position and count for nothing
    p.b = bm_div(p.idx, div_t);
    p.t = p.idx - p.b * T;
    p.sel = p.in && (!mask || mask[p.idx] != 0);       // mask [B][1][T]: the flat position is its index
    return p;
}
__device__ __forceinline__ double* fd_part(const RgWs& ws, int slot, int which) {
    return ws.part_fd + ((size_t)slot * 2 + which) * FD_MAX_BLOCKS;
}
// the target class of a position: truncation towards zero like torch's .long(); valid inside [0, K)
__device__ __forceinline__ bool fd_target(float tv, int K, int& y) {
    const bool valid = tv > -1.f && tv < (float)K;      // false for NaN
    y = valid ? (int)tv : 0;
    return valid;
}

__global__ __launch_bounds__(RG_THREADS) void feature_decoding_fwd_kernel(
    const float* __restrict__ est, const float* __restrict__ out, const unsigned char* __restrict__ mask,
    const float* __restrict__ weights, FdTable tab, unsigned npos, unsigned ntiles, int C, int Co, unsigned T,
    BmFastDiv div_t, RgWs ws, float* __restrict__ loss, float* __restrict__ terms, double* __restrict__ denoms,
    float* __restrict__ lse, int* __restrict__ flag) {
    __shared__ struct {
        RgSumLds sums;
        double s[RG_THREADS], m[RG_THREADS];      // a categorical feature's running (sum, maximum) of every thread
    } sh;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int bad = 0;
    double cnt = 0.0;
    if (wave == 0)
        for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
            cnt += fd_pos(tile, npos, T, div_t, mask).sel ? 1.0 : 0.0;
    cnt = bm_block_sum<RG_WAVES>(cnt, sh.sums.wave[0]);
    if (threadIdx.x == 0) bm_store_partial(fd_part(ws, FD_MAX_FEATURES, 0) + blockIdx.x, cnt);
    int ci = 0;
    for (int f = 0; f < tab.n; ++f) {
        const FdFeature ft = tab.f[f];
        double num = 0.0, den = 0.0;
        if (ft.kind == FD_CONTINUOUS) {
            for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
                const FdPos p = fd_pos(tile, npos, T, div_t, mask);
                const float* e = est + ((size_t)p.b * C + ft.est_start) * T + p.t;
                const float* o = out + ((size_t)p.b * Co + ft.out_start) * T + p.t;
                double s = 0.0;
                for (int c0 = wave; c0 < ft.width; c0 += 4 * FD_UNROLL) {
                    float ev[FD_UNROLL], ov[FD_UNROLL];
#pragma unroll
                    for (int i = 0; i < FD_UNROLL; ++i) {          // loads first: eight channel rows in flight
                        const int c = c0 + 4 * i < ft.width ? c0 + 4 * i : c0;
                        ev[i] = e[(size_t)c * T];
                        ov[i] = o[(size_t)c * T];
                    }
#pragma unroll
                    for (int i = 0; i < FD_UNROLL; ++i) {
                        const double d = (double)(ev[i] - ov[i]);  // the fp32 difference, as torch forms it
                        s += c0 + 4 * i < ft.width ? d * d : 0.0;
                    }
                }
                num += p.sel ? s : 0.0;
            }
        } else {
            const int K = ft.width;
            for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
                const FdPos p = fd_pos(tile, npos, T, div_t, mask);
                const float* x = est + ((size_t)p.b * C + ft.est_start) * T + p.t;
                // running maximum m and s = sum exp(x - m') with m' = m, or 0 while m is still -inf
                float m = -INFINITY;
                double s = 0.0;
                for (int k0 = wave; k0 < K; k0 += 4 * FD_UNROLL) {
                    float xv[FD_UNROLL];
#pragma unroll
                    for (int i = 0; i < FD_UNROLL; ++i) xv[i] = x[(size_t)(k0 + 4 * i < K ? k0 + 4 * i : k0) * T];
                    float cm = m;
#pragma unroll
                    for (int i = 0; i < FD_UNROLL; ++i) cm = k0 + 4 * i < K ? fmaxf(cm, xv[i]) : cm;
                    const float base = cm == -INFINITY ? 0.f : cm;
                    s *= m == -INFINITY ? 1.0 : (double)expf(m - base);      // (no maximum yet: s is 0, or NaN)
#pragma unroll
                    for (int i = 0; i < FD_UNROLL; ++i) s += k0 + 4 * i < K ? (double)expf(xv[i] - base) : 0.0;
                    m = cm;
                }
                sh.m[threadIdx.x] = (double)m;
                sh.s[threadIdx.x] = s;
                __syncthreads();
                if (wave == 0) {
                    float mw[4];
#pragma unroll
                    for (int w = 0; w < 4; ++w) mw[w] = (float)sh.m[w * 64 + lane];
                    const float mx = fmaxf(fmaxf(mw[0], mw[1]), fmaxf(mw[2], mw[3]));
                    const float base = mx == -INFINITY ? 0.f : mx;
                    double S = 0.0;
#pragma unroll
                    for (int w = 0; w < 4; ++w)
                        S += sh.s[w * 64 + lane] * (mw[w] == -INFINITY ? 1.0 : (double)expf(mw[w] - base));
                    const double l = (double)base + log(S);
                    const float tv = out[((size_t)p.b * Co + ft.out_start) * T + p.t];
                    int y;
                    const bool valid = fd_target(tv, K, y);
                    if (p.in && (tv >= (float)K || (p.sel && !valid))) bad = 1;
                    const float xy = x[(size_t)y * T];
                    const float w = ft.weight_off >= 0 ? weights[ft.weight_off + y] : 1.f;
                    if (p.in) lse[(size_t)ci * npos + p.idx] = (float)l;
                    const bool on = p.sel && valid;
                    num += on ? (double)w * (l - (double)xy) : 0.0;
                    den += on ? (double)w : 0.0;
                }
                __syncthreads();
            }
            ++ci;
        }
        num = bm_block_sum<RG_WAVES>(num, sh.sums.wave[0]);
        den = bm_block_sum<RG_WAVES>(den, sh.sums.wave[1]);
        if (threadIdx.x == 0) {
            bm_store_partial(fd_part(ws, f, 0) + blockIdx.x, num);
            bm_store_partial(fd_part(ws, f, 1) + blockIdx.x, den);
        }
    }
    const int any_bad = __syncthreads_or(bad);
    if (any_bad && flag && threadIdx.x == 0) atomicOr(flag, FD_RANGE_BIT);
    if (!bm_last_arriver(ws.tickets + 2, gridDim.x, &sh.sums.last)) return;
    // the last workgroup folds the partials in block order, feature by feature
    double nsel = 0.0;
    for (unsigned k = threadIdx.x; k < gridDim.x; k += RG_THREADS) nsel += fd_part(ws, FD_MAX_FEATURES, 0)[k];
    nsel = bm_block_sum<RG_WAVES>(nsel, sh.sums.wave[0]);
    float total = 0.f;
    for (int f = 0; f < tab.n; ++f) {
        double num = 0.0, den = 0.0;
        for (unsigned k = threadIdx.x; k < gridDim.x; k += RG_THREADS) {
            num += fd_part(ws, f, 0)[k];
            den += fd_part(ws, f, 1)[k];
        }
        num = bm_block_sum<RG_WAVES>(num, sh.sums.wave[0]);
        den = bm_block_sum<RG_WAVES>(den, sh.sums.wave[1]);
        if (tab.f[f].kind == FD_CONTINUOUS) den = nsel * (double)tab.f[f].width;
        if (threadIdx.x == 0) {
            const float term = (float)(num / den);    // nothing selected: 0 / 0 = NaN, like torch's mean of nothing
            terms[f] = term;
            denoms[f] = den;
            total += term;                            // fp32, in feature order (the reference's `loss += ...`)
        }
    }
    if (threadIdx.x == 0) {
        *loss = total;
        if (nsel == 0.0 && flag) atomicOr(flag, FD_NO_MASK_BIT);
    }
}

// Every element of d_est is written exactly once (zero where the mask does not select): blockIdx.y splits the
// channels of every feature further (wavefront w of slice s takes the channels 4 s + w, 4 (s + gridDim.y) + w, ...).
__global__ __launch_bounds__(RG_THREADS) void feature_decoding_bwd_kernel(
    const float* __restrict__ est, const float* __restrict__ out, const unsigned char* __restrict__ mask,
    const float* __restrict__ weights, FdTable tab, unsigned npos, unsigned ntiles, int C, int Co, unsigned T,
    BmFastDiv div_t, const float* __restrict__ grad_out, const double* __restrict__ denoms,
    const float* __restrict__ lse, float* __restrict__ d_est) {
    const int first = (int)(threadIdx.x >> 6) + 4 * (int)blockIdx.y, step = 4 * (int)gridDim.y;
    const float g = *grad_out;
    int ci = 0;
    for (int f = 0; f < tab.n; ++f) {
        const FdFeature ft = tab.f[f];
        const double den = denoms[f];
        if (ft.kind == FD_CONTINUOUS) {
            const float scale = (float)(2.0 / den);        // torch: d * (2 / N) * g
            for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
                const FdPos p = fd_pos(tile, npos, T, div_t, mask);
                const size_t at = ((size_t)p.b * C + ft.est_start) * T + p.t;
                const float* o = out + ((size_t)p.b * Co + ft.out_start) * T + p.t;
                for (int c0 = first; c0 < ft.width; c0 += step * FD_UNROLL) {
                    float ev[FD_UNROLL], ov[FD_UNROLL];
#pragma unroll
                    for (int i = 0; i < FD_UNROLL; ++i) {
                        const int c = c0 + step * i < ft.width ? c0 + step * i : c0;
                        ev[i] = est[at + (size_t)c * T];
                        ov[i] = o[(size_t)c * T];
                    }
#pragma unroll
                    for (int i = 0; i < FD_UNROLL; ++i) {
                        const int c = c0 + step * i;
                        if (c < ft.width && p.in) d_est[at + (size_t)c * T] = p.sel ? (ev[i] - ov[i]) * scale * g : 0.f;
                    }
                }
            }
        } else {
            const int K = ft.width;
            for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
                const FdPos p = fd_pos(tile, npos, T, div_t, mask);
                const size_t at = ((size_t)p.b * C + ft.est_start) * T + p.t;
                int y;
                const bool on = fd_target(out[((size_t)p.b * Co + ft.out_start) * T + p.t], K, y) && p.sel;
                const float w = ft.weight_off >= 0 ? weights[ft.weight_off + y] : 1.f;
                const float coef = g * (float)((double)w / den);
                const float l = lse[(size_t)ci * npos + p.idx];
                for (int k0 = first; k0 < K; k0 += step * FD_UNROLL) {
                    float xv[FD_UNROLL];
#pragma unroll
                    for (int i = 0; i < FD_UNROLL; ++i)
                        xv[i] = est[at + (size_t)(k0 + step * i < K ? k0 + step * i : k0) * T];
#pragma unroll
                    for (int i = 0; i < FD_UNROLL; ++i) {
                        const int k = k0 + step * i;
                        const float v = coef * (expf(xv[i] - l) - (k == y ? 1.f : 0.f));
                        if (k < K && p.in) d_est[at + (size_t)k * T] = on ? v : 0.f;
                    }
                }
            }
            ++ci;
        }
    }
}

// The launcher's copy of the caller's table [n][5] = {kind, est_start, width, out_start, weight_off}: the features
// must tile the channels of est (continuous: width, categorical: K) and of out (continuous: width, categorical: 1)
// in order -- that is what lets the backward write every element of d_est exactly once.
static int fd_table(const char* what, const int* table, int n_features, int B, int C, int Co, int T, long n_weights,
                    bool have_weights, FdTable& tab, int& n_cat, int& max_width) {
    BM_REQUIRE(table && n_features >= 1 && n_features <= FD_MAX_FEATURES, "%s: 1 .. %d features, got %d", what,
               FD_MAX_FEATURES, n_features);
    BM_REQUIRE(B > 0 && C > 0 && Co > 0 && T > 0 && (long)B * C * T < (1L << 31) && (long)B * Co * T < (1L << 31),
               "%s: bad shape (B C T must stay below 2^31)", what);
    tab.n = n_features;
    n_cat = 0;
    max_width = 1;
    int e = 0, o = 0;
    for (int f = 0; f < n_features; ++f) {
        FdFeature& ft = tab.f[f];
        ft.kind = table[5 * f], ft.est_start = table[5 * f + 1], ft.width = table[5 * f + 2];
        ft.out_start = table[5 * f + 3], ft.weight_off = table[5 * f + 4];
        BM_REQUIRE(ft.kind == FD_CONTINUOUS || ft.kind == FD_CATEGORICAL, "%s: feature %d: kind %d", what, f, ft.kind);
        BM_REQUIRE(ft.width >= 1 && ft.est_start == e && ft.out_start == o,
                   "%s: feature %d does not follow its predecessor (est %d, expected %d; out %d, expected %d; width %d)",
                   what, f, ft.est_start, e, ft.out_start, o, ft.width);
        e += ft.width;
        if (ft.kind == FD_CATEGORICAL) {
            BM_REQUIRE(ft.width <= FD_MAX_K, "%s: feature %d: %d classes exceed %d", what, f, ft.width, FD_MAX_K);
            BM_REQUIRE(ft.weight_off == -1 || (have_weights && ft.weight_off >= 0 &&
                                               (long)ft.weight_off + ft.width <= n_weights),
                       "%s: feature %d: weight offset %d outside the %ld weights", what, f, ft.weight_off, n_weights);
            o += 1;
            ++n_cat;
        } else {
            ft.weight_off = -1;
            o += ft.width;
        }
        max_width = ft.width > max_width ? ft.width : max_width;
    }
    BM_REQUIRE(e == C && o == Co, "%s: the features span %d / %d channels, est has %d and out %d", what, e, o, C, Co);
    return BM_OK;
}

extern "C" int bm_feature_decoding_fwd(const float* est, const float* out, const unsigned char* mask,
                                       const float* weights, long n_weights, const int* table, int n_features, int B,
                                       int C, int Co, int T, float* loss, float* terms, double* denoms, float* lse,
                                       void* workspace, long workspace_bytes, int* flag, void* stream) {
    FdTable tab;
    int n_cat, max_width;
    const int rc = fd_table("feature_decoding_fwd", table, n_features, B, C, Co, T, n_weights, weights != nullptr, tab,
                            n_cat, max_width);
    if (rc != BM_OK) return rc;
    BM_REQUIRE(est && out && loss && terms && denoms && (lse || n_cat == 0), "feature_decoding_fwd: null pointer");
    if (!workspace || workspace_bytes < RG_WS_BYTES)
        return bm_set_error(BM_ERR_WORKSPACE, "feature_decoding_fwd: workspace");
    const unsigned npos = (unsigned)((long)B * T);
    const unsigned ntiles = (unsigned)cdiv(npos, FD_TILE);
    const unsigned blocks = ntiles < FD_MAX_BLOCKS ? ntiles : FD_MAX_BLOCKS;
    hipLaunchKernelGGL(feature_decoding_fwd_kernel, dim3(blocks), dim3(RG_THREADS), 0, (hipStream_t)stream, est, out,
                       mask, weights, tab, npos, ntiles, C, Co, (unsigned)T, bm_fastdiv((unsigned)T), rg_ws(workspace),
                       loss, terms, denoms, lse, flag);
    return bm_check_launch("feature_decoding_fwd");
}

extern "C" int bm_feature_decoding_bwd(const float* est, const float* out, const unsigned char* mask,
                                       const float* weights, long n_weights, const int* table, int n_features, int B,
                                       int C, int Co, int T, const float* grad_out, const double* denoms,
                                       const float* lse, float* d_est, void* stream) {
    FdTable tab;
    int n_cat, max_width;
    const int rc = fd_table("feature_decoding_bwd", table, n_features, B, C, Co, T, n_weights, weights != nullptr, tab,
                            n_cat, max_width);
    if (rc != BM_OK) return rc;
    BM_REQUIRE(est && out && grad_out && denoms && d_est && (lse || n_cat == 0), "feature_decoding_bwd: null pointer");
    const unsigned npos = (unsigned)((long)B * T);
    const unsigned ntiles = (unsigned)cdiv(npos, FD_TILE);
    const unsigned gx = ntiles < FD_BWD_MAX_TILES ? ntiles : FD_BWD_MAX_TILES;
    // ~2 048 workgroups: short batches split the channels of the widest feature over blockIdx.y
    int gy = cdiv(2048, gx);
    const int most = cdiv(max_width, 4);
    gy = gy > most ? most : gy;
    gy = gy > 64 ? 64 : gy;
    hipLaunchKernelGGL(feature_decoding_bwd_kernel, dim3(gx, gy), dim3(RG_THREADS), 0, (hipStream_t)stream, est, out,
                       mask, weights, tab, npos, ntiles, C, Co, (unsigned)T, bm_fastdiv((unsigned)T), grad_out, denoms,
                       lse, d_est);
    return bm_check_launch("feature_decoding_bwd");
}

// ---- ClassificationAcc (bm/metrics.py:173-180): one thread per (b, t) of the window [t0, T) ---------------------------
// pred = the first index of the maximum over the K rows (a NaN counts as the maximum: torch.argmax); a selected position
// adds 1 to count[t] and, when (float)pred == target, 1 to hits[t].  Integer atomics: the sums do not depend on the
// order, two runs are equal.
__global__ __launch_bounds__(RG_THREADS) void class_acc_kernel(const float* __restrict__ est, long est_bstride,
                                                               const float* __restrict__ tgt, long tgt_bstride,
                                                               const unsigned char* __restrict__ mask,
                                                               long mask_bstride, int B, int K, int T, int t0,
                                                               unsigned long long* __restrict__ acc) {
    const int Tw = T - t0;
    const long i = (long)blockIdx.x * RG_THREADS + threadIdx.x;
    if (i >= (long)B * Tw) return;
    const int b = (int)(i / Tw), col = (int)(i - (long)b * Tw), t = t0 + col;
    if (mask && !mask[b * mask_bstride + t]) return;
    const float* x = est + b * est_bstride + t;
    float best = x[0];
    int pred = 0;
    for (int k0 = 1; k0 < K; k0 += FD_UNROLL) {
        float xv[FD_UNROLL];
#pragma unroll
        for (int i2 = 0; i2 < FD_UNROLL; ++i2) xv[i2] = x[(long)(k0 + i2 < K ? k0 + i2 : k0) * T];
#pragma unroll
        for (int i2 = 0; i2 < FD_UNROLL; ++i2) {
            const bool take = k0 + i2 < K && best == best && (xv[i2] > best || xv[i2] != xv[i2]);
            best = take ? xv[i2] : best;
            pred = take ? k0 + i2 : pred;
        }
    }
    atomicAdd(acc + Tw + col, 1ull);
    if ((float)pred == tgt[b * tgt_bstride + t]) atomicAdd(acc + col, 1ull);
}

extern "C" int bm_class_acc_update(const float* est, long est_bstride, const float* target, long target_bstride,
                                   const unsigned char* mask, long mask_bstride, int B, int K, int T, int t0, long* acc,
                                   void* stream) {
    BM_REQUIRE(B >= 0 && K > 0 && T > 0 && t0 >= 0 && t0 < T && acc, "class_acc_update: bad arguments");
    BM_REQUIRE(B == 0 || (est && target), "class_acc_update: null pointer");
    BM_REQUIRE((long)B * (T - t0) < (1L << 31) * RG_THREADS, "class_acc_update: too many positions");
    if (B == 0) return BM_OK;
    hipLaunchKernelGGL(class_acc_kernel, dim3(cdiv((long)B * (T - t0), RG_THREADS)), dim3(RG_THREADS), 0,
                       (hipStream_t)stream, est, est_bstride, target, target_bstride, mask, mask_bstride, B, K, T, t0,
                       (unsigned long long*)acc);
    return bm_check_launch("class_acc_update");
}
