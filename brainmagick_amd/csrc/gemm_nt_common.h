// What the narrow "NT" time-contraction kernels (gemm_nt.hip: exact fp32, gemm_nt_x3.hip: 3 x bf16) share: the
// argument block, the walk of a workgroup over its share of the (segment, 32-sample chunk) list, the partial-tile
// epilogue, and on the host the argument check, the launch tail and the tile table.  A family keeps its staging and
// its MFMA loop.  The wide f16x2 kernel (gemm_nt_h2w.hip) has its own, hand-scheduled, prologue and only takes the
// declarations of the C-ABI from here: every definition of these units is compiled against the header that the
// ctypes binding parses (after bm_common.h, whose BM_ACT_* enumerators the header restates as macros).
#pragma once
#include "mfma_split.h"
#include "../../include/bm_hip.h"

#define BKT 32                                         // samples of one chunk of the reduction

struct GemmNTArgs {
    const float* a; long a_sstride; long a_rstride;   // A[s][m][t]
    const float* x; long x_sstride; long x_rstride;   // X[s][c][t]
    const int* order;                                  // segment list (grouped) or null = identity
    const int* seg;                                    // [G+1] group boundaries or null = one group [0, S)
    float* part;                                       // [G*nsplit][M][Cn*KS]
    int S, M, Cn, T, dil, nsplit, G;
    int tiles_m, tiles_c;
};

// What a workgroup works on: tile (tm, tc) = rows from m0, columns from c0, of split `split` of group g; the group's
// segments [s_begin, s_end) of `order`, cps chunks per segment, and the split's share [q_begin, q_end) of the group's
// flat (segment, chunk) list.
struct GemmNTWork {
    int tm, tc, split, g, m0, c0, s_begin, s_end, cps;
    long q_begin, q_end;
};

// block -> (tile_m, tile_c, split, g).  XCD-aware: all tiles of one (g, split) -- which stream the SAME segments --
// get consecutive logical ids, i.e. run on one XCD and share its L2.
template <int BM, int BC>
__device__ __forceinline__ GemmNTWork gemm_nt_work(const GemmNTArgs& a) {
    GemmNTWork w;
    int id = bm_xcd_remap(blockIdx.x, gridDim.x);
    w.tm = id % a.tiles_m; id /= a.tiles_m;
    w.tc = id % a.tiles_c; id /= a.tiles_c;
    w.split = id % a.nsplit;
    w.g = id / a.nsplit;
    w.m0 = w.tm * BM; w.c0 = w.tc * BC;
    w.s_begin = a.seg ? a.seg[w.g] : 0;
    w.s_end = a.seg ? a.seg[w.g + 1] : a.S;
    w.cps = (a.T + BKT - 1) / BKT;                     // chunks per segment
    const long nchunks = (long)(w.s_end - w.s_begin) * w.cps;
    w.q_begin = nchunks * w.split / a.nsplit;
    w.q_end = nchunks * (w.split + 1) / a.nsplit;
    return w;
}

template <int MT, int NT, int KS>
__device__ __forceinline__ void gemm_nt_zero(f32x16 (&acc)[MT][NT][KS]) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int j = 0; j < KS; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][k][j][r] = 0.f;
}

// epilogue: part[(g*nsplit+split)][m][c*KS + j]; wavefront (wm, wc) of WM x WC owns MT x NT 32x32 blocks per tap
// (C/D layout: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5))
template <int WM, int WC, int MT, int NT, int KS>
__device__ __forceinline__ void gemm_nt_store_partial(const GemmNTArgs& a, const GemmNTWork& w,
                                                      const f32x16 (&acc)[MT][NT][KS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WC, wc = wave % WC;
    const int nl = lane & 31, h = lane >> 5;
    const long N = (long)a.Cn * KS;
    float* dst = a.part + (long)(w.g * a.nsplit + w.split) * a.M * N;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const int c = w.c0 + wc * NT * 32 + k * 32 + nl;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = w.m0 + wm * MT * 32 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < a.M && c < a.Cn) {
#pragma unroll
                    for (int j = 0; j < KS; ++j) dst[(long)m * N + (long)c * KS + j] = acc[i][k][j][r];
                }
            }
        }
}

// host: the bm_gemm_nt contract, checked and filled into `g` (`family` names the entry point in the messages)
static inline int gemm_nt_fill_args(GemmNTArgs& g, const char* family, const float* a, long a_sstride, long a_rstride,
                                    const float* x, long x_sstride, long x_rstride, const int* order, const int* seg,
                                    float* part, int S, int G, int M, int Cn, int T, int dil, int nsplit) {
    BM_REQUIRE(a && x && part, "%s: null pointer", family);
    BM_REQUIRE(M > 0 && Cn > 0 && T > 0 && G > 0 && nsplit > 0 && S >= 0, "%s: bad dims", family);
    BM_REQUIRE(G == 1 || seg, "%s: grouped call needs seg[]", family);
    g.a = a; g.a_sstride = a_sstride; g.a_rstride = a_rstride;
    g.x = x; g.x_sstride = x_sstride; g.x_rstride = x_rstride;
    g.order = order; g.seg = seg; g.part = part;
    g.S = S; g.M = M; g.Cn = Cn; g.T = T; g.dil = dil; g.nsplit = nsplit; g.G = G;
    return BM_OK;
}

// host: launch of `kernel` with WM x WC wavefronts on BM x BC tiles and `lds` bytes of dynamic LDS
static inline int gemm_nt_launch(void (*kernel)(GemmNTArgs), GemmNTArgs a, int BM, int BC, int nthreads, size_t lds,
                                 const char* label, hipStream_t stream) {
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return bm_set_error((int)e, "%s: hipFuncSetAttribute: %s", label, hipGetErrorString(e));
    }
    a.tiles_m = cdiv(a.M, BM);
    a.tiles_c = cdiv(a.Cn, BC);
    const long nblocks = (long)a.tiles_m * a.tiles_c * a.nsplit * a.G;
    if (nblocks <= 0) return BM_OK;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblocks), dim3(nthreads), lds, stream, a);
    return bm_check_launch(label);
}

// host: the tile table -- 2 x 2 wavefronts of MT x NT blocks, 128 or 64 rows / columns by least padding; the taps
// multiply the accumulators, so 3 taps keep 64 columns and 5 taps 64 x 64.  Family::launch<WM, WC, MT, NT, KS> is
// the family's launcher, Family::name its entry point.
template <class Family>
static int gemm_nt_launch_tile(const GemmNTArgs& g, int KS, hipStream_t s) {
    const bool bigM = prefer_big(g.M);
    if (KS == 1) {
        const bool bigC = prefer_big(g.Cn);
        if (bigM && bigC) return Family::template launch<2, 2, 2, 2, 1>(g, s);
        if (bigM) return Family::template launch<2, 2, 2, 1, 1>(g, s);
        if (bigC) return Family::template launch<2, 2, 1, 2, 1>(g, s);
        return Family::template launch<2, 2, 1, 1, 1>(g, s);
    }
    if (KS == 3) {
        if (bigM) return Family::template launch<2, 2, 2, 1, 3>(g, s);
        return Family::template launch<2, 2, 1, 1, 3>(g, s);
    }
    if (KS == 5) return Family::template launch<2, 2, 1, 1, 5>(g, s);
    return bm_set_error(BM_ERR_UNSUPPORTED, "%s: kernel size %d not supported (1, 3, 5)", Family::name, KS);
}
