// task.lowpass (bm/solver.py:278-281): julius.lowpass_filter(meg, cutoff, zeros) with stride 1 and pad=True -- a windowed
// sinc FIR of 2 * half + 1 taps over the replicate-padded last dimension, same length out:
//     y[r][t] = sum_k taps[k] * x[r][clamp(t + k - half, 0, T - 1)]        for t < keep,        +0.0 for t >= keep.
// ONE launch that reads x in place through a row stride (the `offset_meg_ms` view of the batch: no contiguous copy),
// writes every element of y exactly once and publishes max |y| into the tensor's amax slot.  With keep < T it is the
// encode task's `mask * lowpass(meg)` (bm/solver.py:288-292) and then reads only x[r][0 : min(T, keep + half)]; the tail
// is +0.0 whatever x holds there, as in encode.hip.
//
// The sum is ALWAYS the direct one (julius switches to an FFT convolution above 32 half-taps: the same mathematics,
// other last bits) in ONE order: fp32 fmaf, k ascending, from 0.f.  The scalar and the 16-byte instantiation, every
// grid, every `keep` and every compute mode therefore give the same bits.
//
// A workgroup stages R whole padded rows (row pitch Wp = T + 2 half rounded up to 4 floats, R Wp <= LP_LDS) and the taps
// in LDS, then every thread produces V adjacent outputs (V = 4 when T % 4 == 0 and y is 16-byte aligned): it slides a
// window of 2 V samples through registers, one V-wide LDS read of samples and one of taps (the same address in every
// lane: a broadcast) per V taps, both issued one block ahead of the V * V fmaf that consume them.  Consecutive lanes read
// consecutive V-float slots.  The edges are replicated while staging: the body is loaded from x (16-byte loads when x
// and row_stride allow it), the pads are copied from the staged first / last sample; no load index leaves
// [row start, row start + T).  The loads of a workgroup's NEXT rows are issued into registers before the current rows are
// filtered and land in LDS after them: a workgroup has one CU to itself (64 KB of LDS, at most 256 of them: few, large
// workgroups and the last-arriver fold of the maxima, bm_block.h, as in encode.hip): nothing else hides their latency.
//
// Measured at 256 x 273 x 360 through the [..., 18:] view, 21 taps (profiles/lowpass_vs_torch.txt; kernel times by
// rocprofv3): 131 us with 512 threads and no look-ahead, 88-92 us as it is (74 us where x allows 16-byte loads), 1.6 us
// more per tap -- about 40 % of the fp32 FMA rate inside the tap loop.  A stated baseline: loading, staging and
// filtering are phases of ONE workgroup per CU, separated by barriers, so memory and LDS take turns.  Tried and dropped
// because the time did not move: storing a round's results one round later (the wait for the loads also waits for the
// stores in front of it), and staging 12 288 floats at a time.  Two workgroups per CU, or waves that only load, are next.
#include "bm_block.h"

#define LP_THREADS 1024
#define LP_WAVES (LP_THREADS / 64)
#define LP_MAX_BLOCKS 256
#define LP_LDS 8192                 // floats of staged rows: the largest padded row, T + 2 half
#define LP_SLACK 16                 // floats the look-ahead reads may run past the staged rows / the taps (never used)

// Workspace (bm_lowpass_workspace_bytes): the ticket counter, then the per-workgroup partial maxima.
static const long LP_WS_BYTES = BmFoldWs<float>::bytes(LP_MAX_BLOCKS);

extern "C" long bm_lowpass_workspace_bytes(void) { return LP_WS_BYTES; }

struct LpPlan {
    int R;                  // rows a workgroup stages at a time
    int Wp;                 // LDS row pitch, a multiple of 4
    int n_body;             // samples of a row that are loaded: min(T, keep + half), 0 when keep == 0
    int nq;                 // loads per row: n_body scalars or ceil(n_body / 4) vectors
    BmFastDiv div_nq, div_pad, div_tg;
};

// The loads of the rows [row0, row0 + nr) into registers: item i = (row, q) is the VL samples from q VL on.  A vector
// that would cross the end of the row is loaded sample by sample.
template <int VL>
__device__ __forceinline__ void lp_load(typename BmVec<VL>::F* pre, const float* __restrict__ x, long row_stride, int row0,
                                        int nr, int T, const LpPlan& plan) {
    typedef typename BmVec<VL>::F FL;
#pragma unroll
    for (int u = 0; u < LP_LDS / VL / LP_THREADS; ++u) {
        const unsigned i = u * LP_THREADS + threadIdx.x;
        if (i < (unsigned)(nr * plan.nq)) {
            const unsigned r = bm_div(i, plan.div_nq);
            const int s = (int)(i - r * plan.nq) * VL;
            const float* src = x + (long)(row0 + r) * row_stride + s;
            if (s + VL <= T) {
                pre[u] = *(const FL*)src;
            } else {
#pragma unroll
                for (int e = 0; e < VL; ++e) bm_set(pre[u], e, s + e < T ? src[e] : 0.f);
            }
        }
    }
}

// ... and from the registers to LDS column half + s of their row.
template <int VL>
__device__ __forceinline__ void lp_stage(const typename BmVec<VL>::F* pre, float* smp, int nr, int T, int half,
                                         const LpPlan& plan) {
#pragma unroll
    for (int u = 0; u < LP_LDS / VL / LP_THREADS; ++u) {
        const unsigned i = u * LP_THREADS + threadIdx.x;
        if (i < (unsigned)(nr * plan.nq)) {
            const unsigned r = bm_div(i, plan.div_nq);
            const int s = (int)(i - r * plan.nq) * VL;
            float* dst = smp + r * plan.Wp + half + s;
#pragma unroll
            for (int e = 0; e < VL; ++e)
                if (s + e < T) dst[e] = bm_get(pre[u], e);
        }
    }
}

template <int V, int VL>
__global__ __launch_bounds__(LP_THREADS) void lowpass_kernel(const float* __restrict__ x, long row_stride,
                                                             float* __restrict__ y, int rows, int T, int keep,
                                                             const float* __restrict__ taps, int half, LpPlan plan,
                                                             float* __restrict__ amax_out, unsigned* ticket,
                                                             float* part) {
    typedef typename BmVec<V>::F FV;
    typedef typename BmVec<VL>::F FL;
    __shared__ __attribute__((aligned(16))) float smp[LP_LDS + LP_SLACK];
    __shared__ __attribute__((aligned(16))) float tp[LP_LDS + LP_SLACK];
    __shared__ BmFoldLds<float, LP_WAVES> sh;
    const int ntaps = 2 * half + 1, Wp = plan.Wp, npad = 2 * half;
    const unsigned Tg = (unsigned)(T / V);
    for (int k = threadIdx.x; k < ntaps + 2 * V; k += LP_THREADS) tp[k] = k < ntaps ? taps[k] : 0.f;
    float mx = 0.f;
    FL pre[LP_LDS / VL / LP_THREADS];               // the next rows, in flight while the current ones are filtered
    int row0 = blockIdx.x * plan.R;
    lp_load<VL>(pre, x, row_stride, row0, min(plan.R, rows - row0), T, plan);
    while (row0 < rows) {
        const int nr = min(plan.R, rows - row0);
        lp_stage<VL>(pre, smp, nr, T, half, plan);
        __syncthreads();
        // replicate padding: `half` copies of the first sample in front, of the last one behind (those only when the
        // whole row was loaded: with keep + half <= T no output that is kept reaches them)
        for (unsigned i = threadIdx.x; i < (unsigned)(nr * npad); i += LP_THREADS) {
            const unsigned r = bm_div(i, plan.div_pad);
            const int j = (int)(i - r * npad);
            float* row = smp + r * Wp;
            if (j < half) {
                if (plan.n_body > 0) row[j] = row[half];
            } else if (plan.n_body == T) {
                row[T + j] = row[half + T - 1];
            }
        }
        __syncthreads();
        const int next = row0 + gridDim.x * plan.R;
        if (next < rows) lp_load<VL>(pre, x, row_stride, next, min(plan.R, rows - next), T, plan);
        for (unsigned g = threadIdx.x; g < (unsigned)nr * Tg; g += LP_THREADS) {
            const unsigned r = bm_div(g, plan.div_tg);
            const int t0 = (int)(g - r * Tg) * V;
            FV out;
#pragma unroll
            for (int i = 0; i < V; ++i) bm_set(out, i, 0.f);
            if (t0 < keep) {
                const float* a = smp + r * Wp + t0;
                FV c0 = *(const FV*)a, c1 = *(const FV*)(a + V), tk = *(const FV*)tp;
                float acc[V];
#pragma unroll
                for (int i = 0; i < V; ++i) acc[i] = 0.f;
                for (int kb = 0; kb < ntaps; kb += V) {
                    const FV nx = *(const FV*)(a + kb + 2 * V), tn = *(const FV*)(tp + kb + V);
                    float w[2 * V];
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        w[i] = bm_get(c0, i);
                        w[V + i] = bm_get(c1, i);
                    }
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        if (kb + j < ntaps) {                       // uniform
                            const float c = bm_get(tk, j);
#pragma unroll
                            for (int i = 0; i < V; ++i) acc[i] = fmaf(c, w[i + j], acc[i]);
                        }
                    }
                    c0 = c1;
                    c1 = nx;
                    tk = tn;
                }
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const float e = t0 + i < keep ? acc[i] : 0.f;
                    bm_set(out, i, e);
                    mx = fmaxf(mx, fabsf(e));
                }
            }
            ((FV*)y)[(unsigned)row0 * Tg + g] = out;
        }
        __syncthreads();                                    // the next rows overwrite what was just read
        row0 = next;
    }
    if (!amax_out) return;                              // kernel argument: uniform
    if (!bm_amax_arrive(mx, part + blockIdx.x, ticket, gridDim.x, sh)) return;
    bm_amax_fold<LP_WAVES>(part, gridDim.x, amax_out, sh.wave[0]);
}

extern "C" int bm_lowpass(const float* x, long row_stride, float* y, int rows, int T, int keep, const float* taps,
                          int half, float* amax_out, void* workspace, long workspace_bytes, void* stream) {
    BM_REQUIRE(rows >= 0 && T > 0 && half >= 0 && (long)rows * T < (1L << 31), "lowpass: bad shape");
    BM_REQUIRE(row_stride >= T, "lowpass: row_stride %ld is below T = %d", row_stride, T);
    BM_REQUIRE(rows == 0 || (x && y && taps), "lowpass: null pointer");
    if ((long)T + 2L * half > LP_LDS)
        return bm_set_error(BM_ERR_UNSUPPORTED, "lowpass: T + 2 * half = %ld exceeds the limit of %d samples per padded "
                            "row (T = %d, half = %d)", (long)T + 2L * half, LP_LDS, T, half);
    if (amax_out && (!workspace || workspace_bytes < LP_WS_BYTES))
        return bm_set_error(BM_ERR_WORKSPACE, "lowpass: workspace");
    if (rows == 0) return BM_OK;
    keep = keep < 0 ? 0 : keep > T ? T : keep;
    LpPlan plan;
    plan.Wp = (T + 2 * half + 3) & ~3;
    const int rmax = LP_LDS / plan.Wp;                   // >= 1: LP_LDS is a multiple of 4
    plan.R = cdiv(rows, LP_MAX_BLOCKS);
    plan.R = plan.R < 1 ? 1 : plan.R > rmax ? rmax : plan.R;
    const int blocks = cdiv(rows, plan.R) < LP_MAX_BLOCKS ? cdiv(rows, plan.R) : LP_MAX_BLOCKS;
    const long reach = (long)keep + half;
    plan.n_body = keep == 0 ? 0 : reach < T ? (int)reach : T;
    const bool vload = ((uintptr_t)x & 15) == 0 && row_stride % 4 == 0;
    plan.nq = vload ? cdiv(plan.n_body, 4) : plan.n_body;
    const bool vec = T % 4 == 0 && ((uintptr_t)y & 15) == 0;
    plan.div_nq = bm_fastdiv(plan.nq > 0 ? plan.nq : 1);
    plan.div_pad = bm_fastdiv(half > 0 ? 2 * half : 1);
    plan.div_tg = bm_fastdiv(vec ? T / 4 : T);
    const BmFoldWs<float> ws = BmFoldWs<float>::at(amax_out ? workspace : nullptr);
    hipStream_t s = (hipStream_t)stream;
#define LP_LAUNCH(V, VL)                                                                                        \
    hipLaunchKernelGGL((lowpass_kernel<V, VL>), dim3(blocks), dim3(LP_THREADS), 0, s, x, row_stride, y, rows, T, keep, \
                       taps, half, plan, amax_out, ws.tickets, ws.part)
    if (vec && vload)
        LP_LAUNCH(4, 4);
    else if (vec)
        LP_LAUNCH(4, 1);
    else if (vload)
        LP_LAUNCH(1, 4);
    else
        LP_LAUNCH(1, 1);
#undef LP_LAUNCH
    return bm_check_launch("lowpass");
}
