// The encode task's model input (bm/solver.py:288-292): x[b][c][t] = meg[b][c][t] for t < limit, 0 for every other t --
// the reference's `mask * meg` with mask[:limit] = 1, in ONE launch that reads only the head (limit / T of the tensor),
// writes every element of x exactly once (x needs no fill) and publishes max |x| into the tensor's amax slot.
//
// Two deliberate differences to `mask * meg`, both in the tail t >= limit, which is never read:
//   * a tail element is +0.0 even where the reference's product 0 * meg would be -0.0 (meg negative);
//   * a non-finite value in the tail gives 0, not NaN (0 * inf).  The Solver's finiteness check has covered the whole
//     of meg before this kernel runs; what it rejects never reaches the model.
// The head is copied bit for bit (-0.0, NaN included).  max |x| is taken with fmaxf: a NaN in the head does not reach it.
//
// One flat grid-stride walk over the vectors of V elements (V = 4 when T % 4 == 0 and both pointers are 16-byte
// aligned, so a vector never straddles two rows; the `limit` boundary inside a vector is resolved by select), rows
// (b, c) in memory order: consecutive lanes store consecutive vectors whatever T is.  A workgroup takes chunks of
// MI_THREADS * MI_UNROLL consecutive vectors; a thread has MI_UNROLL loads, then MI_UNROLL stores in flight.  No
// workgroup waits for another: the per-workgroup maxima are folded by the workgroup that finishes last
// (bm_block.h).  That ticket is one agent-scope atomic per workgroup on one address, about 12 ns each on the
// MI355X -- with 2 048 workgroups of 256 threads it cost more than the stores (40 us against 17 us without the maximum
// at 256 x 273 x 360); hence few, large workgroups: at most one per CU, 512 threads (19 us).
#include "bm_block.h"

#define MI_THREADS 512
#define MI_WAVES (MI_THREADS / 64)
#define MI_MAX_BLOCKS 256
#define MI_UNROLL 4

// Workspace (bm_meg_init_workspace_bytes): the ticket counter, then the per-workgroup partial maxima.
static const long MI_WS_BYTES = BmFoldWs<float>::bytes(MI_MAX_BLOCKS);

extern "C" long bm_meg_init_workspace_bytes(void) { return MI_WS_BYTES; }

template <int V>
__global__ __launch_bounds__(MI_THREADS) void meg_init_kernel(const float* __restrict__ meg, float* __restrict__ x,
                                                              unsigned nvec, unsigned Tv, BmFastDiv div_tv, int limit,
                                                              float* __restrict__ amax_out, unsigned* ticket,
                                                              float* part) {
    typedef typename BmVec<V>::F FV;
    __shared__ BmFoldLds<float, MI_WAVES> sh;
    const unsigned chunk = MI_THREADS * MI_UNROLL;
    float mx = 0.f;
    for (unsigned base = blockIdx.x * chunk; base < nvec; base += gridDim.x * chunk) {
        FV r[MI_UNROLL];
#pragma unroll
        for (int u = 0; u < MI_UNROLL; ++u) {
            const unsigned j = base + u * MI_THREADS + threadIdx.x;
            const unsigned jc = j < nvec ? j : nvec - 1;    // past the end: re-reads the last vector, stores nothing
            const unsigned row = bm_div(jc, div_tv);
            const int t = (int)(jc - row * Tv) * V;         // first sample of the vector
            FV v;
#pragma unroll
            for (int i = 0; i < V; ++i) bm_set(v, i, 0.f);
            if (t < limit) v = ((const FV*)meg)[jc];
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float e = t + i < limit ? bm_get(v, i) : 0.f;
                bm_set(r[u], i, e);
                mx = fmaxf(mx, fabsf(e));
            }
        }
#pragma unroll
        for (int u = 0; u < MI_UNROLL; ++u) {
            const unsigned j = base + u * MI_THREADS + threadIdx.x;
            if (j < nvec) ((FV*)x)[j] = r[u];
        }
    }
    if (!amax_out) return;                              // kernel argument: uniform
    if (!bm_amax_arrive(mx, part + blockIdx.x, ticket, gridDim.x, sh)) return;
    bm_amax_fold<MI_WAVES>(part, gridDim.x, amax_out, sh.wave[0]);
}

extern "C" int bm_meg_init(const float* meg, float* x, int B, int C, int T, int limit, float* amax_out,
                           void* workspace, long workspace_bytes, void* stream) {
    BM_REQUIRE(B >= 0 && C > 0 && T > 0 && (long)B * C * T < (1L << 31), "meg_init: bad shape");
    BM_REQUIRE(B == 0 || (meg && x), "meg_init: null pointer");
    if (amax_out && (!workspace || workspace_bytes < MI_WS_BYTES))
        return bm_set_error(BM_ERR_WORKSPACE, "meg_init: workspace");
    if (B == 0) return BM_OK;
    limit = limit < 0 ? 0 : limit > T ? T : limit;      // the reference's mask[:limit] = 1 saturates
    const bool vec = T % 4 == 0 && (((uintptr_t)meg | (uintptr_t)x) & 15) == 0;
    const int V = vec ? 4 : 1;
    const unsigned nvec = (unsigned)((long)B * C * T / V), Tv = (unsigned)(T / V);
    int blocks = cdiv(nvec, MI_THREADS * MI_UNROLL);
    blocks = blocks < 1 ? 1 : blocks > MI_MAX_BLOCKS ? MI_MAX_BLOCKS : blocks;
    const BmFoldWs<float> ws = BmFoldWs<float>::at(amax_out ? workspace : nullptr);
    hipStream_t s = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(meg_init_kernel<4>, dim3(blocks), dim3(MI_THREADS), 0, s, meg, x, nvec, Tv, bm_fastdiv(Tv),
                           limit, amax_out, ws.tickets, ws.part);
    else
        hipLaunchKernelGGL(meg_init_kernel<1>, dim3(blocks), dim3(MI_THREADS), 0, s, meg, x, nvec, Tv, bm_fastdiv(Tv),
                           limit, amax_out, ws.tickets, ws.part);
    return bm_check_launch("meg_init");
}
