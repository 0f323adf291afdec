// What the kernels that reduce over a workgroup, or over a grid in ONE launch, share: the scalar / 16-byte vector
// instantiation of an element walk, the block maximum, sum and OR, the ticket by which the workgroup that finishes last
// folds the others' partials, the workspace and LDS that go with it, and the fold of partial maxima into an amax slot.
#pragma once
#include "bm_common.h"

template <int V> struct BmVec;
template <> struct BmVec<1> {
    typedef float F;
    typedef unsigned char M;
};
template <> struct BmVec<4> {
    typedef f32x4 F;
    typedef uchar4 M;
};
__device__ __forceinline__ float bm_get(const float& v, int) { return v; }
__device__ __forceinline__ float bm_get(const f32x4& v, int i) { return v[i]; }
__device__ __forceinline__ unsigned char bm_get(const unsigned char& v, int) { return v; }
__device__ __forceinline__ unsigned char bm_get(const uchar4& v, int i) {
    return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}
__device__ __forceinline__ void bm_set(float& v, int, float x) { v = x; }
__device__ __forceinline__ void bm_set(f32x4& v, int i, float x) { v[i] = x; }

// ---- block reductions: WAVES = blockDim.x / 64, sh = WAVES values of LDS, the result in every thread ------------------
// ONE order, pairwise: (s0 + s1) + (s2 + s3) for four wavefronts.  The sums of the callers are bit-reproducible because
// of it; a maximum (fmaxf over values >= 0, or with -inf as "nothing") does not depend on the order at all.
template <int N, typename T, typename Op>
__device__ __forceinline__ T bm_pairwise(const T* v, Op op) {
    if constexpr (N == 1) return v[0];
    else return op(bm_pairwise<N / 2>(v, op), bm_pairwise<N - N / 2>(v + N / 2, op));
}
// `wv`: a wavefront's value.  Two barriers: `sh` is free again on return.
template <int WAVES, typename T, typename Op>
__device__ __forceinline__ T bm_block_fold(T wv, T* sh, Op op) {
    bm_wave_to_lds(wv, sh);
    __syncthreads();
    wv = bm_pairwise<WAVES>(sh, op);
    __syncthreads();
    return wv;
}
__device__ __forceinline__ float bm_max2(float a, float b) { return fmaxf(a, b); }
template <int WAVES>
__device__ __forceinline__ float bm_block_max(float v, float* sh) {
    return bm_block_fold<WAVES>(bm_wave_max(v), sh, bm_max2);
}
template <int WAVES>
__device__ __forceinline__ float bm_block_sum(float v, float* sh) {
    return bm_block_fold<WAVES>(bm_wave_sum(v), sh, [](float a, float b) { return a + b; });
}
template <int WAVES>
__device__ __forceinline__ double bm_block_sum(double v, double* sh) {
    return bm_block_fold<WAVES>(bm_wave_sum_d(v), sh, [](double a, double b) { return a + b; });
}
// The OR of the wavefronts' flag bits in THREAD 0 only (another thread keeps `wv`): what a kernel does before thread 0
// adds the workgroup's bits to a flag word in memory.  `wv`: bm_wave_or of the lanes' bits, or bits that are uniform over
// the wavefront.  ONE barrier, in front of thread 0's reads of `sh`; an OR does not depend on the order.
// (__lane_id() == 0 compiles to the test of bm_wave_to_lds, threadIdx.x & 63; spelled with threadIdx.x the compiler
// also learns the low bits of threadIdx.x inside the branch, forms sh's address a second way, and word_hash_pick_kernel
// holds both forms in registers across its loop: 2 VGPRs.)
template <int WAVES>
__device__ __forceinline__ int bm_block_or(int wv, int* sh) {
    if (__lane_id() == 0) sh[threadIdx.x >> 6] = wv;
    __syncthreads();
    if (threadIdx.x == 0) wv = bm_pairwise<WAVES>(sh, [](int a, int b) { return a | b; });
    return wv;
}

// ---- the last-arriver fold ----------------------------------------------------------------------------------------------
// Workspace: 64 bytes of ticket counters (ZERO between launches: the last workgroup of a launch resets its counter),
// then the per-workgroup partials.
template <typename P>
struct BmFoldWs {
    unsigned* tickets;
    P* part;
    static constexpr long bytes(long n_partials) { return 64 + n_partials * (long)sizeof(P); }
    static BmFoldWs at(void* base) {                    // null (nothing to fold): both pointers null
        return base ? BmFoldWs{(unsigned*)base, (P*)((char*)base + 64)} : BmFoldWs{nullptr, nullptr};
    }
};
// LDS: N sets of wavefront values (a kernel that reduces N values at a time) and the last-arriver flag.
template <typename T, int WAVES, int N = 1>
struct BmFoldLds {
    T wave[N][WAVES];
    int last;
};

// Thread 0 stores its workgroup's partial write-through (sc1: no agent-scope release needed -- a release would write
// back the whole XCD L2, which the backward has just filled with dEst), waits for the store, draws a ticket; returns
// true in every thread of the workgroup that finished last, after the acquire that makes the other workgroups'
// partials visible to it.
template <typename P>
__device__ __forceinline__ void bm_store_partial(P* dst, P v) {
    __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool bm_last_arriver(unsigned* ticket, unsigned nblocks, int* sh_flag) {
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = prev == nblocks - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        }
        *sh_flag = last;
    }
    __syncthreads();
    return *sh_flag != 0;
}

// A producer's max |output| (`mx`: the thread's, >= 0) in the same launch: the workgroup's maximum goes to *part_dst;
// true in the workgroup that finished last, which then calls bm_amax_fold or bm_amax_fold_rows.
template <int WAVES>
__device__ __forceinline__ bool bm_amax_arrive(float mx, float* part_dst, unsigned* ticket, unsigned nblocks,
                                               BmFoldLds<float, WAVES>& sh) {
    bm_wave_to_lds(bm_wave_max(mx), sh.wave[0]);
    __syncthreads();
    if (threadIdx.x == 0) bm_store_partial(part_dst, bm_pairwise<WAVES>(sh.wave[0], bm_max2));
    return bm_last_arriver(ticket, nblocks, &sh.last);      // its barrier also stands behind thread 0's reads of sh.wave
}
// The folds of partial maxima by ONE workgroup of WAVES wavefronts, the last thing it does with `sh` (one barrier, none
// behind the reads): out[0] = the maximum (NaN-ignoring fmaxf; partial maxima are >= 0), out[1 .. BM_AMAX_SHARDS) = 0.
template <int WAVES>
__device__ __forceinline__ void bm_amax_slot_store(float m, float* out, float* sh) {
    bm_wave_to_lds(bm_wave_max(m), sh);
    __syncthreads();
    if (threadIdx.x < BM_AMAX_SHARDS) {
        float v = 0.f;
        if (threadIdx.x == 0) v = bm_pairwise<WAVES>(sh, bm_max2);
        out[threadIdx.x] = v;
    }
}
template <int WAVES>
__device__ __forceinline__ void bm_amax_fold(const float* part, int n, float* out, float* sh) {
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += WAVES * 64) m = fmaxf(m, part[i]);
    bm_amax_slot_store<WAVES>(m, out, sh);
}
// ... of partials part[r * row_stride + k * split_stride], r < rows, k < nsplit (no workspace holds more than 2^31 of
// them): rows_out[r] (nullable) = the maximum over the splits, and the maximum of all into the slot.
template <int WAVES>
__device__ __forceinline__ void bm_amax_fold_rows(const float* part, int rows, int nsplit, int row_stride,
                                                  int split_stride, float* out, float* rows_out, float* sh) {
    float m = 0.f;
    for (int r = threadIdx.x; r < rows; r += WAVES * 64) {
        float v = 0.f;
        for (int k = 0; k < nsplit; ++k) v = fmaxf(v, part[r * row_stride + k * split_stride]);
        if (rows_out) rows_out[r] = v;
        m = fmaxf(m, v);
    }
    bm_amax_slot_store<WAVES>(m, out, sh);
}
