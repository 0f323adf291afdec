// What the one-launch kernels with a last-arriver fold share (regress.hip, encode.hip): the scalar / 16-byte vector
// instantiation of an element walk, and the ticket by which the workgroup that finishes last folds the others' partials.
#pragma once
#include "bm_common.h"

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
