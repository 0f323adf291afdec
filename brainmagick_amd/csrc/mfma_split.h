// What the split-operand MFMA contractions (f16x2: conv_nn_h2w / pack_h2 / gemm_nt_h2w; 3 x bf16: conv_nn_x3 /
// gemm_nt_x3; staging vectors also gemm_nt) share: the scale rule, the operand splits, the buffer descriptor and the
// compile-time loop.  Producer, packer and consumer must apply the scale rule bit for bit the same way, so it lives
// here ONCE.  Its CPU restatements, for the tests: scripts/emulate_f16x2_split.py and scale_from_amax in
// tests/test_host_cpu.py.
#pragma once
#include <utility>
#include "bm_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// N-wide register vectors whose width is a template expression (staging sets)
template <int N> struct FVec { typedef float type __attribute__((ext_vector_type(N))); };
template <int N> struct UVec { typedef unsigned int type __attribute__((ext_vector_type(N))); };

// Power-of-two scale s with amax * s in [2^14, 2^15), and its exact inverse.  amax == 0 / subnormal / inf /
// nan: s = 1 (non-finite operands then propagate through the split as inf / nan like in fp32).
__host__ __device__ __forceinline__ void bm_scale_from_amax(float amax, float& s, float& inv) {
    const unsigned e = (__builtin_bit_cast(unsigned, amax) >> 23) & 0xffu;
    int se = 127;
    if (e != 0u && e != 255u) {
        se = 268 - (int)e;              // 127 + 14 - (e - 127)
        se = se > 253 ? 253 : (se < 1 ? 1 : se);
    }
    s = __builtin_bit_cast(float, (unsigned)se << 23);
    inv = __builtin_bit_cast(float, (unsigned)(254 - se) << 23);
}

// two fp32 values -> scaled f16 pairs: hi = f16(x * s), lo = f16(x * s - hi) (the product is exact, s is a power
// of two; the difference is exact in fp32), written straight into the halves of the packed results: 4 VALU.
// One scale per value; the one-scale form passes the same register twice.
__device__ __forceinline__ void bm_split_pair(float x0, float x1, float s0, float s1, unsigned& hi, unsigned& lo) {
    asm("v_fma_mixlo_f16 %0, %2, %4, 0\n\t"
        "v_fma_mixhi_f16 %0, %3, %5, 0\n\t"
        "v_fma_mixlo_f16 %1, %2, %4, -%0 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %1, %3, %5, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(hi), "=&v"(lo)
        : "v"(x0), "v"(x1), "v"(s0), "v"(s1));
}
__device__ __forceinline__ void bm_split_pair(float x0, float x1, float s, unsigned& hi, unsigned& lo) {
    bm_split_pair(x0, x1, s, s, hi, lo);
}

// exact 3-way split of 8 fp32 values into bf16 planes (hi, mid, lo).  LATE_LO only moves the last subtraction behind
// the stores of hi and mid: the same values, but the statement order reaches the instruction scheduler, and each of
// the two callers (conv_nn_x3: false, gemm_nt_x3: true) keeps the order its kernels were measured with.
template <bool LATE_LO>
__device__ __forceinline__ void bm_split8_bf16(const float* f, u32x4& hi, u32x4& mid, u32x4& lo) {
    bf16x8 h, m, l;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const __bf16 a = (__bf16)f[i];
        const float r1 = f[i] - (float)a;
        const __bf16 b = (__bf16)r1;
        if constexpr (LATE_LO) {
            h[i] = a; m[i] = b; l[i] = (__bf16)(r1 - (float)b);
        } else {
            const float r2 = r1 - (float)b;
            h[i] = a; m[i] = b; l[i] = (__bf16)r2;
        }
    }
    hi = __builtin_bit_cast(u32x4, h);
    mid = __builtin_bit_cast(u32x4, m);
    lo = __builtin_bit_cast(u32x4, l);
}

// wave-uniform buffer descriptor over `bytes` bytes at p: out-of-range dwords (rows past the end, t < 0 on the
// first row) read as 0 without any per-lane predicate
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bm_buffer_rsrc(const void* p, unsigned bytes) {
    const unsigned long long u = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0,
                                             __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a compile-time constant
template <int... I, class F>
__device__ __forceinline__ void bm_static_for_impl(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void bm_static_for(F&& f) {
    bm_static_for_impl(std::make_integer_sequence<int, N>{}, f);
}
