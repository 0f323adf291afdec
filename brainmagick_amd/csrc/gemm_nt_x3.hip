// fp32-ACCURATE time-contraction GEMM on the bf16 matrix cores (compute mode "f32x3", see
// conv_nn_x3.hip): both operands are split exactly into three bf16 planes while they are staged into
// LDS and every 32x32x16 block is evaluated as six bf16 MFMAs (lo*hi, hi*lo, mid*mid, mid*hi, hi*mid,
// hi*hi) with fp32 accumulation.
//
//   part[g, split][m][c*KS + j] = sum_{s in group g} sum_t A[s][m][t] * X[s][c][t + (j - KS/2)*dil]
//
// LDS: rows of 32 samples = 4 slots of 16 bytes, slot index XOR-swizzled with bits 2-3 of the row so that
// both the row-per-lane ds_read_b128 of the MFMA operands and the 8-lane ds_write_b128 groups of the
// staging pass are bank-conflict free (a +1 pad slot made the writes 2-way); three planes per operand, one pre-shifted
// copy of the X tile per tap.  Software pipeline as in gemm_nt.hip; split-K, grouping, XCD mapping and the partial
// tiles are gemm_nt_common.h's.
#include "gemm_nt_common.h"

#define SLOTS 4          // 16-byte data slots per row, XOR-swizzled: slot (row, q) lives at row*4 + (q ^ ((row >> 2) & 3))
#define SWZ(ROW_, Q_) ((ROW_) * SLOTS + ((Q_) ^ (((ROW_) >> 2) & 3)))

template <int WM, int WC, int MT, int NT, int KS>
__global__ __launch_bounds__(WM * WC * 64, (MT * NT * KS <= 3) ? 3 : 2) void gemm_nt_x3_kernel(GemmNTArgs a) {
    constexpr int NW = WM * WC;
    constexpr int NTH = NW * 64;
    constexpr int BM = WM * MT * 32;
    constexpr int BC = WC * NT * 32;
    constexpr int AIT = BM * SLOTS / NTH;             // 8-sample items per thread (A)
    constexpr int XPT = BC * SLOTS / NTH;             // 8-sample items per thread and tap (X)
    constexpr int XIT = KS * XPT;
    static_assert((BM * SLOTS) % NTH == 0 && (BC * SLOTS) % NTH == 0, "tiles must split evenly over the threads");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    u32x4* As = reinterpret_cast<u32x4*>(smem);       // [3 planes][BM][SLOTS]
    u32x4* Xs = As + 3 * BM * SLOTS;                  // [3 planes][KS][BC][SLOTS]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WC, wc = wave % WC;
    const int nl = lane & 31, h = lane >> 5;

    const GemmNTWork w = gemm_nt_work<BM, BC>(a);
    const int m0 = w.m0, c0 = w.c0, s_begin = w.s_begin, cps = w.cps;
    const long q_begin = w.q_begin, q_end = w.q_end;
    const int halo = (KS >> 1) * a.dil;
    const int a_bytes = (int)(((long)(a.M - 1) * a.a_rstride + a.T) * 4);
    const int x_bytes = (int)(((long)(a.Cn - 1) * a.x_rstride + a.T) * 4);

    f32x16 acc[MT][NT][KS];
    gemm_nt_zero(acc);

    typename FVec<8 * AIT>::type areg;
    typename FVec<8 * XIT>::type xreg;

    // per-thread element offsets inside a segment (row * stride + 8 * slot), fixed for the whole kernel
    int a_off[AIT], x_off[XPT];
#pragma unroll
    for (int i = 0; i < AIT; ++i) {
        const int e = tid + i * NTH;
        a_off[i] = (m0 + (e >> 2)) * (int)a.a_rstride + 8 * (e & 3);
    }
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
        const int e = tid + i * NTH;
        x_off[i] = (c0 + (e >> 2)) * (int)a.x_rstride + 8 * (e & 3);
    }

    // interior chunks: 8 consecutive samples starting at element offset OFF_ (>= 0) of the segment behind
    // RS_ as two dwordx4 buffer loads (dword alignment is all the hardware asks for, so every tap shift
    // takes this path); rows past the end of the segment come back as 0 from the buffer bounds check
#define LOAD8(DST_, D0_, RS_, OFF_)                                                               \
    {                                                                                             \
        const u32x4 v0 = __builtin_amdgcn_raw_buffer_load_b128(RS_, (OFF_) * 4, 0, 0);            \
        const u32x4 v1 = __builtin_amdgcn_raw_buffer_load_b128(RS_, (OFF_) * 4 + 16, 0, 0);       \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                           \
            DST_[D0_ + r] = __uint_as_float(v0[r]);                                               \
            DST_[D0_ + 4 + r] = __uint_as_float(v1[r]);                                           \
        }                                                                                         \
    }
    // edge chunks (wave-uniform, the first / last chunks of a segment): one dword per sample, samples whose
    // time index falls outside [0, T) get an out-of-range offset and therefore read as 0.  (A negative
    // voffset must never meet a positive immediate offset: the bounds check does not wrap.)
#define LOAD8E(DST_, D0_, RS_, OFF_, T_)                                                          \
    {                                                                                             \
        _Pragma("unroll") for (int r = 0; r < 8; ++r) {                                           \
            const int tt = (T_) + r;                                                              \
            const int off = (tt >= 0 && tt < a.T) ? ((OFF_) + r) * 4 : 0x7ffffff0;                \
            DST_[D0_ + r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(RS_, off, 0, 0)); \
        }                                                                                         \
    }
#define NT_LOAD()        /* stages chunk (ld_s, ld_c) and advances the cursor */                  \
    {                                                                                             \
        const int t0 = ld_c * BKT;                                                                \
        int sidx = s_begin + ld_s;                                                                \
        if (a.order) sidx = a.order[sidx];                                                        \
        const __amdgpu_buffer_rsrc_t ra = bm_buffer_rsrc(a.a + (long)sidx * a.a_sstride, a_bytes);\
        const __amdgpu_buffer_rsrc_t rx = bm_buffer_rsrc(a.x + (long)sidx * a.x_sstride, x_bytes);\
        if (t0 - halo < 0 || t0 + BKT + halo > a.T) {                                             \
            _Pragma("unroll") for (int i = 0; i < AIT; ++i)                                       \
                LOAD8E(areg, 8 * i, ra, a_off[i] + t0, t0 + 8 * ((tid + i * NTH) & 3))            \
            _Pragma("unroll") for (int j = 0; j < KS; ++j) {                                      \
                const int shift = (j - (KS >> 1)) * a.dil;                                        \
                _Pragma("unroll") for (int i = 0; i < XPT; ++i)                                   \
                    LOAD8E(xreg, 8 * (j * XPT + i), rx, x_off[i] + t0 + shift,                    \
                           t0 + shift + 8 * ((tid + i * NTH) & 3))                                \
            }                                                                                     \
        } else {                                                                                  \
            _Pragma("unroll") for (int i = 0; i < AIT; ++i) LOAD8(areg, 8 * i, ra, a_off[i] + t0)  \
            _Pragma("unroll") for (int j = 0; j < KS; ++j) {                                      \
                const int shift = (j - (KS >> 1)) * a.dil;                                        \
                _Pragma("unroll") for (int i = 0; i < XPT; ++i)                                   \
                    LOAD8(xreg, 8 * (j * XPT + i), rx, x_off[i] + t0 + shift)                     \
            }                                                                                     \
        }                                                                                         \
        if (++ld_c == cps) { ld_c = 0; ++ld_s; }                                                  \
    }
#define NT_STORE()                                                                                \
    {                                                                                             \
        _Pragma("unroll") for (int i = 0; i < AIT; ++i) {                                         \
            const int e = tid + i * NTH;                                                          \
            float f[8];                                                                           \
            _Pragma("unroll") for (int r = 0; r < 8; ++r) f[r] = areg[8 * i + r];                 \
            u32x4 hi, mid, lo;                                                                    \
            bm_split8_bf16<true>(f, hi, mid, lo);                                                 \
            const int slot = SWZ(e >> 2, e & 3);                                                  \
            As[slot] = hi; As[BM * SLOTS + slot] = mid; As[2 * BM * SLOTS + slot] = lo;           \
        }                                                                                         \
        _Pragma("unroll") for (int j = 0; j < KS; ++j)                                            \
            _Pragma("unroll") for (int i = 0; i < XPT; ++i) {                                     \
                const int e = tid + i * NTH;                                                      \
                float f[8];                                                                       \
                _Pragma("unroll") for (int r = 0; r < 8; ++r) f[r] = xreg[8 * (j * XPT + i) + r]; \
                u32x4 hi, mid, lo;                                                                \
                bm_split8_bf16<true>(f, hi, mid, lo);                                             \
                const int slot = j * BC * SLOTS + SWZ(e >> 2, e & 3);                             \
                Xs[slot] = hi; Xs[KS * BC * SLOTS + slot] = mid; Xs[2 * KS * BC * SLOTS + slot] = lo; \
            }                                                                                     \
    }

    int ld_s = (int)(q_begin / cps);
    int ld_c = (int)(q_begin - (long)ld_s * cps);
    if (q_begin < q_end) {
        NT_LOAD();
        NT_STORE();
    }
    __syncthreads();
    for (long q = q_begin; q < q_end; ++q) {
        const bool more = q + 1 < q_end;
        if (more) NT_LOAD();
        // row-per-lane operand reads; rows of the 32-row MFMA blocks start at multiples of 32, so the
        // swizzle term only depends on the lane's row-in-block nl
        const u32x4* ap = As + (wm * MT * 32 + nl) * SLOTS;
        const u32x4* xp = Xs + (wc * NT * 32 + nl) * SLOTS;
        const int sw = (nl >> 2) & 3;
        constexpr int APL = BM * SLOTS, XPL = KS * BC * SLOTS;      // plane strides
#pragma unroll
        for (int kk = 0; kk < BKT / 16; ++kk) {
            bf16x8 ah[MT], am[MT], al[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int q = (2 * kk + h) ^ sw;
                ah[i] = __builtin_bit_cast(bf16x8, ap[i * 32 * SLOTS + q]);
                am[i] = __builtin_bit_cast(bf16x8, ap[APL + i * 32 * SLOTS + q]);
                al[i] = __builtin_bit_cast(bf16x8, ap[2 * APL + i * 32 * SLOTS + q]);
            }
#pragma unroll
            for (int k = 0; k < NT; ++k) {
#pragma unroll
                for (int j = 0; j < KS; ++j) {
                    const int o = (j * BC + k * 32) * SLOTS + ((2 * kk + h) ^ sw);
                    const bf16x8 bh = __builtin_bit_cast(bf16x8, xp[o]);
                    const bf16x8 bm = __builtin_bit_cast(bf16x8, xp[XPL + o]);
                    const bf16x8 bl = __builtin_bit_cast(bf16x8, xp[2 * XPL + o]);
#pragma unroll
                    for (int i = 0; i < MT; ++i) {
                        f32x16 c = acc[i][k][j];
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bm, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bh, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bm, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh, c, 0, 0, 0);
                        acc[i][k][j] = c;
                    }
                }
            }
        }
        __syncthreads();
        if (more) {
            NT_STORE();
            __syncthreads();
        }
    }
#undef NT_LOAD
#undef NT_STORE
#undef LOAD8
#undef LOAD8E

    gemm_nt_store_partial<WM, WC, MT, NT, KS>(a, w, acc);
}

struct GemmNTX3 {
    static constexpr const char* name = "gemm_nt_x3";
    template <int WM, int WC, int MT, int NT, int KS>
    static int launch(const GemmNTArgs& a, hipStream_t stream) {
        constexpr int BM = WM * MT * 32, BC = WC * NT * 32;
        return gemm_nt_launch(gemm_nt_x3_kernel<WM, WC, MT, NT, KS>, a, BM, BC, WM * WC * 64,
                              (size_t)3 * (BM + KS * BC) * SLOTS * 16, name, stream);
    }
};

// Same contract as bm_gemm_nt (fp32 partial tiles out); fp32-accurate 3-plane bf16 emulation.
extern "C" int bm_gemm_nt_x3(const float* a, long a_sstride, long a_rstride, const float* x,
                               long x_sstride, long x_rstride, const int* order, const int* seg,
                               float* part, int S, int G, int M, int Cn, int T, int KS, int dil,
                               int nsplit, void* stream) {
    GemmNTArgs g;
    if (int e = gemm_nt_fill_args(g, GemmNTX3::name, a, a_sstride, a_rstride, x, x_sstride, x_rstride, order, seg, part,
                                  S, G, M, Cn, T, dil, nsplit))
        return e;
    // The staging addresses are 32-bit byte offsets into one segment (buffer descriptors).  An operand whose
    // segment spans 2 GB or more (e.g. 2 048 wav2vec candidates x 368 640 samples on 8 GPUs) goes through the
    // exact-fp32 kernel, which addresses with 64-bit pointers (same contract, at least as accurate).
    if (((long)(M - 1) * a_rstride + T) * 4 >= 0x7fffff00L || ((long)(Cn - 1) * x_rstride + T) * 4 >= 0x7fffff00L)
        return bm_gemm_nt(a, a_sstride, a_rstride, x, x_sstride, x_rstride, order, seg, part, S, G, M, Cn, T, KS,
                          dil, nsplit, stream);
    return gemm_nt_launch_tile<GemmNTX3>(g, KS, (hipStream_t)stream);
}
