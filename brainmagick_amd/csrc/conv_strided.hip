// Strided and transposed 1-D convolutions (nn.Conv1d with stride, nn.ConvTranspose1d: bm/models/common.py:96,
// 112-114) and their weight gradient, on exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) like conv_nn.hip / gemm_nt.hip.
// fp32 tensors [B][C][T], T fastest.
//
//   gather form   y[b][m][u] = ep( bias[m] + sum_{c,j} W[m][c][j] * x[b][c][u*s + j*dil - pad] )
//                 forward of the strided conv, data gradient of the transposed conv
//   scatter form  y[b][m][t] = ep( bias[m] + sum_{c,j} W[c][m][j] * x[b][c][(t + pad - j*dil) / s] )   (integer indices only)
//                 forward of the transposed conv, data gradient of the strided conv
//   weight grad   out[r][q][j] = sum_{b,u} A[b][r][u] * X[b][q][u*s + j*dil - pad]
//                 strided layer: A = dY, X = x -> dW[m][c][j];  transposed layer: A = x, X = dY -> dW[c][m][j]
//
// Both data forms run in ONE kernel that only knows stride-1 reads.  Write an input index as v*s + r (phase r = index
// mod s).  Gather form: tap j reads x[(u + q_j)*s + r_j] with j*dil - pad = q_j*s + r_j, i.e. column u + q_j of the
// phase-r_j sub-sequence of x.  The staged window of x (width s*(128 + span) ~ 128*s + dil*(K-1), once per channel
// chunk, shared by all taps as in conv_nn.hip) is therefore DE-INTERLEAVED when it is written to LDS -- row layout
// [phase][column] -- and every B-fragment read is 32 consecutive floats: the lane stride of s that the strided read
// would carry (2-way / 4-way bank conflicts at s = 2 / 4) never reaches the LDS.  Scatter form: the output is split
// into its s phases t = v*s + p; phase p only sees the taps with (p + pad - j*dil) divisible by s -- an arithmetic
// progression j0, j0 + jstep, ... -- and reads x[v + e_j]: a stride-1 conv with a tap subset.  A tile owns 128 columns
// of ONE output phase, so every output element has exactly one owner (no atomics); a phase without taps is bias only.
//
// Tiling as conv_nn.hip: 4 wavefronts, [32*MT] x [128] tile, weights pre-packed by pack.hip as [chunk][tap][16][Mpad],
// software pipeline through registers into double-buffered LDS, one barrier per (chunk, tap) stage.  The A-slab staging
// and the epilogue are conv_common.h's, shared with conv_nn.hip: conv_tile_epilogue (bias, pre-activation output,
// affine, activation, per-tile BatchNorm sums in the [tiles][M][2] layout that bm_bn_finalize reads), called with the
// tile's column mapping.  Above the kernels one pair of autograd functions serves both families
// (functional.Conv1dFn / ConvBNActFn).
#include "conv_common.h"
#include "mfma_split.h"

struct ConvStridedArgs {
    ConvNNArgs c;          // c.T = OUTPUT length (row pitch of y); c.ntiles_n = column tiles per segment, all phases
    int Tin;               // input length (row pitch of x)
    int stride, pad, scatter;
    int si;                // phases of the staged input window: stride (gather) or 1 (scatter)
    int so;                // output phases: 1 (gather) or stride (scatter)
    int qmin;              // smallest column offset of any tap
    int PW;                // columns per phase in the window = 128 + qmax - qmin
    int ntiles_v;          // column tiles per output phase
    BmFastDiv fsi;
};

// XP = 64-lane passes per staged window row (window <= 64 * XP floats)
template <int MT, int XP>
__global__ __launch_bounds__(256, 2) void conv_strided_kernel(ConvStridedArgs g) {
    const ConvNNArgs& a = g.c;
    constexpr int BM = 32 * MT;
    constexpr int BN = 128;
    constexpr int BKC = BM_BKC;
    constexpr int Q = BM / 4;                         // float4 per A row
    constexpr int AREG = (BKC * Q + 255) / 256;       // float4 per thread per (chunk, tap) A slab
    static_assert(AREG <= 2 && BKC == 16, "staging register set");
    typedef typename FVec<4 * XP>::type xvec_t;       // 4 rows per wavefront x XP passes
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nl = lane & 31;
    const int h = lane >> 5;

    int id = bm_xcd_remap(blockIdx.x, gridDim.x);
    const int mtile = id % a.ntiles_m;
    id /= a.ntiles_m;
    const int ntile = id % a.ntiles_n;
    const int b = id / a.ntiles_n;
    const int p = ntile / g.ntiles_v;                 // output phase (0 in the gather form)
    const int v0 = (ntile - p * g.ntiles_v) * BN;     // first column of the tile inside its phase
    const int m0 = mtile * BM;

    // taps of this tile: j0, j0 + jstep, ... (nv of them)
    int j0 = 0, jstep = 1, nv = a.KS;
    if (g.scatter) {
        int gc = a.dil, r = g.stride;
        while (r) { const int t = gc % r; gc = r; r = t; }       // gcd(dil, stride)
        jstep = g.stride / gc;
        j0 = -1;
        for (int j = 0; j < a.KS && j < jstep; ++j)
            if ((p + g.pad - j * a.dil) % g.stride == 0) { j0 = j; break; }
        nv = j0 < 0 ? 0 : (a.KS - 1 - j0) / jstep + 1;
    }

    const int W = g.si * g.PW;                        // staged floats per channel row
    const int XWP = W;
    const int t_start = (v0 + g.qmin) * g.si;         // input index of window element 0
    float* As = smem;                                 // two A slabs [BKC][BM]
    float* Xs = smem + 2 * BKC * BM;                  // two windows [BKC][si][PW]

    const float* xb = a.x + (long)b * a.x_bstride;

    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;

    float4 a0 = make_float4(0, 0, 0, 0), a1 = a0;
    xvec_t xr;
#pragma unroll
    for (int k = 0; k < 4 * XP; ++k) xr[k] = 0.f;
    const int nstage = a.nchunk * nv;

    // column of a float4 inside the slab row: rows past Mpad feed discarded outputs
#define BS_COL (m0 + q * 4 <= a.Mpad - 4 ? m0 + q * 4 : a.Mpad - 4)
#define BS_LOAD_A(CHUNK_, J_)                                                                     \
    {                                                                                             \
        const float* wsrc = a.wp + ((long)(CHUNK_) * a.KS + (J_)) * BKC * a.Mpad;                 \
        CONV_A_LOAD1(0, a0, wsrc, BS_COL) CONV_A_LOAD1(1, a1, wsrc, BS_COL)                       \
    }
#define BS_PUT_A(BUF_)                                                                            \
    {                                                                                             \
        float* dst = As + (BUF_) * BKC * BM;                                                      \
        CONV_A_STORE1(0, a0, dst) CONV_A_STORE1(1, a1, dst)                                       \
    }
#define BS_LOAD_X(CHUNK_)                                                                         \
    {                                                                                             \
        const int c0 = (CHUNK_) * BKC;                                                            \
        _Pragma("unroll") for (int k = 0; k < XP; ++k) {                                          \
            const int i = lane + k * 64;                                                          \
            const int t = t_start + i;                                                            \
            const bool ok = i < W && t >= 0 && t < g.Tin;                                         \
            _Pragma("unroll") for (int rr = 0; rr < 4; ++rr) {                                    \
                const int c = c0 + wave + rr * 4;                                                 \
                xr[rr * XP + k] = (ok && c < a.Cin) ? xb[(long)c * g.Tin + t] : 0.f;              \
            }                                                                                     \
        }                                                                                         \
    }
#define BS_PUT_X(BUF_)                                                                          \
    {                                                                                             \
        float* dst = Xs + (BUF_) * BKC * XWP;                                                     \
        _Pragma("unroll") for (int k = 0; k < XP; ++k) {                                          \
            const int i = lane + k * 64;                                                          \
            const int v = (int)bm_div((unsigned)i, g.fsi);                                        \
            const int off = (i - v * g.si) * g.PW + v;        /* [phase][column] */               \
            if (i < W) {                                                                          \
                _Pragma("unroll") for (int rr = 0; rr < 4; ++rr)                                  \
                    dst[(wave + rr * 4) * XWP + off] = xr[rr * XP + k];                           \
            }                                                                                     \
        }                                                                                         \
    }

    if (nstage > 0) {
        BS_LOAD_A(0, j0);
        BS_LOAD_X(0);
        BS_PUT_A(0);
        BS_PUT_X(0);
        __syncthreads();
        int s = 0;
        for (int chunk = 0; chunk < a.nchunk; ++chunk) {
            const float* xbuf = Xs + (chunk & 1) * BKC * XWP;
            for (int i = 0; i < nv; ++i, ++s) {
                const int j = j0 + i * jstep;
                const bool last_tap = i == nv - 1;
                const int nc = last_tap ? chunk + 1 : chunk;
                const int nj = last_tap ? j0 : j + jstep;
                const bool more_a = nc < a.nchunk;
                const bool more_x = last_tap && more_a;
                if (more_a) BS_LOAD_A(nc, nj);
                if (more_x) BS_LOAD_X(chunk + 1);
                // tap j -> (phase, column offset) inside the de-interleaved window
                int ph = 0, q;
                if (g.scatter) {
                    q = (p + g.pad - j * a.dil) / g.stride;          // exact by the choice of j
                } else {
                    const int o = j * a.dil - g.pad;
                    q = bm_floordiv(o, g.stride);
                    ph = o - q * g.stride;
                }
                // ---- MFMA: k runs over channel pairs; lanes 0-31 feed k even, 32-63 k odd ----
                const float* xrow = xbuf + h * XWP + ph * g.PW + (q - g.qmin) + wave * 32 + nl;
                const float* arow = As + (s & 1) * BKC * BM + h * BM + nl;
#pragma unroll
                for (int pp = 0; pp < BKC / 2; ++pp) {
                    const float bv = xrow[2 * pp * XWP];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const float av = arow[2 * pp * BM + mt * 32];
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[mt], 0, 0, 0);
                    }
                }
                if (more_a) BS_PUT_A((s + 1) & 1);
                if (more_x) BS_PUT_X((chunk + 1) & 1);
                __syncthreads();
            }
        }
    }
#undef BS_COL
#undef BS_LOAD_A
#undef BS_PUT_A
#undef BS_LOAD_X
#undef BS_PUT_X

    // the tile's columns are those of ONE output phase: t = v * so + p
    conv_tile_epilogue<MT>(a, acc, smem, b, ntile, m0, v0, tid, g.so, p);
}

template <int MT, int XP>
static int launch_conv_strided_x(const ConvStridedArgs& g, hipStream_t stream) {
    constexpr int BM = 32 * MT;
    const int W = g.si * g.PW;
    size_t lds = (size_t)(2 * BM_BKC * BM + 2 * BM_BKC * W) * sizeof(float);
    const size_t lds_ep = (size_t)(11 * BM) * sizeof(float);
    if (lds < lds_ep) lds = lds_ep;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(conv_strided_kernel<MT, XP>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return bm_set_error((int)e, "conv_strided: hipFuncSetAttribute: %s", hipGetErrorString(e));
    }
    const long nblocks = (long)g.c.B * g.c.ntiles_n * g.c.ntiles_m;
    if (nblocks <= 0) return BM_OK;
    hipLaunchKernelGGL((conv_strided_kernel<MT, XP>), dim3((unsigned)nblocks), dim3(256), lds, stream, g);
    return bm_check_launch("conv_strided");
}

template <int MT>
static int launch_conv_strided(const ConvStridedArgs& g, hipStream_t stream) {
    const int W = g.si * g.PW;
    if (W <= 192) return launch_conv_strided_x<MT, 3>(g, stream);
    if (W <= 320) return launch_conv_strided_x<MT, 5>(g, stream);
    if (W <= 576) return launch_conv_strided_x<MT, 9>(g, stream);
    return bm_set_error(BM_ERR_UNSUPPORTED,
                        "conv_strided: the staged window of %d floats per channel (stride * (128 + tap span)) exceeds 576", W);
}

// Row-tile height (32-row MFMA blocks) of the strided family: 1, 2 or 4.
static int strided_mt_for(int M) { return M <= 32 ? 1 : (M <= 64 ? 2 : 4); }

extern "C" int bm_conv_mpad(int M);

// Output length of nn.Conv1d (transposed = 0) / nn.ConvTranspose1d with output_padding 0 (transposed = 1) for an input
// of T samples; < 1 means torch refuses the shape.
extern "C" int bm_conv1d_out_len(int T, int KS, int stride, int dil, int pad, int transposed) {
    if (transposed) return (T - 1) * stride - 2 * pad + dil * (KS - 1) + 1;
    const int span = T + 2 * pad - dil * (KS - 1) - 1;
    return span < 0 ? 0 : span / stride + 1;
}

// Number of [M][2] partial-statistics tiles that a launch with `stats` writes (all of them are written).
extern "C" int bm_conv_strided_stats_tiles(int B, int Tout, int stride, int transposed) {
    const int so = transposed ? stride : 1;
    return B * so * cdiv(cdiv(Tout, so), 128);
}

static int conv_strided_common(int scatter, const float* x, long x_bstride, const float* wpacked, const float* bias,
                               const float* ep_scale, const float* ep_shift, float* y_pre, float* y_out,
                               long y_bstride, float* stats, int B, int Cin, int M, int T, int Tout, int KS,
                               int stride, int dil, int pad, int act, float leak, void* stream) {
    BM_REQUIRE(KS >= 1 && stride >= 1 && dil >= 1 && pad >= 0, "conv_strided: bad geometry K=%d s=%d dil=%d pad=%d",
               KS, stride, dil, pad);
    BM_REQUIRE(T > 0, "conv_strided: bad dims");
    ConvStridedArgs g;
    ConvNNArgs& a = g.c;
    // a.T = the OUTPUT length; no weight groups, no residual
    if (int e = conv_nn_fill_args(a, "conv_strided", x, x_bstride, wpacked, nullptr, bias, 0, ep_scale, ep_shift, nullptr, 0,
                                  y_pre, y_out, y_bstride, stats, B, Cin, M, Tout, KS, dil, act, leak))
        return e;
    BM_REQUIRE((long)M * Tout < (1L << 31) && (long)Cin * T < (1L << 31), "conv_strided: a segment exceeds 2^31 elements");
    const int mt = strided_mt_for(M);
    a.Mpad = bm_conv_mpad(M);
    a.nchunk = cdiv(Cin, BM_BKC);
    a.ntiles_m = cdiv(M, 32 * mt);
    g.Tin = T; g.stride = stride; g.pad = pad; g.scatter = scatter;
    int qmax;
    if (scatter) {
        g.si = 1; g.so = stride;
        g.qmin = bm_floordiv(pad - (KS - 1) * dil, stride);
        qmax = bm_floordiv(stride - 1 + pad, stride);
    } else {
        g.si = stride; g.so = 1;
        g.qmin = bm_floordiv(-pad, stride);
        qmax = bm_floordiv((KS - 1) * dil - pad, stride);
    }
    g.PW = 128 + qmax - g.qmin;
    g.ntiles_v = cdiv(cdiv(Tout, g.so), 128);
    a.ntiles_n = g.so * g.ntiles_v;
    g.fsi = bm_fastdiv((unsigned)g.si);
    hipStream_t s = (hipStream_t)stream;
    switch (mt) {
        case 1: return launch_conv_strided<1>(g, s);
        case 2: return launch_conv_strided<2>(g, s);
        default: return launch_conv_strided<4>(g, s);
    }
}

// C-ABI: nn.Conv1d with stride (bm/models/common.py:96, 112-114) -- and, with Tout = the layer's input length, the
// data gradient of nn.ConvTranspose1d.  Weights packed by bm_pack_weights as rows = output channels.
extern "C" int bm_conv1d_strided(const float* x, long x_bstride, const float* wpacked, const float* bias,
                                 const float* ep_scale, const float* ep_shift, float* y_pre, float* y_out,
                                 long y_bstride, float* stats, int B, int Cin, int M, int T, int Tout, int KS,
                                 int stride, int dil, int pad, int act, float leak, void* stream) {
    return conv_strided_common(0, x, x_bstride, wpacked, bias, ep_scale, ep_shift, y_pre, y_out, y_bstride, stats, B,
                               Cin, M, T, Tout, KS, stride, dil, pad, act, leak, stream);
}

// C-ABI: nn.ConvTranspose1d, output_padding 0 (bm/models/common.py:96, 112-114) -- and, with Tout = the layer's input
// length, the data gradient of the strided nn.Conv1d.
extern "C" int bm_conv1d_transposed(const float* x, long x_bstride, const float* wpacked, const float* bias,
                                    const float* ep_scale, const float* ep_shift, float* y_pre, float* y_out,
                                    long y_bstride, float* stats, int B, int Cin, int M, int T, int Tout, int KS,
                                    int stride, int dil, int pad, int act, float leak, void* stream) {
    return conv_strided_common(1, x, x_bstride, wpacked, bias, ep_scale, ep_shift, y_pre, y_out, y_bstride, stats, B,
                               Cin, M, T, Tout, KS, stride, dil, pad, act, leak, stream);
}

// ------------------------------------------------------------------------------------------------------------------
// Weight gradient.  A workgroup is 2 x 2 wavefronts and owns a 64 (rows of A) x 64 (rows of X) tile of TJ taps; the
// reduction runs over a flat list of (segment, 32-column chunk of u) pairs shared by `nsplit` workgroups that write
// separate partial tiles (folded in a fixed order by pack.hip's bm_reduce_splits).  The window of X that a chunk
// needs is de-interleaved by phase in LDS like above, rows at an odd pitch (row-per-lane reads without conflicts).
#define WG_BKT 32

struct WgradArgs {
    const float* a; long a_sstride;        // A[s][r][u], rows U apart
    const float* x; long x_sstride;        // X[s][q][t], rows L apart
    float* part;                            // [nsplit][R][Q * KS]
    int S, R, Q, U, L, KS, stride, dil, pad, nsplit;
    int tiles_r, tiles_q, ngroups;
    int qmin, PW, W, PX;
    BmFastDiv fW, fsi;
};

template <int TJ, int XVN>
__global__ __launch_bounds__(256) void conv_strided_wgrad_kernel(WgradArgs a) {
    constexpr int BM = 64, BC = 64, NTH = 256;
    constexpr int PA = WG_BKT + 1;
    constexpr int AVN = BM * WG_BKT / NTH;
    typedef typename FVec<AVN>::type avec_t;
    typedef typename FVec<XVN>::type xvec_t;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wc = wave & 1;
    const int nl = lane & 31, h = lane >> 5;
    float* As = smem;                       // [BM][PA]
    float* Xs = smem + BM * PA;             // [BC][PX]

    int id = bm_xcd_remap(blockIdx.x, gridDim.x);
    const int tr = id % a.tiles_r; id /= a.tiles_r;
    const int tq = id % a.tiles_q; id /= a.tiles_q;
    const int jg = id % a.ngroups;
    const int split = id / a.ngroups;
    const int r0 = tr * BM, q0 = tq * BC, jbase = jg * TJ;

    const int cps = (a.U + WG_BKT - 1) / WG_BKT;
    const long nchunks = (long)a.S * cps;
    const long c_begin = nchunks * split / a.nsplit;
    const long c_end = nchunks * (split + 1) / a.nsplit;

    // taps of this workgroup -> offset of (phase, column) inside a window row; a tap past KS repeats the last one
    int toff[TJ];
#pragma unroll
    for (int jj = 0; jj < TJ; ++jj) {
        const int j = jbase + jj < a.KS ? jbase + jj : a.KS - 1;
        const int o = j * a.dil - a.pad;
        const int q = bm_floordiv(o, a.stride);
        toff[jj] = (o - q * a.stride) * a.PW + (q - a.qmin);
    }

    f32x16 acc[TJ];
#pragma unroll
    for (int jj = 0; jj < TJ; ++jj)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[jj][r] = 0.f;

    avec_t areg;
    xvec_t xreg;
    int u0 = 0;

#define WG_LOAD(C_)                                                                               \
    {                                                                                             \
        const int sl = (int)((C_) / cps);                                                         \
        u0 = (int)((C_) - (long)sl * cps) * WG_BKT;                                               \
        const float* ab = a.a + (long)sl * a.a_sstride;                                           \
        const float* xb = a.x + (long)sl * a.x_sstride;                                           \
        _Pragma("unroll") for (int k = 0; k < AVN; ++k) {                                         \
            const int r = r0 + (tid >> 5) + k * (NTH / 32);                                       \
            const int u = u0 + (tid & 31);                                                        \
            areg[k] = (r < a.R && u < a.U) ? ab[(long)r * a.U + u] : 0.f;                         \
        }                                                                                         \
        const int ts = (u0 + a.qmin) * a.stride;                                                  \
        _Pragma("unroll") for (int k = 0; k < XVN; ++k) {                                         \
            const int e = tid + k * NTH;                                                          \
            const int i = (int)bm_div((unsigned)e, a.fW);                                         \
            const int t = ts + e - i * a.W;                                                       \
            const int q = q0 + i;                                                                 \
            xreg[k] = (i < BC && q < a.Q && t >= 0 && t < a.L) ? xb[(long)q * a.L + t] : 0.f;     \
        }                                                                                         \
    }
#define WG_STORE()                                                                                \
    {                                                                                             \
        _Pragma("unroll") for (int k = 0; k < AVN; ++k)                                           \
            As[((tid >> 5) + k * (NTH / 32)) * PA + (tid & 31)] = areg[k];                        \
        _Pragma("unroll") for (int k = 0; k < XVN; ++k) {                                         \
            const int e = tid + k * NTH;                                                          \
            const int i = (int)bm_div((unsigned)e, a.fW);                                         \
            const int xx = e - i * a.W;                                                           \
            const int v = (int)bm_div((unsigned)xx, a.fsi);                                       \
            if (i < BC) Xs[i * a.PX + (xx - v * a.stride) * a.PW + v] = xreg[k];                  \
        }                                                                                         \
    }

    if (c_begin < c_end) {
        WG_LOAD(c_begin);
        WG_STORE();
    }
    __syncthreads();
    for (long c = c_begin; c < c_end; ++c) {
        const int uvalid = min(WG_BKT, a.U - u0);
        const int ksteps = (uvalid + 1) >> 1;
        const bool more = c + 1 < c_end;
        if (more) WG_LOAD(c + 1);              // in flight during the MFMAs below (u0 now = next chunk)
        const float* ap = As + (wm * 32 + nl) * PA + h;
        const float* xp = Xs + (wc * 32 + nl) * a.PX + h;
#define WG_KSTEP(KK_)                                                                             \
    {                                                                                             \
        const float av = ap[2 * (KK_)];                                                           \
        _Pragma("unroll") for (int jj = 0; jj < TJ; ++jj) {                                       \
            const float bv = xp[2 * (KK_) + toff[jj]];                                            \
            acc[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[jj], 0, 0, 0);             \
        }                                                                                         \
    }
        // groups of 4 k-steps, unrolled; a partial last chunk only runs the groups it needs (the A tile is
        // zero-filled beyond U)
        const int kgroups = (ksteps + 3) >> 2;
        for (int g4 = 0; g4 < kgroups; ++g4) {
            WG_KSTEP(4 * g4 + 0)
            WG_KSTEP(4 * g4 + 1)
            WG_KSTEP(4 * g4 + 2)
            WG_KSTEP(4 * g4 + 3)
        }
#undef WG_KSTEP
        __syncthreads();
        if (more) {
            WG_STORE();
            __syncthreads();
        }
    }
#undef WG_LOAD
#undef WG_STORE

    const long N = (long)a.Q * a.KS;
    float* dst = a.part + (long)split * a.R * N;
    const int q = q0 + wc * 32 + nl;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = r0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m < a.R && q < a.Q) {
#pragma unroll
            for (int jj = 0; jj < TJ; ++jj)
                if (jbase + jj < a.KS) dst[(long)m * N + (long)q * a.KS + jbase + jj] = acc[jj][r];
        }
    }
}

template <int TJ, int XVN>
static int launch_wgrad_x(const WgradArgs& a, hipStream_t stream) {
    const size_t lds = (size_t)(64 * (WG_BKT + 1) + 64 * a.PX) * sizeof(float);
    const long nblocks = (long)a.tiles_r * a.tiles_q * a.ngroups * a.nsplit;
    if (nblocks <= 0) return BM_OK;
    hipLaunchKernelGGL((conv_strided_wgrad_kernel<TJ, XVN>), dim3((unsigned)nblocks), dim3(256), lds, stream, a);
    return bm_check_launch("conv_strided_wgrad");
}

template <int TJ>
static int launch_wgrad(const WgradArgs& a, hipStream_t stream) {
    if (a.W <= 96) return launch_wgrad_x<TJ, 24>(a, stream);
    if (a.W <= 160) return launch_wgrad_x<TJ, 40>(a, stream);
    return bm_set_error(BM_ERR_UNSUPPORTED,
                        "conv_strided_wgrad: the staged window of %d floats per row (stride * (32 + tap span)) exceeds 160", a.W);
}

// taps per workgroup: the K taps in equal groups of at most 4
static int wgrad_tj_for(int KS) { return cdiv(KS, cdiv(KS, 4)); }

extern "C" int bm_conv1d_strided_wgrad_suggest_splits(int R, int Q, int KS, int S, int U) {
    const long tiles = (long)cdiv(R, 64) * cdiv(Q, 64) * cdiv(KS, wgrad_tj_for(KS));
    const long chunks = (long)S * cdiv(U, WG_BKT);
    long want = (1024 + tiles - 1) / tiles;
    if (want > chunks / 8) want = chunks / 8;     // keep >= 8 chunks of work per workgroup
    if (want < 1) want = 1;
    if (want > 256) want = 256;
    return (int)want;
}

// C-ABI: weight gradient of the strided nn.Conv1d (a = dY [S][R = M][U = Tout], xl = x [S][Q = Cin][L = T] ->
// dW[m][c][j]) and of nn.ConvTranspose1d (a = x [S][R = Cin][U = T], xl = dY [S][Q = M][L = Tout] -> dW[c][m][j]):
// autograd of bm/models/common.py:96, 112-114.  part = [nsplit][R][Q * KS] partial tiles for bm_reduce_splits.
extern "C" int bm_conv1d_strided_wgrad(const float* a, long a_sstride, const float* xl, long xl_sstride, float* part,
                                       int S, int R, int Q, int U, int L, int KS, int stride, int dil, int pad,
                                       int nsplit, void* stream) {
    BM_REQUIRE(a && xl && part, "conv_strided_wgrad: null pointer");
    BM_REQUIRE(S >= 0 && R > 0 && Q > 0 && U > 0 && L > 0 && nsplit > 0, "conv_strided_wgrad: bad dims");
    BM_REQUIRE(KS >= 1 && stride >= 1 && dil >= 1 && pad >= 0, "conv_strided_wgrad: bad geometry K=%d s=%d dil=%d pad=%d",
               KS, stride, dil, pad);
    BM_REQUIRE((long)R * U < (1L << 31) && (long)Q * L < (1L << 31), "conv_strided_wgrad: a segment exceeds 2^31 elements");
    WgradArgs g;
    g.a = a; g.a_sstride = a_sstride; g.x = xl; g.x_sstride = xl_sstride; g.part = part;
    g.S = S; g.R = R; g.Q = Q; g.U = U; g.L = L; g.KS = KS; g.stride = stride; g.dil = dil; g.pad = pad;
    g.nsplit = nsplit;
    const int tj = wgrad_tj_for(KS);
    g.tiles_r = cdiv(R, 64); g.tiles_q = cdiv(Q, 64); g.ngroups = cdiv(KS, tj);
    g.qmin = bm_floordiv(-pad, stride);
    const int qmax = bm_floordiv((KS - 1) * dil - pad, stride);
    g.PW = WG_BKT + qmax - g.qmin;
    g.W = stride * g.PW;
    g.PX = g.W | 1;
    g.fW = bm_fastdiv((unsigned)g.W);
    g.fsi = bm_fastdiv((unsigned)stride);
    hipStream_t s = (hipStream_t)stream;
    switch (tj) {
        case 1: return launch_wgrad<1>(g, s);
        case 2: return launch_wgrad<2>(g, s);
        case 3: return launch_wgrad<3>(g, s);
        default: return launch_wgrad<4>(g, s);
    }
}
