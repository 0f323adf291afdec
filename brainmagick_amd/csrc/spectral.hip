// optim.svd (bm/svd.py:17-45, bm/solver.py:379-380): the squared largest singular value of every penalised weight, estimated
// as torch.svd_lowrank(p.view(p.shape[0], -1), 16, niters)[1][0] ** 2 does it (torch/_lowrank.py), and its gradient in
// closed form -- for ALL matrices of a model in the same launches.
//
// For a weight A (rows x cols, read in place through a row stride) let At be A when it is tall, else A^T: mt x nt, mt >= nt.
// With q = min(dim, nt) columns of the Gaussian test matrix R and S = 2 niters + 2 stages, M_k = At (k even) / At^T (k odd):
//     X_k = M_k Q_{k-1}   (Q_{-1} = R),     Q_k = X_k L_k^{-T},   L_k L_k^T = X_k^T X_k   (Cholesky of the fp64 Gram matrix)
//     value = largest eigenvalue of X_{S-1}^T X_{S-1}   (X_{S-1}^T = B = Q^T At),  eigenvector u.
// The value depends on range(Q_k) only, so any orthonormalisation gives torch's number -- a column of X_k that adds nothing
// to the range is dropped (sp_chol_inv), so a rank-deficient X_k keeps its range too.  A Gram matrix accumulated in fp32
// loses a decaying spectrum (sigma_16 / sigma_1 = 3e-5 squares to 1e-9): the Gram partials, the factorisation, L^{-1} and
// the product X L^{-T} are fp64; what is stored (X, Q) is fp32.
//
// ONE kernel does every stage, forward and backward: out = op(A) . (Z1 T1 + Z2 T2) over a (row slab of 64, matrix) grid.
// Each workgroup first folds the PREVIOUS launch's per-slab 16 x 16 fp64 partials in slab order and derives the small
// matrices T1 / T2 from them (redundantly: a few hundred fp64 operations), then walks the contraction in chunks of 64:
// the op(A) tile goes through LDS, the 16-wide operand rows are transformed in fp64 on the way into LDS (so Q_k is never a
// pass of its own; the slab-0 workgroup also stores the transformed rows, which the backward needs), the product is
// exact-fp32 MFMA (v_mfma_f32_16x16x4_f32, two accumulators), and the epilogue stores its slab and the slab's fp64 partial
// E^T out.  Stream order is the only synchronisation: no workgroup waits for another, no atomics, fixed fold orders --
// two runs give the same bits, in every compute mode.
//
//   forward  k:  Z1 = X_{k-1} (R for k = 0), T1 = L_{k-1}^{-T};  stores Q_{k-1}, X_k, partial X_k^T X_k
//   top:         Jacobi (fp64, parallel cyclic ordering, SP_SWEEPS sweeps) on the last Gram matrix -> value, u
//   backward 0:  Z1 = X_{S-1}, T1 = 2 u u^T;  stores V = Z1 T1, G_Q = At V, partial Q_K^T G_Q           (K = S - 2)
//   backward k = K..1:  Z1 = G_Q, Z2 = Q_k, T1 = L_k^{-1}, T2 = -(Q_k^T G_Q) L_k^{-1};  stores G_X,k = Z1 T1 + Z2 T2
//                (the projection G_Q - Q_k Q_k^T G_Q, zero in exact arithmetic, and the triangular solve), the next
//                G_Q = M_k^T G_X,k and its partial;  k = 0 stores G_X,0 only
//   dW:          dAt = sum_k U_k V_k^T,  (U_k, V_k) = (G_X,k, Q_{k-1}) for even k, (Q_{k-1}, G_X,k) for odd k, the pair
//                (Q_K, V) of the direct term as k = S - 1: one product of depth 16 S that writes every element once,
//                in A's own layout, scaled by the incoming gradient.
// Every loop is bounded by a constant or a shape: a NaN weight ends in a NaN value, never in a spin.
#include "bm_common.h"

#define SP_Q 16
#define SP_SLAB 64
#define SP_THREADS 256
#define SP_PITCH_N 68              // LDS pitch of an op(A) tile stored [row][k]: conflict-free 16 x 4 fragment reads
#define SP_PITCH_T 80              // ... stored [k][row]
#define SP_SWEEPS 12
#define SP_MAX_NITERS 8

enum { SP_FWD = 0, SP_BWD0 = 1, SP_BWD = 2 };
enum { SP_X = 0, SP_QM = 1, SP_GQ = 2, SP_GX = 3 };         // the four [S][slot] float arrays of a matrix

struct SpMat {
    const float* w;         // A, rows x cols, unit stride inside a row
    long ld;                // floats between rows
    int rows, cols;
    int mt, nt;             // tall orientation
    int wide;               // 1: At = A^T
    int q;                  // min(dim, nt)
    int nslab;              // cdiv(mt, 64): slabs per partial array
    int pad_;
    long r_off;             // first row of this matrix in R_all
    long wsf, wsd;          // offsets into the float / double workspace
    long slot;              // floats per [rows][16] buffer
    long g_off;             // offset of dA in the flat gradient buffer
};

static inline long sp_mtpad(int rows, int cols) { return (long)cdiv(rows > cols ? rows : cols, SP_SLAB) * SP_SLAB; }

extern "C" long bm_spectral_table_entry_bytes(void) { return (long)sizeof(SpMat); }
extern "C" long bm_spectral_ws_floats(int rows, int cols, int niters) {
    return 4L * (2 * niters + 2) * sp_mtpad(rows, cols) * SP_Q;
}
extern "C" long bm_spectral_ws_doubles(int rows, int cols, int niters) {
    const long S = 2 * niters + 2, nslab = sp_mtpad(rows, cols) / SP_SLAB;
    return 2 * S * nslab * 256 + S * 256 + 32;
}

extern "C" int bm_spectral_table_fill(void* entry, const float* w, int rows, int cols, long ld, int dim, long r_off,
                                      long ws_float_off, long ws_double_off, long grad_off) {
    BM_REQUIRE(entry && rows > 0 && cols > 0 && ld >= cols, "spectral: bad matrix %d x %d, row stride %ld", rows, cols, ld);
    BM_REQUIRE(dim >= 1 && dim <= SP_Q, "spectral: dim = %d, the limit is 1..%d", dim, SP_Q);
    BM_REQUIRE((ws_float_off & 15) == 0, "spectral: workspace offset");
    SpMat m;
    m.w = w;
    m.ld = ld;
    m.rows = rows;
    m.cols = cols;
    m.wide = rows < cols;
    m.mt = m.wide ? cols : rows;
    m.nt = m.wide ? rows : cols;
    m.q = dim < m.nt ? dim : m.nt;
    m.nslab = cdiv(m.mt, SP_SLAB);
    m.pad_ = 0;
    m.r_off = r_off;
    m.wsf = ws_float_off;
    m.wsd = ws_double_off;
    m.slot = sp_mtpad(rows, cols) * SP_Q;
    m.g_off = grad_off;
    *(SpMat*)entry = m;
    return BM_OK;
}

__device__ __forceinline__ int sp_slabs(int n) { return (n + SP_SLAB - 1) / SP_SLAB; }
__device__ __forceinline__ float* sp_buf(float* wsf, const SpMat& m, int kind, int k, int S) {
    return wsf + m.wsf + ((long)kind * S + k) * m.slot;
}
// doubles of a matrix: forward partials [S][nslab][256], backward partials [S][nslab][256], L^{-1} [S][256], u[16], value
__device__ __forceinline__ double* sp_part(double* wsd, const SpMat& m, int bwd, int k, int S) {
    return wsd + m.wsd + (((long)bwd * S + k) * m.nslab) * 256;
}
__device__ __forceinline__ double* sp_linv(double* wsd, const SpMat& m, int k, int S) {
    return wsd + m.wsd + 2L * S * m.nslab * 256 + (long)k * 256;
}
__device__ __forceinline__ double* sp_eig(double* wsd, const SpMat& m, int S) {
    return wsd + m.wsd + 2L * S * m.nslab * 256 + (long)S * 256;
}

// Ls: a symmetric 16 x 16 matrix whose leading q x q block is factorised in place (lower L); Li receives L^{-1}, zero
// outside the block.  All SP_THREADS threads call it.
//
// A pivot that carries no information DROPS its column: row and column j of L^{-1} are zero, there is no rank-1 update,
// so Q gets a zero column and range(Q) stays range(X) -- what Householder QR gives torch at a rank-deficient X (a zero or
// duplicated column of a weight with at most 16 of them, a weight of rank below 16, the all-zero weight), where a plain
// Cholesky takes the root of a rounding residue of either sign and ends in NaN.  The pivot d_j is the squared distance of
// column j of X from the span of the columns before it.  X is STORED in fp32: each element carries a relative error of
// up to eps = 2^-24, a column of squared norm g an error of squared norm up to eps^2 g, and the distance sees the errors
// of at most SP_Q columns, none of them longer than dmax = the largest diagonal entry of the Gram matrix.  A pivot of at
// most SP_Q eps^2 dmax (5.7e-14 dmax) is therefore what rounding alone can put there.  What the fixture factors is far
// above it (its worst case, spectrum 0.5^i, has pivots from 1e-9 dmax).  The comparison is false for a NaN pivot: a NaN
// weight still ends in a NaN value.
#define SP_PIVOT_FLOOR (16.0 * 0x1p-48)             // SP_Q eps^2
__device__ __forceinline__ void sp_chol_inv(double* Ls, double* Li, int q) {
    const int t = threadIdx.x, i = t >> 4, c = t & 15;
    __syncthreads();
    double dmax = 0.0;
    for (int j = 0; j < q; ++j) {
        const double g = Ls[j * 16 + j];
        if (g > dmax) dmax = g;
    }
    unsigned dropped = 0;                           // uniform: every thread sees the same pivots
    for (int j = 0; j < q; ++j) {
        __syncthreads();
        const double d = Ls[j * 16 + j], lij = Ls[i * 16 + j], lcj = Ls[c * 16 + j];
        __syncthreads();
        const bool drop = d <= SP_PIVOT_FLOOR * dmax;
        if (drop) dropped |= 1u << j;
        if (i < q && c < q) {
            if (c == j) {
                if (i >= j) Ls[i * 16 + j] = drop ? (i == j ? 1.0 : 0.0) : (i == j ? sqrt(d) : lij / sqrt(d));
            } else if (c > j && i >= c && !drop) {
                Ls[i * 16 + c] -= lij * lcj / d;
            }
        }
    }
    Li[t] = 0.0;
    __syncthreads();
    if (t < q && !(dropped >> t & 1)) {             // column t of L^{-1} by forward substitution
        double x[SP_Q];
#pragma unroll
        for (int r = 0; r < SP_Q; ++r) {
            x[r] = 0.0;
            if (r < q) {
                double s = r == t ? 1.0 : 0.0;
#pragma unroll
                for (int j = 0; j < r; ++j) s -= Ls[r * 16 + j] * x[j];
                x[r] = r >= t && !(dropped >> r & 1) ? s / Ls[r * 16 + r] : 0.0;
                Li[r * 16 + t] = x[r];
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ double sp_fold(const double* part, int nslab) {
    double s = 0.0;
    for (int i = 0; i < nslab; ++i) s += part[(long)i * 256 + threadIdx.x];
    return s;
}

// 16 floats of row `r` of a 16-wide operand: 16-byte loads from the workspace buffers (pitch 16), scalar loads of the
// first `zcols` columns from R (pitch dim).
__device__ __forceinline__ void sp_load_row(float* z, const float* Z, long r, int zld, int zcols, bool valid) {
    if (!valid) {
#pragma unroll
        for (int a = 0; a < SP_Q; ++a) z[a] = 0.f;
    } else if (zld == SP_Q && zcols == SP_Q) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const f32x4 x = *(const f32x4*)(Z + r * SP_Q + 4 * v);
#pragma unroll
            for (int e = 0; e < 4; ++e) z[4 * v + e] = x[e];
        }
    } else {
#pragma unroll
        for (int a = 0; a < SP_Q; ++a) z[a] = a < zcols ? Z[r * zld + a] : 0.f;
    }
}

__global__ __launch_bounds__(SP_THREADS) void spectral_stage_kernel(const SpMat* __restrict__ table,
                                                                    const float* __restrict__ R, int dim, float* wsf,
                                                                    double* wsd, int mode, int k, int S) {
    __shared__ __attribute__((aligned(16))) float As[SP_SLAB * SP_PITCH_T];
    __shared__ __attribute__((aligned(16))) float Qs[SP_SLAB * SP_Q];
    __shared__ __attribute__((aligned(16))) float Os[SP_SLAB * SP_Q];
    __shared__ __attribute__((aligned(16))) float Es[SP_SLAB * SP_Q];
    __shared__ double T1s[256], T2s[256], Ws[256], Cs[256];
    const SpMat m = table[blockIdx.y];
    const int slab = blockIdx.x, t = threadIdx.x, ti = t >> 4, tc = t & 15;
    // M_j = At (j even) or At^T (j odd), At = A or A^T:  op(A) = A^T when (j & 1) ^ wide
    const int odd = k & 1;
    int trans, orows, kdim;
    bool do_prod = true;
    if (mode == SP_FWD) {
        trans = odd ^ m.wide;
        orows = odd ? m.nt : m.mt;
        kdim = odd ? m.mt : m.nt;
    } else if (mode == SP_BWD0) {
        trans = m.wide;
        orows = m.mt;
        kdim = m.nt;
    } else {                                        // M_k^T
        trans = !(odd ^ m.wide);
        orows = odd ? m.mt : m.nt;
        kdim = odd ? m.nt : m.mt;
        do_prod = k > 0;
    }
    if (slab >= (do_prod ? sp_slabs(orows) : 1)) return;

    const float *Z1, *Z2 = nullptr, *E = nullptr;
    float *bout, *out;
    double* pout;
    int zld = SP_Q, zcols = SP_Q;
    T2s[t] = 0.0;
    if (mode == SP_FWD) {
        if (k == 0) {
            Z1 = R + m.r_off * dim;
            zld = dim;
            zcols = m.q;
            T1s[t] = ti == tc ? 1.0 : 0.0;
        } else {
            Z1 = sp_buf(wsf, m, SP_X, k - 1, S);
            Ws[t] = sp_fold(sp_part(wsd, m, 0, k - 1, S), sp_slabs(kdim));
            sp_chol_inv(Ws, Cs, m.q);
            T1s[t] = Cs[tc * 16 + ti];                      // L^{-T}
            if (slab == 0) sp_linv(wsd, m, k - 1, S)[t] = Cs[t];
        }
        bout = sp_buf(wsf, m, SP_QM, k, S);
        out = sp_buf(wsf, m, SP_X, k, S);
        pout = sp_part(wsd, m, 0, k, S);
    } else if (mode == SP_BWD0) {
        const double* u = sp_eig(wsd, m, S);
        Z1 = sp_buf(wsf, m, SP_X, S - 1, S);
        T1s[t] = 2.0 * u[ti] * u[tc];
        bout = sp_buf(wsf, m, SP_GX, S - 1, S);
        out = sp_buf(wsf, m, SP_GQ, S - 2, S);
        E = sp_buf(wsf, m, SP_QM, S - 1, S);
        pout = sp_part(wsd, m, 1, S - 2, S);
    } else {
        Z1 = sp_buf(wsf, m, SP_GQ, k, S);
        Z2 = sp_buf(wsf, m, SP_QM, k + 1, S);
        Ws[t] = sp_linv(wsd, m, k, S)[t];
        Cs[t] = sp_fold(sp_part(wsd, m, 1, k, S), sp_slabs(kdim));
        __syncthreads();
        T1s[t] = Ws[t];
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < SP_Q; ++b) s -= Cs[ti * 16 + b] * Ws[b * 16 + tc];
        T2s[t] = s;
        bout = sp_buf(wsf, m, SP_GX, k, S);
        out = do_prod ? sp_buf(wsf, m, SP_GQ, k - 1, S) : nullptr;
        E = sp_buf(wsf, m, SP_QM, k, S);
        pout = do_prod ? sp_part(wsd, m, 1, k - 1, S) : nullptr;
    }
    __syncthreads();

    const int wave = t >> 6, lane = t & 63, row0 = slab * SP_SLAB;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const int nchunks = (kdim + SP_SLAB - 1) / SP_SLAB;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int k0 = ch * SP_SLAB;
        __syncthreads();                                    // the previous chunk's fragments have been read
        if (do_prod) {
#pragma unroll 4
            for (int u = 0; u < 16; ++u) {
                const int fast = t & 63, slow = (t >> 6) + 4 * u;
                if (!trans) {                               // A[row0 + slow][k0 + fast]
                    const int r = row0 + slow, c = k0 + fast;
                    As[slow * SP_PITCH_N + fast] = r < orows && c < kdim ? m.w[(long)r * m.ld + c] : 0.f;
                } else {                                    // A[k0 + slow][row0 + fast]
                    const int r = k0 + slow, c = row0 + fast;
                    As[slow * SP_PITCH_T + fast] = r < kdim && c < orows ? m.w[(long)r * m.ld + c] : 0.f;
                }
            }
        }
        {
            const int zr = t >> 2, cg = (t & 3) * 4;
            const long gr = k0 + zr;
            const bool valid = gr < kdim;
            float z[SP_Q];
            double o[4] = {0.0, 0.0, 0.0, 0.0};
            sp_load_row(z, Z1, gr, zld, zcols, valid);
#pragma unroll
            for (int a = 0; a < SP_Q; ++a)
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fma((double)z[a], T1s[a * 16 + cg + j], o[j]);
            if (Z2) {                                       // uniform
                sp_load_row(z, Z2, gr, SP_Q, SP_Q, valid);
#pragma unroll
                for (int a = 0; a < SP_Q; ++a)
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = fma((double)z[a], T2s[a * 16 + cg + j], o[j]);
            }
            const f32x4 qv = {(float)o[0], (float)o[1], (float)o[2], (float)o[3]};
            *(f32x4*)(Qs + zr * SP_Q + cg) = qv;
            if (slab == 0 && valid) *(f32x4*)(bout + gr * SP_Q + cg) = qv;
        }
        __syncthreads();
        if (do_prod) {
            const int fm = wave * 16 + (lane & 15), fk = lane >> 4;
#pragma unroll
            for (int s = 0; s < 16; s += 2) {
                const float a0 = trans ? As[(s * 4 + fk) * SP_PITCH_T + fm] : As[fm * SP_PITCH_N + s * 4 + fk];
                const float a1 = trans ? As[(s * 4 + 4 + fk) * SP_PITCH_T + fm] : As[fm * SP_PITCH_N + s * 4 + 4 + fk];
                const float b0 = Qs[(s * 4 + fk) * SP_Q + (lane & 15)];
                const float b1 = Qs[(s * 4 + 4 + fk) * SP_Q + (lane & 15)];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc1, 0, 0, 0);
            }
        }
    }
    if (!do_prod) return;
    // epilogue: this slab of `out`, and the slab's fp64 partial E^T out (E = out in the forward: the Gram matrix)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int rl = wave * 16 + (lane >> 4) * 4 + j, col = lane & 15;
        const float v = acc0[j] + acc1[j];
        Os[rl * SP_Q + col] = v;
        if (row0 + rl < orows) out[(long)(row0 + rl) * SP_Q + col] = v;
    }
    if (E) {
        const int er = t >> 2, cg = (t & 3) * 4;
        f32x4 e = {0.f, 0.f, 0.f, 0.f};
        if (row0 + er < orows) e = *(const f32x4*)(E + (long)(row0 + er) * SP_Q + cg);
        *(f32x4*)(Es + er * SP_Q + cg) = e;
    }
    __syncthreads();
    const float* Ep = E ? Es : Os;
    double s = 0.0;
#pragma unroll 8
    for (int r = 0; r < SP_SLAB; ++r) s = fma((double)Ep[r * SP_Q + ti], (double)Os[r * SP_Q + tc], s);
    pout[(long)slab * 256 + t] = s;
}

// The largest eigenvalue and its eigenvector of the last Gram matrix: one wavefront per matrix, cyclic Jacobi in fp64 in
// the round-robin ordering (15 rounds of 8 disjoint rotations make a sweep), a fixed number of sweeps.
__global__ __launch_bounds__(64) void spectral_top_kernel(const SpMat* __restrict__ table, double* wsd, float* values,
                                                          int S) {
    __shared__ double Gs[256], Vs[256], cs[16];
    __shared__ int pq[16];
    const SpMat m = table[blockIdx.x];
    const int lane = threadIdx.x;
    const double* part = sp_part(wsd, m, 0, S - 1, S);
    const int nsl = (m.nt + SP_SLAB - 1) / SP_SLAB;
    for (int e = lane; e < 256; e += 64) {
        double s = 0.0;
        for (int i = 0; i < nsl; ++i) s += part[(long)i * 256 + e];
        Gs[e] = s;
        Vs[e] = (e >> 4) == (e & 15) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < SP_SWEEPS; ++sweep) {
        for (int r = 0; r < 15; ++r) {
            __syncthreads();
            if (lane < 8) {
                const int p = lane == 0 ? 15 : (r + lane) % 15, q = lane == 0 ? r : (r + 15 - lane) % 15;
                const double app = Gs[p * 16 + p], aqq = Gs[q * 16 + q], apq = Gs[p * 16 + q];
                double c = 1.0, s = 0.0;
                if (apq != 0.0) {
                    const double tau = (aqq - app) / (2.0 * apq);
                    const double tt = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + tt * tt);
                    s = tt * c;
                }
                cs[2 * lane] = c;
                cs[2 * lane + 1] = s;
                pq[2 * lane] = p;
                pq[2 * lane + 1] = q;
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < 2; ++it) {                // columns of G and V
                const int item = lane + 64 * it, i = item & 15, g = item >> 4, p = pq[2 * g], q = pq[2 * g + 1];
                const double c = cs[2 * g], s = cs[2 * g + 1];
                const double gp = Gs[i * 16 + p], gq = Gs[i * 16 + q], vp = Vs[i * 16 + p], vq = Vs[i * 16 + q];
                Gs[i * 16 + p] = c * gp - s * gq;
                Gs[i * 16 + q] = s * gp + c * gq;
                Vs[i * 16 + p] = c * vp - s * vq;
                Vs[i * 16 + q] = s * vp + c * vq;
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < 2; ++it) {                // rows of G
                const int item = lane + 64 * it, j = item & 15, g = item >> 4, p = pq[2 * g], q = pq[2 * g + 1];
                const double c = cs[2 * g], s = cs[2 * g + 1];
                const double gp = Gs[p * 16 + j], gq = Gs[q * 16 + j];
                Gs[p * 16 + j] = c * gp - s * gq;
                Gs[q * 16 + j] = s * gp + c * gq;
            }
        }
    }
    __syncthreads();
    int best = 0;
    double lam = Gs[0];
    bool bad = lam != lam;
    for (int i = 1; i < SP_Q; ++i) {
        const double d = Gs[i * 16 + i];
        bad = bad || d != d;
        if (d > lam) {
            lam = d;
            best = i;
        }
    }
    if (bad) lam = __builtin_nan("");                       // a NaN anywhere on the diagonal is a NaN value
    double* eig = sp_eig(wsd, m, S);
    if (lane < SP_Q) eig[lane] = Vs[lane * 16 + best];
    if (lane == 0) {
        eig[16] = lam;
        values[blockIdx.x] = (float)lam;
    }
}

__global__ __launch_bounds__(64) void spectral_sum_kernel(const SpMat* __restrict__ table, const double* wsd, int nmat,
                                                          int S, float* total) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < nmat; ++i) {
        const SpMat m = table[i];
        s += (wsd + m.wsd + 2L * S * m.nslab * 256 + (long)S * 256)[16];
    }
    *total = (float)s;
}

// dA = gscale * sum_k P_k C_k^T in A's layout, a 64 x 64 tile per workgroup (a wavefront: 16 rows x 64 columns).
__global__ __launch_bounds__(SP_THREADS) void spectral_dw_kernel(const SpMat* __restrict__ table, float* wsf,
                                                                 const float* __restrict__ gscale, float* grads, int S) {
    const SpMat m = table[blockIdx.y];
    const int ntc = (m.cols + 63) / 64, ntr = (m.rows + 63) / 64;
    if ((int)blockIdx.x >= ntc * ntr) return;
    const int tr = blockIdx.x / ntc, tcol = blockIdx.x - tr * ntc;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, fk = lane >> 4, fl = lane & 15;
    const int i = tr * 64 + wave * 16 + fl;                 // row of the A-operand fragment
    const int j0 = tcol * 64;
    f32x4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < S; ++k) {
        // rows of dAt come from U_k, columns from V_k; a wide A is dAt^T: the roles swap
        const bool rows_from_qm = ((k & 1) ^ m.wide) != 0;
        const float* P = sp_buf(wsf, m, rows_from_qm ? SP_QM : SP_GX, k, S);
        const float* C = sp_buf(wsf, m, rows_from_qm ? SP_GX : SP_QM, k, S);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float a = i < m.rows ? P[(long)i * SP_Q + s * 4 + fk] : 0.f;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int j = j0 + n * 16 + fl;
                const float b = j < m.cols ? C[(long)j * SP_Q + s * 4 + fk] : 0.f;
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[n], 0, 0, 0);
            }
        }
    }
    const float gs = *gscale;
    float* dA = grads + m.g_off;
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int r = tr * 64 + wave * 16 + fk * 4 + jj, c = j0 + n * 16 + fl;
            if (r < m.rows && c < m.cols) dA[(long)r * m.cols + c] = gs * acc[n][jj];
        }
}

static int sp_check(const void* table, int nmat, int max_slabs, int niters, const void* wsf, const void* wsd) {
    BM_REQUIRE(nmat >= 0 && nmat <= 65535, "spectral: %d matrices, the limit of one launch is 65535", nmat);
    BM_REQUIRE(niters >= 0 && niters <= SP_MAX_NITERS, "spectral: niters = %d, the limit is 0..%d", niters, SP_MAX_NITERS);
    BM_REQUIRE(nmat == 0 || (table && wsf && wsd && max_slabs > 0), "spectral: null pointer");
    return BM_OK;
}

extern "C" int bm_spectral_fwd(const void* table, int nmat, int max_slabs, const float* R, int dim, int niters,
                               float* ws_floats, double* ws_doubles, float* values, float* total, void* stream) {
    if (int e = sp_check(table, nmat, max_slabs, niters, ws_floats, ws_doubles)) return e;
    BM_REQUIRE(dim >= 1 && dim <= SP_Q, "spectral: dim = %d, the limit is 1..%d", dim, SP_Q);
    BM_REQUIRE(nmat == 0 || (R && values && total), "spectral: null pointer");
    if (nmat == 0) return BM_OK;
    hipStream_t s = (hipStream_t)stream;
    const SpMat* tb = (const SpMat*)table;
    const int S = 2 * niters + 2;
    for (int k = 0; k < S; ++k)
        hipLaunchKernelGGL(spectral_stage_kernel, dim3(max_slabs, nmat), dim3(SP_THREADS), 0, s, tb, R, dim, ws_floats,
                           ws_doubles, (int)SP_FWD, k, S);
    hipLaunchKernelGGL(spectral_top_kernel, dim3(nmat), dim3(64), 0, s, tb, ws_doubles, values, S);
    hipLaunchKernelGGL(spectral_sum_kernel, dim3(1), dim3(64), 0, s, tb, (const double*)ws_doubles, nmat, S, total);
    return bm_check_launch("spectral_fwd");
}

extern "C" int bm_spectral_bwd(const void* table, int nmat, int max_slabs, int max_tiles, int niters, float* ws_floats,
                               double* ws_doubles, const float* gscale, float* grads, void* stream) {
    if (int e = sp_check(table, nmat, max_slabs, niters, ws_floats, ws_doubles)) return e;
    BM_REQUIRE(nmat == 0 || (gscale && grads && max_tiles > 0), "spectral: null pointer");
    if (nmat == 0) return BM_OK;
    hipStream_t s = (hipStream_t)stream;
    const SpMat* tb = (const SpMat*)table;
    const int S = 2 * niters + 2;
    hipLaunchKernelGGL(spectral_stage_kernel, dim3(max_slabs, nmat), dim3(SP_THREADS), 0, s, tb, (const float*)nullptr, 0,
                       ws_floats, ws_doubles, (int)SP_BWD0, 0, S);
    for (int k = S - 2; k >= 0; --k)
        hipLaunchKernelGGL(spectral_stage_kernel, dim3(k > 0 ? max_slabs : 1, nmat), dim3(SP_THREADS), 0, s, tb,
                           (const float*)nullptr, 0, ws_floats, ws_doubles, (int)SP_BWD, k, S);
    hipLaunchKernelGGL(spectral_dw_kernel, dim3(max_tiles, nmat), dim3(SP_THREADS), 0, s, tb, ws_floats, gscale, grads, S);
    return bm_check_launch("spectral_bwd");
}
