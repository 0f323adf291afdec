// LSTM recurrence (nn.LSTM inside bm/models/convrnn.py:25-29): the cell step, forward and backward, on exact-fp32
// MFMA (v_mfma_f32_32x32x2_f32) in every compute mode.  Activations are time-major inside the stack, [T][C][B] with
// the batch contiguous, so one time step h_t is an [H][B] matrix -- a "segment" of the library's [segment][channel]
// [time] layout -- and everything that is not the recurrence (the input projection W_ih X + b over all steps, dX, dW_ih,
// dW_hh, the bias gradients) runs on the existing conv / gemm_nt / channel-sum kernels.
//
//   forward step   G_t = W_hh[4H][H] h_{t-1}[H][B] + Gx_t       gates i, f, g, o (PyTorch's order)
//                  c_t = s(f) c_{t-1} + s(i) tanh(g),  h_t = s(o) tanh(c_t)
//   backward step  dh_t = dY_t + W_hh^T[H][4H] dG_{t+1}[4H][B];  dc_t, the four gate gradients dG_t
//
// ONE LAUNCH PER TIME STEP, on purpose: stream order is the only synchronisation between steps.  There is no
// persistent or cooperative kernel, no flag that one workgroup sets and another polls -- a recurrence that waits for a
// step that never arrives would hang a device other people share, and ~100 launches per layer and pass are cheap next
// to that.  The host entry points enqueue all T launches of a (layer, pass); both directions of a bidirectional layer
// share a launch through gridDim.z (the reverse direction walks t downwards with the same code).
//
// Tiling: a workgroup (4 wavefronts) owns 32 hidden units x 32 batch columns of one direction -- forward: the four gate
// rows j, H+j, 2H+j, 3H+j of its units, so the cell update runs in the epilogue on the workgroup's own accumulators
// and the [4H][B] pre-activation never reaches memory.  The reduction (H forward, 4H backward) is split four ways
// across the wavefronts of the workgroup: each runs a quarter of every staged chunk, the partial accumulators are
// folded through LDS in a fixed order (deterministic, no atomics), and each wavefront finishes a quarter of the rows.
// Operands are read from nn.LSTM's own weight_hh [4H][H] (no packed copy): coalesced global loads with bounds checks
// (any H, B: zero fill) into registers one chunk ahead, then LDS.  Sigmoid and tanh are the accurate library
// functions (expf, tanhf, IEEE division).
#include "bm_common.h"

#define LSTM_KC 64      // forward: reduction chunk (16 per wavefront)
#define LSTM_KCB 128    // backward: reduction chunk (32 per wavefront)
#define LSTM_PA 65      // forward A tile row pitch (row-per-lane reads without bank conflicts)

struct LstmFwdArgs {
    const float* whh0; const float* whh1;      // [4H][H] per direction
    const float* gx0; const float* gx1;        // [T][4H][B]: W_ih x_t + b_ih + b_hh
    float* y;                                   // [T][H * dirs][B]: h_t at channel offset dir * H
    float* gates0; float* gates1;               // [T][4H][B]: activated i, f, g, o (saved for the backward pass)
    float* c0; float* c1;                       // [T][H][B]
    int H, B, T, dirs, step;
};

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(256) void lstm_step_fwd_kernel(LstmFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[4 * 4 * 16 * 64];      // 64 KB: staging, then the partial sums
    float* As = smem;                            // [128 = gate * 32 + unit][LSTM_PA]
    float* Bs = smem + 128 * LSTM_PA;            // [LSTM_KC][32]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nl = lane & 31;
    const int h = lane >> 5;
    const int j0 = blockIdx.x * 32;
    const int b0 = blockIdx.y * 32;
    const int d = blockIdx.z;
    const int H = a.H, B = a.B;
    const int t = d ? a.T - 1 - a.step : a.step;
    const int tp = d ? t + 1 : t - 1;            // the step before, in this direction's order
    const bool has_prev = a.step > 0;
    const float* whh = d ? a.whh1 : a.whh0;
    const float* gx = (d ? a.gx1 : a.gx0) + (long)t * 4 * H * B;
    float* gates = (d ? a.gates1 : a.gates0) + (long)t * 4 * H * B;
    float* ct = (d ? a.c1 : a.c0) + (long)t * H * B;
    const float* cp = (d ? a.c1 : a.c0) + (long)tp * H * B;
    const long ypitch = (long)H * a.dirs * B;
    const float* hp = a.y + tp * ypitch + (long)d * H * B;
    float* ht = a.y + t * ypitch + (long)d * H * B;

    f32x16 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;

    if (has_prev) {                              // h_{-1} = 0: the first step is the epilogue alone
        float ar[32], br[8];
        const int akc = tid & 63, ar0 = tid >> 6;        // A: column of the chunk, first of 32 rows (4 apart)
        const int bcol = tid & 31, bk0 = tid >> 5;       // B: column, first of 8 rows (8 apart)
        const int nchunk = (H + LSTM_KC - 1) / LSTM_KC;
#define LSTM_LOAD(K0_)                                                                            \
    {                                                                                             \
        const int k = (K0_) + akc;                                                                \
        _Pragma("unroll") for (int i = 0; i < 32; ++i) {                                          \
            const int r = ar0 + 4 * i;                                                            \
            const int j = j0 + (r & 31);                                                          \
            ar[i] = (j < H && k < H) ? whh[((long)(r >> 5) * H + j) * H + k] : 0.f;               \
        }                                                                                         \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                           \
            const int kb = (K0_) + bk0 + 8 * i;                                                   \
            br[i] = (kb < H && b0 + bcol < B) ? hp[(long)kb * B + b0 + bcol] : 0.f;               \
        }                                                                                         \
    }
        LSTM_LOAD(0);
        for (int c = 0; c < nchunk; ++c) {
#pragma unroll
            for (int i = 0; i < 32; ++i) As[(ar0 + 4 * i) * LSTM_PA + akc] = ar[i];
#pragma unroll
            for (int i = 0; i < 8; ++i) Bs[(bk0 + 8 * i) * 32 + bcol] = br[i];
            __syncthreads();
            if (c + 1 < nchunk) LSTM_LOAD((c + 1) * LSTM_KC);      // in flight during the MFMAs below
            const float* ap = As + nl * LSTM_PA + wave * 16 + h;
            const float* bp = Bs + (wave * 16 + h) * 32 + nl;
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
                const float bv = bp[2 * kk * 32];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float av = ap[g * 32 * LSTM_PA + 2 * kk];
                    acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[g], 0, 0, 0);
                }
            }
            __syncthreads();
        }
#undef LSTM_LOAD
    }

    // ---- fold the four partial sums, then the cell update: wavefront w finishes registers 4w .. 4w+3 ----
    float* red = smem;                           // [wave][gate][16][64]
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[((wave * 4 + g) * 16 + r) * 64 + lane] = acc[g][r];
    __syncthreads();
    const int b = b0 + nl;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = 4 * wave + q;
        const int j = j0 + q + 8 * wave + 4 * h;         // accumulator register r holds row (r & 3) + 8 (r >> 2) + 4 h
        if (j < H && b < B) {
            float pre[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float s = red[((0 * 4 + g) * 16 + r) * 64 + lane];
                s += red[((1 * 4 + g) * 16 + r) * 64 + lane];
                s += red[((2 * 4 + g) * 16 + r) * 64 + lane];
                s += red[((3 * 4 + g) * 16 + r) * 64 + lane];
                pre[g] = s + gx[((long)g * H + j) * B + b];
            }
            const float ig = lstm_sigmoid(pre[0]);
            const float fg = lstm_sigmoid(pre[1]);
            const float gg = tanhf(pre[2]);
            const float og = lstm_sigmoid(pre[3]);
            const float cprev = has_prev ? cp[(long)j * B + b] : 0.f;
            const float cn = fg * cprev + ig * gg;
            gates[((long)0 * H + j) * B + b] = ig;
            gates[((long)1 * H + j) * B + b] = fg;
            gates[((long)2 * H + j) * B + b] = gg;
            gates[((long)3 * H + j) * B + b] = og;
            ct[(long)j * B + b] = cn;
            ht[(long)j * B + b] = og * tanhf(cn);
        }
    }
}

struct LstmBwdArgs {
    const float* whh0; const float* whh1;      // [4H][H]
    const float* dy;                            // [T][H * dirs][B]
    const float* gates0; const float* gates1;   // [T][4H][B]
    const float* c0; const float* c1;           // [T][H][B]
    float* dg0; float* dg1;                     // [T][4H][B]: gradient of the gate pre-activations
    float* dc0; float* dc1;                     // [H][B]: dL/dc carried from step to step (in: dL/dc_n)
    int H, B, T, dirs, step;
};

__global__ __launch_bounds__(256) void lstm_step_bwd_kernel(LstmBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[2 * LSTM_KCB * 32];     // 32 KB: staging, then the partial sums
    float* As = smem;                            // [LSTM_KCB][32]: W_hh[k][j0 + m]
    float* Bs = smem + LSTM_KCB * 32;            // [LSTM_KCB][32]: dG_{next}[k][b0 + n]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nl = lane & 31;
    const int h = lane >> 5;
    const int j0 = blockIdx.x * 32;
    const int b0 = blockIdx.y * 32;
    const int d = blockIdx.z;
    const int H = a.H, B = a.B;
    const int fs = a.T - 1 - a.step;             // index of the forward step this launch differentiates
    const int t = d ? a.T - 1 - fs : fs;
    const int tn = d ? t - 1 : t + 1;            // the forward step after it (its dG is this step's operand)
    const int tp = d ? t + 1 : t - 1;            // the forward step before it (c_{t-1})
    const bool has_next = a.step > 0;
    const bool has_prev = fs > 0;
    const float* whh = d ? a.whh1 : a.whh0;
    const float* gates = (d ? a.gates1 : a.gates0) + (long)t * 4 * H * B;
    const float* ct = (d ? a.c1 : a.c0) + (long)t * H * B;
    const float* cp = (d ? a.c1 : a.c0) + (long)tp * H * B;
    float* dgt = (d ? a.dg1 : a.dg0) + (long)t * 4 * H * B;
    const float* dgn = (d ? a.dg1 : a.dg0) + (long)tn * 4 * H * B;
    float* dc = d ? a.dc1 : a.dc0;
    const float* dyt = a.dy + (long)t * H * a.dirs * B + (long)d * H * B;
    const int K = 4 * H;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    if (has_next) {
        float ar[16], br[16];
        const int col = tid & 31, k0t = tid >> 5;        // column, first of 16 rows (8 apart), both operands
        const int nchunk = (K + LSTM_KCB - 1) / LSTM_KCB;
#define LSTM_LOAD(K0_)                                                                            \
    {                                                                                             \
        _Pragma("unroll") for (int i = 0; i < 16; ++i) {                                          \
            const int k = (K0_) + k0t + 8 * i;                                                    \
            ar[i] = (k < K && j0 + col < H) ? whh[(long)k * H + j0 + col] : 0.f;                  \
            br[i] = (k < K && b0 + col < B) ? dgn[(long)k * B + b0 + col] : 0.f;                  \
        }                                                                                         \
    }
        LSTM_LOAD(0);
        for (int c = 0; c < nchunk; ++c) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                As[(k0t + 8 * i) * 32 + col] = ar[i];
                Bs[(k0t + 8 * i) * 32 + col] = br[i];
            }
            __syncthreads();
            if (c + 1 < nchunk) LSTM_LOAD((c + 1) * LSTM_KCB);
            const float* ap = As + (wave * 32 + h) * 32 + nl;
            const float* bp = Bs + (wave * 32 + h) * 32 + nl;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * kk * 32], bp[2 * kk * 32], acc, 0, 0, 0);
            __syncthreads();
        }
#undef LSTM_LOAD
    }

    float* red = smem;                           // [wave][16][64]
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();
    const int b = b0 + nl;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = 4 * wave + q;
        const int j = j0 + q + 8 * wave + 4 * h;
        if (j < H && b < B) {
            float s = red[(0 * 16 + r) * 64 + lane];
            s += red[(1 * 16 + r) * 64 + lane];
            s += red[(2 * 16 + r) * 64 + lane];
            s += red[(3 * 16 + r) * 64 + lane];
            const long e = (long)j * B + b;
            const float dh = s + dyt[e];
            const float ig = gates[((long)0 * H + j) * B + b];
            const float fg = gates[((long)1 * H + j) * B + b];
            const float gg = gates[((long)2 * H + j) * B + b];
            const float og = gates[((long)3 * H + j) * B + b];
            const float tc = tanhf(ct[e]);
            const float cprev = has_prev ? cp[e] : 0.f;
            const float dct = dc[e] + dh * og * (1.0f - tc * tc);
            dgt[((long)0 * H + j) * B + b] = dct * gg * ig * (1.0f - ig);
            dgt[((long)1 * H + j) * B + b] = dct * cprev * fg * (1.0f - fg);
            dgt[((long)2 * H + j) * B + b] = dct * ig * (1.0f - gg * gg);
            dgt[((long)3 * H + j) * B + b] = dh * tc * og * (1.0f - og);
            dc[e] = dct * fg;
        }
    }
}

static int lstm_check_dims(const char* what, int H, int B, int T, int dirs) {
    BM_REQUIRE(H > 0 && B > 0 && T > 0, "%s: bad dims H=%d B=%d T=%d", what, H, B, T);
    BM_REQUIRE(dirs == 1 || dirs == 2, "%s: dirs must be 1 or 2, got %d", what, dirs);
    BM_REQUIRE((long)T * 4 * H * B < (1L << 40) && (long)4 * H * H < (1L << 31) && (long)4 * H * B < (1L << 31),
               "%s: tensor too large", what);
    BM_REQUIRE(cdiv(B, 32) <= 65535, "%s: batch of %d columns exceeds the grid", what, B);
    return BM_OK;
}

// C-ABI: the recurrence of one nn.LSTM layer, all T steps (bm/models/convrnn.py:35), both directions when dirs = 2.
// gx_d = W_ih x + b_ih + b_hh for every step [T][4H][B]; y [T][H * dirs][B] receives h_t at channel offset d * H;
// gates_d [T][4H][B] (activated i, f, g, o) and c_d [T][H][B] are saved for bm_lstm_layer_bwd.  h_{-1} = c_{-1} = 0.
// The *1 pointers are ignored when dirs = 1.
extern "C" int bm_lstm_layer_fwd(const float* whh0, const float* whh1, const float* gx0, const float* gx1, float* y,
                                 float* gates0, float* gates1, float* c0, float* c1, int H, int B, int T, int dirs,
                                 void* stream) {
    if (int e = lstm_check_dims("lstm_layer_fwd", H, B, T, dirs)) return e;
    BM_REQUIRE(whh0 && gx0 && y && gates0 && c0, "lstm_layer_fwd: null pointer");
    BM_REQUIRE(dirs == 1 || (whh1 && gx1 && gates1 && c1), "lstm_layer_fwd: null pointer (reverse direction)");
    LstmFwdArgs a;
    a.whh0 = whh0; a.whh1 = whh1; a.gx0 = gx0; a.gx1 = gx1; a.y = y; a.gates0 = gates0; a.gates1 = gates1;
    a.c0 = c0; a.c1 = c1; a.H = H; a.B = B; a.T = T; a.dirs = dirs;
    const dim3 grid((unsigned)cdiv(H, 32), (unsigned)cdiv(B, 32), (unsigned)dirs);
    for (int s = 0; s < T; ++s) {
        a.step = s;
        hipLaunchKernelGGL(lstm_step_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    }
    return bm_check_launch("lstm_step_fwd");
}

// C-ABI: autograd of bm_lstm_layer_fwd (bm/models/convrnn.py:35 backward).  dy [T][H * dirs][B] is dL/dy with dL/dh_n
// already added at each direction's last step; dc_d [H][B] holds dL/dc_n on entry and is the carried dL/dc (overwritten).
// Writes dg_d [T][4H][B], the gradient of the gate pre-activations -- the operand of dX, dW_ih, dW_hh and the bias sums.
extern "C" int bm_lstm_layer_bwd(const float* whh0, const float* whh1, const float* dy, const float* gates0,
                                 const float* gates1, const float* c0, const float* c1, float* dg0, float* dg1,
                                 float* dc0, float* dc1, int H, int B, int T, int dirs, void* stream) {
    if (int e = lstm_check_dims("lstm_layer_bwd", H, B, T, dirs)) return e;
    BM_REQUIRE(whh0 && dy && gates0 && c0 && dg0 && dc0, "lstm_layer_bwd: null pointer");
    BM_REQUIRE(dirs == 1 || (whh1 && gates1 && c1 && dg1 && dc1), "lstm_layer_bwd: null pointer (reverse direction)");
    LstmBwdArgs a;
    a.whh0 = whh0; a.whh1 = whh1; a.dy = dy; a.gates0 = gates0; a.gates1 = gates1; a.c0 = c0; a.c1 = c1;
    a.dg0 = dg0; a.dg1 = dg1; a.dc0 = dc0; a.dc1 = dc1; a.H = H; a.B = B; a.T = T; a.dirs = dirs;
    const dim3 grid((unsigned)cdiv(H, 32), (unsigned)cdiv(B, 32), (unsigned)dirs);
    for (int s = 0; s < T; ++s) {
        a.step = s;
        hipLaunchKernelGGL(lstm_step_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    }
    return bm_check_launch("lstm_step_bwd");
}
