/* libbmhip -- C-ABI of the MI355X (gfx950) SimpleConv + ClipLoss training hot path.
 *
 * The reference (facebookresearch/brainmagick) is 100 % Python: its "FFI" for this path is the set
 * of PyTorch ops its modules call.  Each entry point below replaces the ATen kernels behind one such
 * call site (cited as bm/<file>:<line>, relative to the reference root).  The reference-side binding
 * is the ctypes table in brainmagick_amd/_lib.py.
 *
 * Conventions
 *   - every function returns int: 0 = ok, otherwise a hipError_t or a BM_ERR_* code; the message is
 *     available (thread-local) from bm_last_error().  Nothing aborts or throws across the ABI.
 *   - all tensors are fp32, contiguous, [B][channels][T] with T fastest, living in device memory
 *     owned by the caller.  Indices are int32 (widx, order, seg) or int64 (idx of group_by_index).
 *   - every fp32 pointer needs 4-byte alignment only; the 16-byte paths are taken where the pointers allow.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); kernels are
 *     only enqueued, never synchronised.  The library allocates nothing; scratch is caller-provided.
 *   - deterministic: every reduction has a fixed order (split-K partials are folded in order).
 */
#ifndef BM_HIP_H
#define BM_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define BM_ACT_NONE 0
#define BM_ACT_GELU 1   /* exact erf GELU, nn.GELU()          bm/models/simpleconv.py:85-86 */
#define BM_ACT_RELU 2   /* nn.ReLU                             bm/models/simpleconv.py:89-90 */
#define BM_ACT_LEAKY 3  /* nn.LeakyReLU(relu_leakiness)        bm/models/simpleconv.py:87-88 */

/* ---- core ---- */
int bm_version(void);
const char* bm_last_error(void);
int bm_device_count(void);

/* ---- weight packing / grouping / split-K folding (pack.hip) ---- */
/* Tile geometry helpers shared with the host side. */
int bm_conv_mt_for(int M);
int bm_conv_mpad(int M);
int bm_conv_stats_tiles(int B, int T);
long bm_packed_weight_elems(int G, int M, int Cin, int KS);
/* dst[g][chunk][tap][16][Mpad] <- alpha * src[g*sg + m*sm + c*sc + tap'*sj]  (tap' flipped if flip).
 * Expresses nn.Conv1d weights (fwd and data-grad), SubjectLayers.weights (bm/models/common.py:49),
 * ConvTranspose1d(k=1) weights (simpleconv.py:189) and attention weights (common.py:357). */
int bm_pack_weights(const float* src, float* dst, int G, int M, int Cin, int KS, long sg, long sm,
                    long sc, long sj, int flip, const float* alpha_ptr, void* stream);
/* Stable grouping of segments by subject / layout index; replaces the gather at common.py:57.  order[0 .. seg[G]) lists
 * the segments with an index in [0, G) by group, in ascending segment order inside a group; any other index sets
 * *err_flag and its segment is left out (the tail of `order` is then not written).  B + G <= 16 383 (64 KiB of LDS). */
int bm_group_by_index(const long* idx, int B, int G, int* order, int* seg, int* err_flag, void* stream);
/* int64 -> int32 group indices with a range check: out-of-range entries set *err_flag (caller raises like
 * the reference's `self.weights.gather(0, subjects...)`, bm/models/common.py:57) and are clamped to 0. */
int bm_index_to_i32(const long* idx, int B, int G, int* out, int* err_flag, void* stream);
int bm_reduce_splits(const float* part, float* out, int G, int nsplit, int M, int Cn, int KS, long sg,
                     long sm, long sc, long sj, void* stream);
int bm_sum_over_batch(const float* x, float* out, int B, long n, void* stream);

/* ---- implicit-GEMM conv, fp32 MFMA (conv_nn.hip) ----
 * y[b][m][t] = ep(bias[m] + sum_{c,j} W[widx[b]][m][c][j] * x[b][c][t + (j-KS/2)*dil]).
 * Replaces F.conv1d (bm/models/common.py:113-114,133-138; simpleconv.py:113-120,185-189), the
 * einsums of SubjectLayers (common.py:58) and ChannelMerger (common.py:358), their data-gradients
 * and ClipLoss' dEstimate (losses.py:94 backward).  y_pre = value after bias; y_out = after
 * [affine ->] act [-> + res]; stats = per-tile (sum, sumsq) of y_pre for BatchNorm1d (common.py:119). */
int bm_conv1d_nn(const float* x, long x_bstride, const float* wpacked, const int* widx,
                 const float* bias, long bias_gstride, const float* ep_scale, const float* ep_shift, const float* res,
                 long res_bstride, float* y_pre, float* y_out, long y_bstride, float* stats, int B,
                 int Cin, int M, int T, int KS, int dil, int act, float leak, void* stream);

/* ---- strided / transposed conv, fp32 MFMA (conv_strided.hip)  bm/models/common.py:96, 112-114 ----
 * The reference's ConvSequence defaults (kernel 4, stride 2) and its decoder (`decode=True`: nn.ConvTranspose1d).
 * General in KS >= 1 (even kernels included), stride >= 1, dil >= 1, pad >= 0; exact-fp32 MFMA in every compute mode.
 *   bm_conv1d_strided     y[b][m][u] = ep(bias[m] + sum_{c,j} W[m][c][j] * x[b][c][u*stride + j*dil - pad])
 *   bm_conv1d_transposed  y[b][m][t] = ep(bias[m] + sum_{c,j} W[c][m][j] * x[b][c][(t + pad - j*dil) / stride])
 *                         over the (c, j) whose index is an integer; output_padding = 0
 * x is [B][Cin][T], y [B][M][Tout]; an index outside [0, T) reads as zero, so Tout is the caller's: the layer's
 * bm_conv1d_out_len(...) in the forward pass, the layer's INPUT length when one form serves as the data gradient of
 * the other (strided <-> transposed, same stride / dil / pad).  `wpacked` = bm_pack_weights with rows m (no tap flip in
 * either role); y_pre / y_out / ep_scale / ep_shift / act as bm_conv1d_nn; stats = [bm_conv_strided_stats_tiles][M][2]
 * partial (sum, sumsq) of y_pre for bm_bn_finalize.  Shapes whose staged window does not fit (stride * (128 + tap
 * span) > 576 floats in the strided form) return BM_ERR_UNSUPPORTED. */
int bm_conv1d_out_len(int T, int KS, int stride, int dil, int pad, int transposed);
int bm_conv_strided_stats_tiles(int B, int Tout, int stride, int transposed);
int bm_conv1d_strided(const float* x, long x_bstride, const float* wpacked, const float* bias,
                      const float* ep_scale, const float* ep_shift, float* y_pre, float* y_out, long y_bstride,
                      float* stats, int B, int Cin, int M, int T, int Tout, int KS, int stride, int dil, int pad,
                      int act, float leak, void* stream);
int bm_conv1d_transposed(const float* x, long x_bstride, const float* wpacked, const float* bias,
                         const float* ep_scale, const float* ep_shift, float* y_pre, float* y_out, long y_bstride,
                         float* stats, int B, int Cin, int M, int T, int Tout, int KS, int stride, int dil, int pad,
                         int act, float leak, void* stream);
/* Weight gradient of both layers (autograd of bm/models/common.py:96, 112-114), one kernel, operand roles swapped:
 *   part[split][r][q*KS + j] = sum over the split's share of (s, u) of a[s][r][u] * xl[s][q][u*stride + j*dil - pad]
 * strided layer: a = dY [S][M][Tout], xl = x [S][Cin][T] -> dW[m][c][j]; transposed layer: a = x [S][Cin][T],
 * xl = dY [S][M][Tout] -> dW[c][m][j].  Rows of a are U apart, rows of xl L apart.  Separate partial tiles, folded in
 * a fixed order by bm_reduce_splits(part, out, 1, nsplit, R, Q, KS, ...): deterministic. */
int bm_conv1d_strided_wgrad_suggest_splits(int R, int Q, int KS, int S, int U);
int bm_conv1d_strided_wgrad(const float* a, long a_sstride, const float* xl, long xl_sstride, float* part, int S,
                            int R, int Q, int U, int L, int KS, int stride, int dil, int pad, int nsplit,
                            void* stream);

/* ---- LSTM recurrence, fp32 MFMA (lstm.hip)  bm/models/convrnn.py:25-35 (nn.LSTM inside ConvRNN) ----
 * Time-major tensors [T][channels][B], B fastest.  One nn.LSTM layer per call, both directions when dirs = 2 (the *1
 * pointers are ignored when dirs = 1); one kernel launch per time step, stream order is the only synchronisation.
 *   forward   G_t = W_hh h_{t-1} + gx_t (gates i, f, g, o);  c_t = s(f) c_{t-1} + s(i) tanh(g);  h_t = s(o) tanh(c_t)
 *             whh_d = weight_hh_l{k}[_reverse] [4H][H] as nn.LSTM keeps it; gx_d [T][4H][B] = W_ih x + b_ih + b_hh
 *             (bm_conv1d_nn over all steps); y [T][H * dirs][B]; gates_d [T][4H][B] and c_d [T][H][B] are saved.
 *   backward  dy = dL/dy with dL/dh_n added at each direction's last step; dc_d [H][B] = dL/dc_n on entry, overwritten;
 *             dg_d [T][4H][B] = gradient of the gate pre-activations (operand of dX, dW_ih, dW_hh, the bias sums).
 * Any H, B, T >= 1; initial state zero; deterministic (no atomics). */
int bm_lstm_layer_fwd(const float* whh0, const float* whh1, const float* gx0, const float* gx1, float* y,
                      float* gates0, float* gates1, float* c0, float* c1, int H, int B, int T, int dirs,
                      void* stream);
int bm_lstm_layer_bwd(const float* whh0, const float* whh1, const float* dy, const float* gates0,
                      const float* gates1, const float* c0, const float* c1, float* dg0, float* dg1,
                      float* dc0, float* dc1, int H, int B, int T, int dirs, void* stream);

/* ---- fp32-ACCURATE contraction on the bf16 matrix cores: exact 3-way bf16 split of both operands,
 * six partial products per MFMA block, fp32 accumulate (conv_nn_x3.hip / gemm_nt_x3.hip).  Same
 * contracts as bm_conv1d_nn / bm_gemm_nt; compute mode "f32x3". */
long bm_packed_weight_elems_x3(int G, int M, int Cin, int KS);
int bm_pack_weights_x3(const float* src, void* dst, int G, int M, int Cin, int KS, long sg, long sm,
                       long sc, long sj, int flip, const float* alpha_ptr, void* stream);
int bm_conv1d_nn_x3(const float* x, long x_bstride, const void* wpacked, const int* widx,
                    const float* bias, long bias_gstride, const float* ep_scale, const float* ep_shift, const float* res,
                    long res_bstride, float* y_pre, float* y_out, long y_bstride, float* stats, int B,
                    int Cin, int M, int T, int KS, int dil, int act, float leak, void* stream);
int bm_gemm_nt_x3(const float* a, long a_sstride, long a_rstride, const float* x, long x_sstride,
                  long x_rstride, const int* order, const int* seg, float* part, int S, int G, int M,
                  int Cn, int T, int KS, int dil, int nsplit, void* stream);
/* tile height (MFMA row blocks: 3, 4, 5) and padded row count of the narrow f32x3 kernels */
int bm_conv_x3_mt_for(int M);
int bm_conv_x3_mpad(int M);

/* ---- fp32-ACCURATE contraction on the f16 matrix cores, compute mode "f16x2" (conv_nn_h2w.hip, pack_h2.hip): every operand
 * is scaled by a power of two (per tensor for activations, per output row for weights) and split into two f16
 * planes; three partial products per MFMA block, fp32 accumulate, exact inverse scaling in the epilogue.  Half
 * the matrix-core work of "f32x3" at the same parity tolerances.  Same conv contract as bm_conv1d_nn plus
 * `x_amax` (device pointer to an amax slot of the input tensor: 8 floats whose maximum is max|x|, from bm_amax or
 * published by the producing kernel) and G (weight groups packed).
 * Shapes bm_conv_h2_covers() rejects go through bm_conv1d_nn_x3 (also fp32-accurate). */
int bm_conv_h2_mw_for(int M);
int bm_conv_h2_mpad(int M);
int bm_conv_h2_covers(int Cin, int M, int T, int KS, int dil);
long bm_packed_weight_bytes_h2(int G, int M, int Cin, int KS);
int bm_pack_weights_h2(const float* src, void* dst, int G, int M, int Cin, int KS, long sg, long sm, long sc,
                       long sj, int flip, const float* alpha_ptr, void* stream);
/* Batched packing: every weight tensor of a model re-packed by ONE launch per optimizer step.  The host fills a
 * table of bm_pack_h2_job_bytes()-byte jobs with bm_pack_h2_job_fill (same arguments as bm_pack_weights_h2 plus the
 * job's first workgroup `block0`; returns the job's workgroup count, < 0 on bad arguments), copies the table to
 * device memory, and calls bm_pack_weights_h2_batch(table, njobs, sum of the workgroup counts, largest Cin * KS of the jobs). */
int bm_pack_h2_job_bytes(void);
int bm_pack_h2_job_fill(void* job, const float* src, void* dst, int G, int M, int Cin, int KS, long sg, long sm,
                        long sc, long sj, int flip, const float* alpha_ptr, int block0);
int bm_pack_weights_h2_batch(const void* jobs_dev, int njobs, int total_blocks, int max_nk, void* stream);
/* amax slots and workspace: a slot is 8 floats whose maximum is max|x|; `amax_ws` is 16384 floats of scratch that
 * the producers of one stream may share.  bm_amax / bm_amax_checked overwrite the slot (per-workgroup partial maxima
 * in `amax_ws`, folded by a one-workgroup kernel), and so do the PRODUCERS (`amax_out` / `y_amax_out` arguments
 * below).  (bm_clip_cand_prep is the one producer that raises its slot with atomic max: it wants it ZEROED; hip_ops
 * carves every slot out of zeroed pools.) */
int bm_amax_ws_elems(void);
int bm_amax(const float* x, long n, float* out, float* amax_ws, void* stream);
/* Same pass, plus the reference's finiteness assert (bm/solver.py:258-260): *nonfinite_flag (device int, nullable)
 * is set to 1 when x holds an inf or a nan. */
int bm_amax_checked(const float* x, long n, float* out, float* amax_ws, int* nonfinite_flag, void* stream);
/* `stats` (nullable; only together with y_pre alone, no affine / activation / residual: the training-mode BatchNorm
 * layers): CHANNEL-MAJOR [M][bm_conv_h2_stats_tiles(B, T)][2] per-(segment, column tile, wavefront column) partial
 * sums and sums of squares of y_pre, every entry written; input of bm_bn_finalize_cm with ntiles =
 * bm_conv_h2_stats_tiles(B, T). */
int bm_conv_h2_stats_tiles(int B, int T);
int bm_conv1d_nn_h2(const float* x, long x_bstride, const float* x_amax, const void* wpacked, const int* widx,
                    const float* bias, long bias_gstride, const float* ep_scale, const float* ep_shift, const float* res,
                    long res_bstride, float* y_pre, float* y_out, long y_bstride, float* stats, int B, int Cin,
                    int M, int T, int KS, int dil, int act, float leak, int G, float* y_amax_out, float* amax_ws,
                    void* stream);

/* f16x2 weight gradients (gemm_nt_h2w.hip): part[split][m][c*KS + j] over S consecutive segments, one group,
 * KS in {1, 3}; a_amax / x_amax = device pointers to max|a| / max|x| (bm_amax).  Shapes bm_gemm_nt_h2_covers()
 * rejects (grouped / ordered calls, tiny shapes) go through bm_gemm_nt_x3. */
int bm_gemm_nt_h2_covers(int M, int Cn, int KS, int S, int T, int G, int dil, int ordered);
int bm_gemm_nt_h2_suggest_splits(int M, int Cn, int KS, int S, int T);
int bm_gemm_nt_h2(const float* a, long a_sstride, long a_rstride, const float* a_amax, const float* x,
                  long x_sstride, long x_rstride, const float* x_amax, float* part, int S, int M, int Cn, int T,
                  int KS, int dil, int nsplit, void* stream);
/* The same with per-row maxima of `a` ([M] floats, nullable): every row of A -- one gradient channel = one row of dW --
 * carries its own power-of-two scale (320-row tile family, T % 4 == 0; otherwise the per-tensor scale applies). */
int bm_gemm_nt_h2_rows(const float* a, long a_sstride, long a_rstride, const float* a_amax, const float* a_row_amax,
                       const float* x, long x_sstride, long x_rstride, const float* x_amax, float* part, int S,
                       int M, int Cn, int T, int KS, int dil, int nsplit, void* stream);

/* Grouped form (KS = 1): group g contracts the segments order[seg[g] .. seg[g + 1]) (order nullable = identity; seg [G + 1]),
 * part[g][split][m][c] -- the per-(layout, subject) weight gradient of the composed front end and the per-subject
 * gradient of SubjectLayers (bm/models/common.py:55-58 backward).  bm_gemm_nt_h2_covers(..., G, dil, ordered) tells
 * whether a shape is covered; bm_gemm_nt_h2_suggest_splits_grouped the splits per group. */
int bm_gemm_nt_h2_grouped(const float* a, long a_sstride, long a_rstride, const float* a_amax, const float* x,
                          long x_sstride, long x_rstride, const float* x_amax, const int* order, const int* seg,
                          float* part, int S, int G, int M, int Cn, int T, int nsplit, void* stream);
int bm_gemm_nt_h2_suggest_splits_grouped(int M, int Cn, int KS, int S, int T, int G);

/* ClipLoss score contraction in compute mode "f16x2" (bm/losses.py:94, torch.einsum("bct,oct,o->bo") before the
 * candidate norms): part[split][b][o] = sum over the split's share of k of est[b][k] * cand[o][k]; est [B][K] and
 * cand [Bc][K] dense fp32, K = F * T; est_amax / cand_amax as for bm_gemm_nt_h2.  256 candidates x 256 (long K) or 128
 * (short K) estimates per tile, the partial tiles written with 16-byte stores; folded by bm_clip_ce.  Only shapes bm_clip_scores_h2_covers() accepts (Bc % 4 == 0,
 * operands below 2 GB, at most half of a tile padded); otherwise bm_gemm_nt_h2 with M = B, Cn = Bc computes the same. */
int bm_clip_scores_h2_covers(int B, int Bc, long K);
int bm_clip_scores_h2_suggest_splits(int B, int Bc, long K);
int bm_clip_scores_h2(const float* est, const float* est_amax, const float* cand, const float* cand_amax, float* part,
                      int B, int Bc, long K, int nsplit, void* stream);

/* ---- time-contraction GEMM, fp32 MFMA, split-K (gemm_nt.hip) ----
 * part[g,split][m][c*KS+j] = sum_{s in group g} sum_t A[s][m][t] * X[s][c][t + (j-KS/2)*dil].
 * Replaces aten::convolution_backward (weight part), the weight-grad einsums of SubjectLayers /
 * ChannelMerger, torch.einsum("bct,oct,o->bo") (losses.py:94) and einsum("bcd,bod->boc") (common.py:355).
 * bm_gemm_nt_suggest_splits: the split count of bm_gemm_nt / bm_gemm_nt_x3 for one group (G = 1: ~4 workgroups per
 * CU, >= 8 chunks of 32 samples each) and for G > 1 groups of ~S / G segments (splits per group, at most 8; its
 * constants are historical and fixed, they determine the summation order of the grouped gradients).
 * bm_clip_suggest_splits: the same for the ClipLoss score contraction, whose partial tiles are read back. */
int bm_gemm_nt_suggest_splits(int M, int Cn, int KS, int S, int T, int G);
int bm_clip_suggest_splits(int M, int Cn, int S, int T);
int bm_gemm_nt(const float* a, long a_sstride, long a_rstride, const float* x, long x_sstride,
               long x_rstride, const int* order, const int* seg, float* part, int S, int G, int M,
               int Cn, int T, int KS, int dil, int nsplit, void* stream);

/* ---- BatchNorm1d / activation / residual / GLU (norm_act.hip)  bm/models/common.py:113-151 ---- */
int bm_bn_finalize(const float* stats, int ntiles, int C, long count, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, long* num_batches,
                   float momentum, float eps, float* mean, float* invstd, float* scale, float* shift,
                   void* stream);
/* The same for channel-major partials stats[C][ntiles][2] (bm_conv1d_nn_h2's `stats`). */
int bm_bn_finalize_cm(const float* stats, int ntiles, int C, long count, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, long* num_batches,
                   float momentum, float eps, float* mean, float* invstd, float* scale, float* shift,
                   void* stream);
int bm_bn_eval_affine(int C, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, float* mean, float* invstd, float* scale,
                      float* shift, void* stream);
/* `amax_out` (nullable amax slot) + `amax_ws` on the elementwise producers: the slot receives max|output|, the
 * f16x2 scale of the contraction that consumes the tensor -- saves a separate bm_amax pass over it.
 * `amax_rows_out` (bm_act_bn_bwd / bm_glu_bwd; nullable, [C] resp. [2 H] floats): max |output| per CHANNEL -- a
 * gradient channel is a row of the weight gradient, which bm_gemm_nt_h2_rows scales row by row. */
int bm_affine_act_res(const float* y, const float* scale, const float* shift, const float* res,
                      float* out, int B, int C, int T, int act, float leak, float* amax_out, float* amax_ws,
                      void* stream);
int bm_bwd_nsplit(int B);
long bm_act_bn_bwd_workspace_bytes(int B, int C);
int bm_act_bn_bwd_set_fused(int mode);                    /* test hook -- 0: two passes; 1: one pass (-1: the default, one pass); returns the previous setting */
int bm_act_bn_bwd_set_poll_limit(int polls);              /* test hook: polls before a workgroup computes its partners' sums itself (-1: default) */
long bm_act_bn_bwd_fused_fallbacks(void);                 /* debug counter (synchronises): workgroups of the one-pass kernel that gave up on a partner and computed its sums themselves */
int bm_act_bn_bwd_fused_covers(int B, int C, int T);      /* 1: the shape is covered by the ONE-pass train-mode BatchNorm backward (slab in registers); taken when dout, y and dy are 16-byte aligned too */
int bm_act_bn_bwd(const float* dout, const float* y, const float* scale, const float* shift,
                  const float* mean, const float* invstd, int bn_train, float* dy, float* dgamma,
                  float* dbeta, float* dbias, void* workspace, long workspace_bytes, int B, int C,
                  int T, int act, float leak, float* amax_out, float* amax_ws, float* amax_rows_out,
                  void* stream);
long bm_channel_sum_workspace_bytes(int B, int C);
int bm_channel_sum(const float* x, long bstride, float* out, void* workspace, long workspace_bytes,
                   int B, int C, int T, void* stream);
/* one-pass per-channel (sum, sumsq) partials [nsplit][C][2] of a conv output, folded by bm_bn_finalize */
int bm_channel_stats_splits(int B);
int bm_channel_stats(const float* x, float* stats, int B, int C, int T, void* stream);
int bm_glu_fwd(const float* u, float* out, int B, int H, int T, float* amax_out, float* amax_ws, void* stream);
long bm_glu_bwd_workspace_bytes(int B, int H);
int bm_glu_bwd(const float* dout, const float* u, float* du, float* dbias, void* workspace,
               long workspace_bytes, int B, int H, int T, float* amax_out, float* amax_ws,
               float* amax_rows_out, void* stream);
/* out[c][b] = sum_t x[b][c][t]  (per-segment time sums, transposed; bias gradient of the composed front end:
 * bm/models/simpleconv.py:113-120 + bm/models/common.py:55-58 chained) */
int bm_time_sums_t(const float* x, float* out, int B, int C, int T, void* stream);

/* ---- ScaleReject front end (scale.hip)  bm/norm.py:86-87,255-261,325-341; bm/solver.py:245-246 ----
 * out = clamp((x - center[group[b]][c]) / scale[group[b]][c]); maxabs[b] = max|out[b]| (zero-init). */
int bm_center_scale(const float* x, float* out, const long* group, const float* center,
                    const float* scale, int B, int C, int T, int clip, float limit, float* maxabs,
                    void* stream);

/* ---- fitting the scalers (scaler_fit.hip)  bm/norm.py:58-80,96-105,136-142,85-86,110-111 ----
 * RobustScaler.fit (bm/norm.py:58-80 sorts one channel at a time and reads three values back): exact order statistics
 * of every channel by an MSD radix select.  x: fp32 [N][C][T]; column c = the n = N * T values x[:, c, :]; ranks: Q <= 8
 * ascending indices in [0, n), HOST memory; out[c][q] = the value at index ranks[q] of column c sorted ascending -- the
 * element torch.sort leaves there (all NaNs last; -0.0 / +0.0 may come back as either zero).  Integer counting only:
 * two runs are bit-identical.  n < 2^31.  `workspace` (bm_quantile_select_workspace_bytes) is ZEROED by the caller
 * before every call; the launches are ordered by the stream, no workgroup waits for another. */
long bm_quantile_select_workspace_bytes(int C, int Q);
int bm_quantile_select(const float* x, const long* ranks, float* out, int N, int C, int T, int Q, void* workspace,
                       long workspace_bytes, void* stream);
/* StandardScaler.fit (bm/norm.py:96-105) on the channels [f0, f1) of x [N][F][T] under a mask (mask_mode 0 = none,
 * 1 = bytes [N][1][T], 2 = bytes [N][F][T], as the regression kernels read them): count, mean and UNBIASED std, each
 * [f1 - f0]; per_channel = 0 (the reference's default) computes one statistic over all selected elements of the slice
 * and writes it to every channel.  fp64 partials folded in a fixed order, centred second walk, rounded to fp32 once.
 * count < 2: std = NaN (torch.std); count 0: mean = NaN. */
long bm_masked_moments_workspace_bytes(int channels);
int bm_masked_moments(const float* x, const unsigned char* mask, int mask_mode, int N, int F, int T, int f0, int f1,
                      int per_channel, float* mean, float* std, double* count, void* workspace, long workspace_bytes,
                      void* stream);
/* NoOpCategoryCountScaler.fit (bm/norm.py:136-142) on channel f of x [N][F][T]: counts[k] (fp32 like torch.histc,
 * [cardinality], ZEROED by the caller) = number of SELECTED values equal to k; *flags = the reference's assert over ALL
 * of the channel, masked or not: bit 1 = a value is not an integer, bit 2 = max >= cardinality, bit 4 = min != 0.
 * cardinality <= 16 384 (LDS histogram).  `workspace` (bm_category_counts_workspace_bytes): ZEROED before every call. */
long bm_category_counts_workspace_bytes(int cardinality);
int bm_category_counts(const float* x, const unsigned char* mask, int mask_mode, int N, int F, int T, int f,
                       int cardinality, float* counts, int* flags, void* workspace, long workspace_bytes, void* stream);
/* inverse_transform (bm/norm.py:85-86, 110-111): out = (x * scale[group[b]][c]) + center[group[b]][c], two roundings
 * like the reference's two ops; grouping as bm_center_scale.  In-place (out == x) allowed. */
int bm_center_scale_inverse(const float* x, float* out, const long* group, const float* center, const float* scale,
                            int B, int C, int T, void* stream);

/* ---- ChannelMerger front end (merger.hip)  bm/models/common.py:239-271,334-357 ---- */
int bm_fourier_emb(const float* positions, float* emb, long rows, int D, float margin, void* stream);
int bm_masked_softmax(const float* scores, const float* positions, const float* ban_center,
                      float ban_radius, float* weights, int U, int O, int C, void* stream);
int bm_softmax_bwd(const float* w, const float* dw, float* ds, long rows, int C, void* stream);

/* ---- ClipLoss (clip.hip)  bm/losses.py:77-114 ---- */
int bm_clip_inv_norms(const float* cand, int Bc, long K, float* inv_norm, void* stream);
/* The same norms plus, in the same pass over the candidates: max |cand| raised into a ZEROED amax slot (nullable; the
 * f16x2 scale of the score contraction) and the finiteness assert of bm/solver.py:258-260 (nullable device int). */
int bm_clip_cand_prep(const float* cand, int Bc, long K, float* inv_norm, float* amax_slot, int* nonfinite_flag,
                      void* stream);
/* *flag |= 1 when any byte of the bool mask is 0: ClipLoss.forward's `assert mask.all()` (bm/losses.py:110) without
 * a host synchronisation in the middle of the step (the Solver reads the flag word at its one sync point). */
int bm_flag_unless_all_set(const unsigned char* mask, long n, int* flag, void* stream);
int bm_clip_ce(const float* part, int nsplit, const float* inv_norm, float* scores, float* probs,
               float* dscaled, float* loss_row, float* loss, int B, int Bc, int target_offset,
               void* stream);
/* The same with a column mask (col_valid [Bc] floats, nullable; 0 = the candidate is padding): a masked candidate gets
 * score -inf, probability 0 and gradient 0.  Whole-node negatives when ranks rejected different numbers of segments
 * (bm/solver.py:245-246 ScaleReject next to the candidate all-gather of brainmagick_amd.solver). */
int bm_clip_ce_masked(const float* part, int nsplit, const float* inv_norm, const float* col_valid, float* scores,
                      float* probs, float* dscaled, float* loss_row, float* loss, int B, int Bc, int target_offset,
                      void* stream);

/* Column term of the symmetric CLIP objective (opt-in extension named by the hot-path contract, "row/col softmax";
 * the reference computes the row term only, bm/losses.py:104-114): for every target candidate o = target_offset + j,
 * loss_col[j] = logsumexp_b scores[b][o] - scores[j][o].  dscaled (nullable; holds bm_clip_ce's row term) becomes
 * w_row * row term + w_col * (softmax over the column - onehot) / B * inv_norm[o] in place; loss (nullable; holds the
 * row loss) becomes w_row * loss + w_col * mean(loss_col). */
int bm_clip_ce_cols(const float* scores, const float* inv_norm, float* dscaled, float* loss_col, float* loss, int B,
                    int Bc, int target_offset, float w_row, float w_col, void* stream);

/* ---- regression objective: L1Loss / L2Loss and their test metrics (regress.hip)  bm/losses.py:11-26 ----
 * est, out: fp32 [B][F][T]; mask: null (all true), mask_mode 1 = bytes [B][1][T] broadcast over F (SegmentBatch
 * .features_mask), mask_mode 2 = bytes [B][F][T]; nonzero = selected.  kind 0 = L1 (|d|), 1 = MSE (d^2), d = e - o.
 * Forward (ONE launch): *loss = sum_selected w(d) / count (fp64 partials, folded in a fixed order by the workgroup that
 * finishes last), *count = number of selected elements -- torch.nn.L1Loss() / MSELoss() on est[mask.expand_as(est)].
 * count == 0 gives NaN and raises bit 2 of flag (nullable; the Solver's flag word slot 2): the reference's "no mask!"
 * assert, bm/solver.py:354-356.  `workspace` (bm_regress_workspace_bytes) holds the partials and the ticket counters:
 * ZEROED by the caller once; every launch leaves its counter at zero again. */
long bm_regress_workspace_bytes(void);
int bm_regress_loss_fwd(const float* est, const float* out, const unsigned char* mask, int mask_mode, int B, int F,
                        int T, int kind, float* loss, double* count, void* workspace, long workspace_bytes, int* flag,
                        void* stream);
/* Backward (ONE launch): d_est = g * w'(d) * m / count with g = *grad_out and count read on the device (w' = sign,
 * sign(0) = 0, for L1; 2 d for MSE); d_out (nullable: a learnable feature model) = -d_est.  amax_out (nullable amax
 * slot, compute mode f16x2) receives max |d_est| and amax_rows_out ([F] floats, nullable) the per-channel maxima, like
 * bm_glu_bwd / bm_act_bn_bwd publish them: the head's backward contractions need no bm_amax pass. */
int bm_regress_loss_bwd(const float* est, const float* out, const unsigned char* mask, int mask_mode, int B, int F,
                        int T, int kind, const float* grad_out, const double* count, float* d_est, float* d_out,
                        float* amax_out, float* amax_rows_out, void* workspace, long workspace_bytes, void* stream);
/* Test metrics, bm/metrics.py:37-170 with dim = 0 (OnlineCorrelation, L1Reg, L2Reg; bm/play.py:149-151 casts to
 * double): acc = 8 planes of [F][T - t0] fp64 accumulators, += per (f, t) over b, in b order: sum l r m, sum l m,
 * sum r m, sum (l m)^2, sum (r m)^2, sum m, sum ((l - r) m)^2, sum |(l - r) m|.  Only the columns t >= t0 (trim_offset,
 * bm/play.py:144-147).  Rows T floats apart, segments est_bstride / out_bstride floats and mask_bstride bytes apart;
 * mask_full = 0: mask [B][1][T], 1: [B][F][T]; mask null = all true. */
int bm_regress_metric_update(const float* est, long est_bstride, const float* out, long out_bstride,
                             const unsigned char* mask, long mask_bstride, int mask_full, int B, int F, int T, int t0,
                             double* acc, void* stream);

/* ---- the encode task's model input (encode.hip)  bm/solver.py:288-292 ----
 * meg, x: contiguous fp32 [B][C][T].  x[b][c][t] = meg[b][c][t] for t < limit and +0.0 for every other t: the
 * reference's `mask * meg` with mask[:limit] = 1 (limit <= 0: all zeros; limit >= T: a copy).  ONE launch: only the
 * head of meg is read, every element of x is written exactly once (no fill needed), 16-byte accesses when T % 4 == 0
 * and both pointers are 16-byte aligned.  Unlike the product, a tail element is +0.0 where meg is negative and 0 where
 * meg is not finite.  amax_out (nullable amax slot, compute mode f16x2) receives max |x|, folded by the workgroup that
 * finishes last; it needs `workspace` (bm_meg_init_workspace_bytes: ticket counter + partial maxima), ZEROED by the
 * caller once -- every launch leaves the counter at zero again.  B == 0 returns without a launch. */
long bm_meg_init_workspace_bytes(void);
int bm_meg_init(const float* meg, float* x, int B, int C, int T, int limit, float* amax_out, void* workspace,
                long workspace_bytes, void* stream);

/* ---- task.lowpass (lowpass.hip)  bm/solver.py:278-281 ----
 * julius.lowpass_filter(x, cutoff, zeros) with stride 1 and pad=True as one launch: a FIR of 2 * half + 1 taps over the
 * replicate-padded rows,  y[r][t] = sum_k taps[k] * x[r][clamp(t + k - half, 0, T - 1)]  for t < keep and +0.0 for
 * t >= keep (keep saturates to [0, T]; keep < T is the encode task's `mask * lowpass(meg)`, which reads only
 * x[r][0 : min(T, keep + half)] and, like bm_meg_init, gives +0.0 in the tail whatever x holds there).
 * x: `rows` rows of T fp32 samples, unit stride inside a row, row_stride >= T floats between rows (a view
 * meg[..., offset:] is read in place); nothing outside [row start, row start + T) is read.  y: contiguous [rows][T],
 * every element written exactly once.  taps: 2 * half + 1 floats on the device.  The sum is always the direct one, fp32
 * fmaf with k ascending from 0.f: the scalar and the 16-byte paths (loads: x and row_stride 16-byte aligned; stores:
 * T % 4 == 0 and y aligned), every grid and every keep give the same bits.  T + 2 * half <= 8192 (the padded row is
 * staged in LDS), else BM_ERR_UNSUPPORTED; rows * T < 2^31.  amax_out (nullable amax slot, compute mode f16x2) receives
 * max |y|, folded by the workgroup that finishes last; it needs `workspace` (bm_lowpass_workspace_bytes: ticket counter
 * + partial maxima), ZEROED by the caller once -- every launch leaves the counter at zero again.  rows == 0 returns
 * without a launch. */
long bm_lowpass_workspace_bytes(void);
int bm_lowpass(const float* x, long row_stride, float* y, int rows, int T, int keep, const float* taps, int half,
               float* amax_out, void* workspace, long workspace_bytes, void* stream);

/* ---- optim.svd (spectral.hip)  bm/svd.py:17-45, bm/solver.py:379-380 ----
 * svd_penalty: for every penalised weight A = p.view(p.shape[0], -1) (bm/svd.py:40) the estimate
 * torch.svd_lowrank(A, dim, niters)[1][0] ** 2 (bm/svd.py:44) and its gradient in closed form, all matrices of a model
 * in the same launches.  A table entry (bm_spectral_table_entry_bytes bytes, filled on the host by
 * bm_spectral_table_fill, then copied to the device) describes one matrix: `w` rows x cols fp32 read in place with
 * `ld` floats between rows, `r_off` the first of its min(rows, cols) rows in the Gaussian test matrix R [sum, dim]
 * (of which the first min(dim, rows, cols) columns are used), its offsets into the two workspaces (floats: a multiple
 * of 16; sizes from bm_spectral_ws_floats / _doubles) and into the flat gradient buffer.  dim 1..16, niters 0..8.
 * bm_spectral_fwd: 2 niters + 2 stage launches over a (64-row slab, matrix) grid (max_slabs: the largest
 * cdiv(max(rows, cols), 64)), one Jacobi launch, one that adds the estimates: values[nmat], *total.  The products are
 * exact-fp32 MFMA in every compute mode; the 16 x 16 Gram matrices, their Cholesky factors and the eigenpair are fp64.
 * bm_spectral_bwd (after bm_spectral_fwd on the same workspaces, which carry the forward's bases): 2 niters + 2
 * launches of the same kernel and one (max_tiles: the largest cdiv(rows, 64) * cdiv(cols, 64)) that writes
 * grads[g_off + r * cols + c] = *gscale * d value / d A[r][c], every element once.  Stream order is the only
 * synchronisation, no atomics: the same bits every run.  The workspaces need no initialisation and hold no state
 * between calls.  nmat == 0 returns without a launch. */
long bm_spectral_table_entry_bytes(void);
long bm_spectral_ws_floats(int rows, int cols, int niters);
long bm_spectral_ws_doubles(int rows, int cols, int niters);
int bm_spectral_table_fill(void* entry, const float* w, int rows, int cols, long ld, int dim, long r_off,
                           long ws_float_off, long ws_double_off, long grad_off);
int bm_spectral_fwd(const void* table, int nmat, int max_slabs, const float* R, int dim, int niters,
                    float* ws_floats, double* ws_doubles, float* values, float* total, void* stream);
int bm_spectral_bwd(const void* table, int nmat, int max_slabs, int max_tiles, int niters, float* ws_floats,
                    double* ws_doubles, const float* gscale, float* grads, void* stream);

/* ---- the data loader's batch (segments.hip)  bm/dataset.py:349-364, 263-278, 172-175 ----
 * SegmentDataset.__getitem__ + SegmentBatch.collate_fn + the baseline correction of mne.Epochs(..., baseline=...) as ONE
 * launch per tensor over recordings that are resident on the device:
 *     dst[b][c][t] = src_r[c][start_b + t] - mean_b,c   for c < rows_r,   +0.0 for rows_r <= c < C (the F.pad to
 * meg_dimension, bm/dataset.py:353-354), with r = rec[first + b], start_b = start[first + b].
 * table: R entries (bm_segment_table_entry_bytes bytes each, filled on the host by bm_segment_table_fill, then copied to
 * the device): the address of a recording's [rows][n] array (unit stride inside a row, n elements between rows), n and
 * rows -- the recordings are read in place.  rec / start: int32 [n_index] on the device, the arrays of a whole epoch;
 * a batch is the B segments from `first` on.  elem_bytes 4 (fp32) or 1 (bytes: the features mask).
 * Baseline (fp32 only): base0 < 0 = none, the source bits pass through; else mean_b,c is the fp64 sum of the row's
 * window samples base0..base1 (inclusive, 0 <= base0 <= base1 < T) in ascending t, divided once, and the difference is
 * taken in fp64 and rounded once -- one order: the same bits on every grid, alone or among other segments.  A NaN
 * inside the baseline window makes the row NaN.
 * A rec outside [0, R) or a start outside [0, n - T] is checked BEFORE any address is formed: the whole segment is
 * +0.0 and *flag (one int32 on the device, the caller's) is set to 1 by a plain store.  dst: contiguous [B][C][T],
 * 4-byte aligned (16-byte stores are used wherever the flat output allows), every element written exactly once.
 * fp32: T <= 4096, else BM_ERR_UNSUPPORTED; B * C * T < 2^31.  No atomics, no scratch; B == 0 returns without a launch.
 * The byte path is sized for the one-row mask of the reference: one byte per thread, the segment re-checked per byte;
 * correct for any C, slow for a wide one. */
long bm_segment_table_entry_bytes(void);
int bm_segment_table_fill(void* entry, const void* base, long n, int rows);
int bm_segment_gather(const void* table, int R, const int* rec, const int* start, long n_index, long first, int B, int C,
                      int T, int base0, int base1, int elem_bytes, void* dst, int* flag, void* stream);

/* ---- the batch's features from resident events (features.hip)  bm/features/base.py:68-122, 238-267 ----
 * FeaturesBuilder.__call__ with Feature.get_on_overlap, DataSlice.overlap / slice_in_parent (bm/events.py:80-111),
 * MelSpectrum.get (bm/features/audio.py:78-83) and the Wav2Vec chunk rule (bm/features/audio.py:211-274) as ONE launch per
 * batch: dst [B][F][T] fp32 and mask [B][1][T] bytes, both contiguous, every element written exactly once; each output is a
 * copy (a value row, an array entry or a default), the index arithmetic is the reference's in fp64 with rint for round,
 * uncontracted (the rules are written out at the top of features.hip).
 * feat_table (HOST memory): NF <= 32 rows {kind, rule, first channel, channels}, tiling [0, F) in order; kind in [0, NK);
 * rule 0 = constant (one value row per event), 1 = resampled (nearest interpolation of the event's array to the event's
 * own length, then the default get_on_overlap cut with its one-sample replicate pad), 2 = chunk (the wav2vec cut of the
 * overlap, then nearest interpolation to the overlap's length).  feat_default (HOST): the value of unpainted samples.
 * mask_kind: -1 = the mask is all true, else true exactly where an event of that kind paints.
 * kinds: [R][NK] entries (bm_features_table_entry_bytes(0) bytes each, filled by bm_features_kind_fill): the events of
 * one kind of one recording in painting order -- start (non-decreasing), duration and the running maximum of start +
 * duration, float64 on the device; within a kind a later event overwrites an earlier one.  srcs: [R][NF] entries
 * (..entry_bytes(1), bm_features_source_fill): constant = float [n][channels] on the device; otherwise n entries
 * (..entry_bytes(2), bm_features_array_fill) {address of the event's [channels][L] array, read in place, 1 <= L < 2^31,
 * er = L / duration}.  rec: int32 [n_index], wstart / wdur: float64 [n_index] (the window's start and duration in
 * seconds, from the host's division), the arrays of a whole epoch; a batch is the B segments from `first` on.
 * A rec outside [0, R) is checked BEFORE any table address is formed: the segment is defaults (mask false, or true when
 * mask_kind = -1) and *flag is set to 1 by a plain store.  T <= 4096 and NF <= 32, else BM_ERR_UNSUPPORTED; B <= 65535.
 * No atomics, no scratch; B == 0 returns without a launch. */
long bm_features_table_entry_bytes(int which);
int bm_features_kind_fill(void* entry, const double* start, const double* dur, const double* runmax, long n);
int bm_features_source_fill(void* entry, const void* data);
int bm_features_array_fill(void* entry, const float* base, long L, double er);
int bm_segment_features(const int* feat_table, const float* feat_default, int NF, int NK, int mask_kind,
                        const void* kinds, const void* srcs, int R, const int* rec, const double* wstart,
                        const double* wdur, long n_index, long first, int B, int F, int T, double sr, float* dst,
                        unsigned char* mask, int* flag, void* stream);

/* ---- the wave table of the three audio units below (csrc/bm_wave.h) ----
 * table: n_waves <= 65535 entries of bm_wave_table_entry_bytes bytes on the device, each filled on the host by
 * bm_wave_table_fill: {x: a 1-D fp32 waveform on the device, read in place; out: where the unit stores that waveform's
 * result (null for bm_wave_moments), both 4-byte aligned; L: its length, 1 <= L < 2^31}.  lengths (HOST memory): the same
 * lengths, for the grid and the checks. */
long bm_wave_table_entry_bytes(void);
int bm_wave_table_fill(void* entry, const float* x, long L, float* out);

/* ---- the MelSpectrum targets from resident waveforms (mel.hip)  bm/features/audio.py:61-76 ----
 * MelSpectrum._compute behind the channel mean: (wav - wav.mean()) / (1e-8 + wav.std()) (unbiased std), then
 * torchaudio.transforms.MelSpectrogram(n_fft, hop = n_fft / 4, normalized) RESTATED from its documentation -- torch.stft
 * with center=True, reflect padding, a periodic Hann window of n_fft samples, divided by sqrt(sum w^2) when normalized,
 * |.|^2, times the htk filterbank -- and log10(mel + eps).  Two launches for any number of waveforms.
 * table, lengths: the wave table, `out` the [n_mels][1 + L / hop] output of the waveform.
 * bm_wave_moments: mom[w] = {mean, 1 / (1e-8 + unbiased std)} in fp64, ONE launch over a (split, waveform) grid: a
 * waveform is cut into bm_wave_moments_splits(L) splits (a function of L alone), every split is walked twice (its sum,
 * then its squares centred on its own mean) and the workgroup of a waveform that finishes last folds the partials in
 * split order.  tickets: n_waves counters, ZEROED by the caller once (every launch leaves them at zero); part: room for
 * [n_waves][max_splits][2] doubles.  L = 1 gives a NaN scale, like torch.std.
 * bm_mel_spectrogram: ONE launch over a (frame tile of bm_mel_frame_tile(n_fft) frames, waveform) grid; every output
 * element is stored exactly once, no atomics.  mom: what bm_wave_moments wrote, or null for (0, 1); a sample enters as
 * (float)(((double)x - shift) * scale).  basis: [n_fft][2 nbp] fp32, nbp = n_fft / 2 + 1 rounded up to 16: column b <
 * nbp is w[k] cos(2 pi k b / n_fft) / norm, column nbp + b is -w[k] sin(...) / norm, zero for b > n_fft / 2.  The
 * contraction is v_mfma_f32_16x16x4_f32 in one fixed blocked order (per quarter of the window: chains of 8 samples with
 * k ascending, added in ascending order; quarters folded as (q0 + q1) + (q2 + q3)): a frame's bits do not depend on its
 * tile, the grid or the other waveforms.  fbw: [n_mels][n_fft / 2 + 1] filter weights; range (device) and range_host (HOST, the same values):
 * [n_mels][2] = the bins [lo, hi) that row m sums, ascending, by fmaf from 0.f.  8 <= n_fft <= 2048, n_fft % 4 == 0,
 * n_mels <= 256, n_fft / 2 < L, n_waves <= 65535. */
int bm_mel_frame_tile(int n_fft);
int bm_wave_moments_splits(long L);
int bm_wave_moments(const void* table, const long* lengths, int n_waves, unsigned* tickets, double* part,
                    int max_splits, double* mom, void* stream);
int bm_mel_spectrogram(const void* table, const long* lengths, int n_waves, const double* mom, const float* basis,
                       int n_fft, int nbp, const float* fbw, const int* range, const int* range_host, int n_mels,
                       int use_log, float eps, void* stream);

/* ---- julius' fractional resampler over resident waveforms (resample.hip)  bm/features/audio.py:66, 113, 186 ----
 * julius.resample.ResampleFrac(old_sr, new_sr, zeros, rolloff) RESTATED from its published definition, ONE launch for
 * every waveform of one reduced ratio old_rate / new_rate (already divided by their gcd, old_rate != new_rate):
 *     out[f new + i] = sum_k taps[i][k] padded[f old + k],  k < ntaps = 2 width + old,  f new + i < floor(new L / old),
 * `padded` the waveform replicate-padded by width samples on the left and width + old on the right (indexed in place: no
 * padded copy).  table, lengths: the wave table, `out` the floor(new L / old) outputs of the waveform.
 * mom: null, or what bm_wave_moments wrote for the same table: a sample
 * enters as (float)(((double)x - shift) * scale).  taps: [ntp][newp] fp32, taps[k][i] the tap k of phase i, ntp = ntaps
 * rounded up to 4 and newp = new rounded up to 16, zero beyond ntaps and beyond new.  Grid (tile of
 * bm_resample_frames_tile frames, waveform); the samples a tile covers are staged in LDS once.  new >= 16:
 * v_mfma_f32_16x16x4_f32, 16 frames x 16 phases per wavefront, one accumulator chain with k ascending; new < 16: one
 * fmaf chain per output with k ascending.  A ratio always takes the same variant: an output's bits do not depend on its
 * tile, the grid or the other waveforms.  Every output is stored exactly once, no atomics.
 * Limits (BM_ERR_ARG; bm_resample_frames_tile returns 0): new <= 4096 and 15 old + ntp <= 16384 floats (the 64 KiB of
 * LDS that 16 frames cover); 1 <= L < 2^31 and floor(new L / old) < 2^31; n_waves <= 65535. */
int bm_resample_frames_tile(int old_rate, int new_rate, int width);
int bm_resample_frac(const void* table, const long* lengths, int n_waves, const double* mom, const float* taps,
                     int old_rate, int new_rate, int width, void* stream);

/* ---- a long FIR over long rows (fir.hip)  bm/studies/api.py:334-363 (preprocess_mne's highpass) ----
 * With half = (ntaps - 1) / 2, ONE launch:
 *     s[r][t] = sum_{k < ntaps} taps[k] * x[r][clamp(t + k - half, 0, T - 1)],   y[r][t] = subtract ? x[r][t] - s : s
 * -- bm_lowpass's replicate padding, but rows are tiled in time and the taps are walked in chunks, so neither T nor half
 * is bounded by LDS.  x: `rows` rows of T fp32 samples, unit stride inside a row, row_stride >= T floats between rows (a
 * view is read in place); nothing outside [row start, row start + T) is read.  y: contiguous [rows][T], every element
 * stored exactly once, no atomics.  taps: ntaps floats on the device.  Grid (tile of bm_fir_tile outputs, row); the tap
 * axis is walked in chunks of bm_fir_chunk values of j = tap + column, j in [0, ntaps + 15).
 * Arithmetic: v_mfma_f32_16x16x4_f32 in every compute mode, the Toeplitz form of the resampler, ONE accumulator chain per
 * output with j ascending from 0.f carried across the chunks: an output's bits depend on its own window alone (not on
 * the tile, the grid, the chunking or the other rows), and for finite input the outputs equal bm_lowpass's as numbers
 * wherever that kernel applies.  A non-finite sample makes non-finite every output within `half` of it, may do so up to
 * 15 samples further (0 * NaN in the zero corners of the Toeplitz operand), and nothing beyond.
 * Limits (BM_ERR_ARG): 1 <= T < 2^31, rows <= 65535, ntaps odd, half <= bm_fir_max_half (16384); pointers 4-byte
 * aligned; row offsets are 64-bit (rows * T is not limited).  rows == 0 returns without a launch. */
int bm_fir_tile(void);
int bm_fir_chunk(void);
int bm_fir_max_half(void);
int bm_fir_rows(const float* x, long row_stride, float* y, int rows, long T, const float* taps, int ntaps, int subtract,
                void* stream);

/* ---- the Pitch feature from resident waveforms (pitch.hip)  bm/features/audio.py:110-124, bm/lib/pitch_calc/yin.py ----
 * compute_yin(sig, sr, w_len, w_step, f0_min, f0_max, harmo_thresh)[0] as ONE launch: frame t < ceil((L - w_len) /
 * w_step) starts at t w_step;  d(tau) = sum_{j < w_len - tau} (x_j - x_{j + tau})^2  in fp64 with j ascending (the
 * reference's FFT expression as a sum);  c(0) = 0, c(tau) = d(tau) tau / sum_{1..tau} d  with the running sum in
 * ascending tau;  the first tau in [tau_min, tau_max) with c < thresh, walked down while c(tau + 1) < c(tau) and tau + 1 <
 * tau_max;  out[t] = (float)(sr / tau), or 0.f when there is none.  A silent frame (0 / 0) and a frame holding a NaN or
 * an Inf give 0.f.  table, lengths: the wave table, `out` the waveform's frames.  Grid (tile of
 * bm_yin_frames_tile frames, waveform), one wavefront per frame, samples staged in LDS once; no atomics.
 * Limits (BM_ERR_ARG): w_len < L < 2^31, 2 <= w_len <= 1024, 1 <= w_step <= 512, 1 <= tau_min, tau_max <= w_len,
 * n_waves <= 65535. */
int bm_yin_frames_tile(void);
int bm_yin_pitch(const void* table, const long* lengths, int n_waves, double sr, int w_len, int w_step, int tau_min,
                 int tau_max, double thresh, void* stream);

/* ---- FeatureDecodingLoss and ClassificationAcc (regress.hip) bm/losses.py:117-173, bm/metrics.py:173-180 ----
 * est: fp32 [B][C][T] (the model output), out: fp32 [B][Co][T] (the features), mask: null (all true) or bytes
 * [B][1][T].  table (HOST memory): n_features rows {kind, est_start, width, out_start, weight_off}: kind 0 = continuous
 * (width channels of est and of out, MSE over the selected positions and those channels), 1 = categorical (width = K
 * logits in est, ONE channel of out holding the class as a float, truncated towards zero like .long(); cross-entropy
 * weighted by weights[weight_off + class], weight_off = -1: unweighted).  The rows must tile est's and out's channels in
 * order; at most 16 features, K <= 16384, B C T < 2^31 -- anything else is BM_ERR_ARG.
 * Forward (ONE launch): terms[f] = numerator / denoms[f] per feature (continuous: sum (e - o)^2 / (n_selected width);
 * categorical: sum w_y (logsumexp(x) - x_y) / sum w_y, torch's weighted mean), *loss = their fp32 sum in feature
 * order, lse [n_categorical][B][T] = the logsumexp of every position (saved for the backward).  One pass over the K
 * logits (running maximum and sum), fp64 sums, workgroup partials folded in a fixed order by the workgroup that finishes
 * last (workspace: bm_regress_workspace_bytes, as for bm_regress_loss_fwd).  Unselected positions are dropped by
 * select.  flag (nullable, the Solver's flag word slot 2): bit 2 when nothing is selected (the loss is NaN; the
 * reference's `assert mask.any()`, bm/losses.py:133), bit 4 when ANY position holds a class >= K or a selected one a
 * negative or NaN class (bm/losses.py:150; torch would raise) -- such a position contributes nothing.  -100 has no
 * special meaning (the reference's features never produce torch's ignore_index). */
int bm_feature_decoding_fwd(const float* est, const float* out, const unsigned char* mask, const float* weights,
                            long n_weights, const int* table, int n_features, int B, int C, int Co, int T, float* loss,
                            float* terms, double* denoms, float* lse, void* workspace, long workspace_bytes, int* flag,
                            void* stream);
/* Backward (ONE launch): d_est = g 2 (e - o) / denoms[f] on continuous channels, g (w_y / denoms[f]) (softmax(x)_k -
 * [k = y]) on categorical ones, exactly 0 at unselected (or out-of-range) positions; EVERY element of d_est is
 * written once (no fill pass needed).  g = *grad_out, denoms and lse are read on the device. */
int bm_feature_decoding_bwd(const float* est, const float* out, const unsigned char* mask, const float* weights,
                            long n_weights, const int* table, int n_features, int B, int C, int Co, int T,
                            const float* grad_out, const double* denoms, const float* lse, float* d_est, void* stream);
/* ClassificationAcc.update, bm/metrics.py:173-180 with dim = 0: est [B][K][T] (rows T floats apart), target = ONE
 * channel [B][T], mask bytes [B][1][T] or null; segments est_bstride / target_bstride floats and mask_bstride bytes
 * apart.  acc = int64 [2][T - t0]: hits and selected count per column t >= t0 (trim_offset, bm/play.py:144-147),
 * accumulated in place.  Prediction = first index of the maximum (NaN counts as the maximum: torch.argmax); a hit is
 * (float)prediction == target. */
int bm_class_acc_update(const float* est, long est_bstride, const float* target, long target_bstride,
                        const unsigned char* mask, long mask_bstride, int B, int K, int T, int t0, long* acc,
                        void* stream);

/* Gradient of ClipLoss w.r.t. the candidates (learnable feature model, bm/solver.py:304-320):
 * coef[o] = alpha * (sum_b dscaled[b,o]*scores[b,o]) / |cand_o| ;  y[r] -= coef[r] * x[r]. */
int bm_clip_cand_coef(const float* dscaled, const float* scores, const float* inv_norm,
                      const float* alpha, float* coef, int B, int Bc, void* stream);
int bm_row_axpy_sub(float* y, const float* x, const float* coef, int rows, long K, void* stream);
/* Retrieval evaluation: top-k columns per row + "own label among the top-k labels" hit flag.
 * Replaces probs.topk + label gather/compare of scripts/run_eval_probs.py:237-264 and bm/wer.py:104-111.
 * The order of a row's columns, idx_out[row][0 .. k):
 *   - by value, descending;
 *   - NaN ranks above +inf, as torch.topk / torch.sort rank it (an all-NaN row returns columns 0 .. k-1);
 *   - equal values (NaN with NaN, -0 with +0) go by ascending column: torch.sort(descending, stable) cut to k;
 *   - with k > cols the positions past `cols` hold index -1 (and value -inf); they never count as a hit.
 * val_out holds the values of those columns, bit for bit.  hit_out[row] = 1 when col_labels[idx] == row_labels[row]
 * (int64 compare) for any of the row's returned columns. */
int bm_topk_rows(const float* x, int rows, int cols, int k, int* idx_out, float* val_out,
                 const long* col_labels, const long* row_labels, int* hit_out, void* stream);

/* Word-level retrieval, batched (bm/wer.py:91-116): row softmax, per-row dot products (own target
 * replaces the last negative), per-vocabulary-word sums over columns pre-sorted by word. */
int bm_row_softmax(const float* x, float* y, int rows, int cols, void* stream);
int bm_rowwise_dot(const float* a, const float* b, const float* scale, float* out, int rows, long K,
                   void* stream);
int bm_segment_sum_cols(const float* p, const int* order, const int* seg, float* pv, int rows, int cols,
                        int V, void* stream);

/* ---- the word label of every kept test segment (wer.hip)  bm/wer.py:48, 58-66 ----
 * x: the batch's full features fp32 [B][F][T], read in place; c: the channel of the WordHash feature; mask:
 * reject_mask bytes [B] (non-zero = kept) or null (all kept).  For the kept rows in ascending order, rank r:
 * dest[n0 + r] = (int64, the exact integer of the fp32 value) the first non-zero of x[t0], x[t0 - 1] (only if t0 > 0),
 * x[t0 + 1], x[t0 - 2] (only if t0 > 1), x[t0 + 2]: the torch.where chain of bm/wer.py:58-64 over
 * word_hash[reject_mask].  No other element of dest is written, nothing past dest_len.  *flag |= 1: every candidate of a
 * kept row is zero (the assert of bm/wer.py:65; 0 is stored); 2: the value is not finite, not an integer or |v| >= 2^63;
 * 4: n0 + r reached dest_len.  ONE launch of one workgroup, no atomics; the same bits on every run.
 * t0 < 0, t0 + 2 >= T, c outside [0, F) and n0 outside [0, dest_len] are BM_ERR_ARG before any launch. */
int bm_word_hash_pick(const float* x, int B, int F, int T, int c, int t0, const unsigned char* mask, long* dest,
                      long dest_len, long n0, int* flag, void* stream);

/* ---- the labels of every kept test segment of the segment-level evaluation (segment_eval.hip)
 * scripts/run_eval_probs.py:27-57 (_get_extra_info), scripts/run_eval_probs.py:105-130, 155-158 (_load_test_data) ----
 * x: the batch's full features fp32 [B][F][T], read in place; c: the channel of the WordHash feature; mask: reject_mask
 * bytes [B] (non-zero = kept) or null.  rec (int32), wstart (fp64 seconds), subject_index / recording_index (int64): the
 * epoch's arrays of n_index segments, the batch starts at `first`.  kinds: the event table of bm_segment_features ([R][NK]
 * entries; word_kind: the slot of the word events); infos: [R] entries of bm_segment_eval_info_fill, one int64 array
 * [n_words][3] = (word_index, sequence_id, segment_id) per recording.  For the kept rows in ascending order, rank r:
 * dest[n0 + r][0 .. 7) = word_hash, word_index, sequence_id, segment_id, subject_index, recording_index, word_event.
 *   word_hash  = the exact integer of the first non-zero of x[t0], x[t0 - 1] (only if t0 > 0), x[t0 + 1]
 *                (scripts/run_eval_probs.py:116, 122-130); all zero is legal and stored as 0;
 *   word_event = the last word event in table order with max(0, trunc(a)) <= t0 < min(T, trunc(b)), a = sr * (start -
 *                wstart), b = a + sr * duration in fp64 (scripts/run_eval_probs.py:43-47), -1 without one; then
 *                word_index = sequence_id = -1 and segment_id = 0, else the word-info row.
 * *flag |= 1: the word hash is not finite, not an integer or |v| >= 2^63; 2: n0 + r reached dest_rows; 4: a recording
 * index outside [0, R) (that row gets the no-word values).  ONE launch, a wavefront per row; no atomics on dest, one OR
 * per workgroup that has a bit; the same bits on every run.  t0 < 0, t0 + 1 >= T, c outside [0, F) and n0 outside
 * [0, dest_rows] are BM_ERR_ARG before any launch. */
long bm_segment_eval_info_entry_bytes(void);
int bm_segment_eval_info_fill(void* entry, const long* rows, long n);
int bm_segment_eval_labels(const float* x, int B, int F, int T, int c, int t0, const unsigned char* mask,
                           const int* rec, const double* wstart, const long* subject_index,
                           const long* recording_index, long n_index, long first, const void* kinds, int NK,
                           int word_kind, const void* infos, int R, double sr, long* dest, long dest_rows,
                           long n0, int* flag, void* stream);
/* The `seen_segment_hashes` loop of scripts/run_eval_probs.py:141-149 over a whole epoch: ids int64 [N] in [0, n_ids),
 * first: int32 [n_ids] filled with INT_MAX by the caller.  Launch 1: atomicMin(&first[ids[i]], i); launch 2: mask[i] =
 * (first[ids[i]] == i), first_row[i] = first[ids[i]].  An id out of range: *flag |= 8, mask 0, first_row -1.  N < 2^31. */
int bm_first_occurrence(const long* ids, long N, long n_ids, int* first, unsigned char* mask, int* first_row,
                        int* flag, void* stream);

/* ---- fused Adam on the flat bucket (adam.hip)  torch.optim.Adam @ bm/train.py:118-119 ---- */
int bm_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, int step,
                 double lr, double beta1, double beta2, double eps, double grad_scale, void* stream);

/* ---- data-parallel collectives: RCCL behind the C-ABI (comm.hip) ----
 * Replace flashy.distrib.init (bm/train.py:139), flashy.distrib.sync_model (bm/solver.py:386: gradient
 * mean = in-place reduce-scatter of the flat gradient bucket + Adam on the shard + in-place all-gather of
 * the parameters; BatchNorm buffers by all-reduce), flashy.distrib.average_metrics (bm/solver.py:395), and
 * add the whole-node candidate all-gather (README.md:139-143 keeps negatives per GPU).  One process per GPU.
 * librccl is dlopen'ed on first use (BM_RCCL_LIB overrides the path).  The opaque handle is the only state
 * the library owns; fp32 buffers; collectives are enqueued on `stream`, never synchronised; NCCL in-place
 * conventions (all-gather: send == recv + rank*count; reduce-scatter: recv == send + rank*count). */
int bm_comm_unique_id_bytes(void);
int bm_comm_available(void);                              /* 0 = librccl loads and has every symbol (local check) */
int bm_comm_unique_id(void* out_id);                       /* rank 0; the host hands the bytes to the others */
int bm_comm_init(const void* id, int world, int rank, int device, void** handle);
int bm_comm_destroy(void* handle);
int bm_comm_world(void* handle);
int bm_comm_rank(void* handle);
int bm_comm_reported_world(void* handle);                 /* ncclCommCount: the size RCCL itself reports (-1: unknown) */
int bm_comm_reported_rank(void* handle);                  /* ncclCommUserRank */
int bm_comm_allgather(void* handle, const float* send, float* recv, long count, void* stream);
int bm_comm_reduce_scatter(void* handle, const float* send, float* recv, long count, void* stream);
int bm_comm_allreduce(void* handle, const float* send, float* recv, long count, int op, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BM_HIP_H */
