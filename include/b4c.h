/*
 * b4c.h -- C ABI of libb4c_hip.so: the MI355X (gfx950) hot path of BERT4ClickPath's
 * BERT4Rec forward / Cloze-training step.
 *
 * The reference (MiladShahidi/BERT4ClickPath, pure Python on TensorFlow 2.3.1) has no
 * native layer; its hot path bottoms out in TF ops.  Each entry point below replaces the
 * TF call sites cited next to it (paths relative to the reference root).  A binding for
 * the reference's own Python is shown in INTEGRATION.md (ctypes).
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory unless named h_*;
 *  - no allocation, no global state, no synchronisation inside: the caller owns every
 *    buffer and passes the hipStream_t (as void*); calls are thread-safe per stream;
 *  - return 0 on success, a negative B4C_E* code otherwise (b4c_last_error() gives text);
 *  - dtype: B4C_F32 = exact fp32 path (parity), B4C_BF16 = bf16 storage / fp32 accumulate
 *    (throughput).  "T" below means that element type.  Weights master copies, biases,
 *    LayerNorm params, statistics, losses and gradients of weights are always fp32;
 *  - ld* are row pitches in ELEMENTS.  Vector paths need pitches and inner sizes that are
 *    multiples of 8 elements; the host pads (zeros) where the model's sizes are not.
 *  - rows * ld may exceed 2^31 elements (and 2^32 bytes) in the row-wise entry points (softmax, the losses on
 *    probabilities and logits, top-k, candidate ranking, row gather / scatter, the embedding stage, the row
 *    forms of Adam) and in C / gate / residual of b4c_gemm_nt, unless one states a limit of its own.  The
 *    operands that the GEMM, attention and vocab_ce kernels stage tile by tile (A, Bt, X, G, h, wt, q | k | v)
 *    are addressed with 32-bit byte offsets inside a tile: keep 128 * ld * element size below 2^30 bytes
 *    (b4c_gemm_nt and b4c_gemm_nt_softmax check it).
 */
#ifndef B4C_H
#define B4C_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define B4C_F32 0
#define B4C_BF16 1
#define B4C_I32 2    /* (b4c_poison_rows only: int32 rows, poisoned with -1) */

#define B4C_OK 0
#define B4C_EINVAL (-1)   /* bad argument (shape / alignment / dtype)              */
#define B4C_ELAUNCH (-2)  /* the HIP runtime refused the launch (see last_error)    */
#define B4C_EUNSUPPORTED (-3)

#define B4C_MAX_FEATURES 4
#define B4C_MAX_TOPK 16
#define B4C_MAX_EXCL 1024   /* longest exclusion list per ranked row (b4c_exclusions_prep and the *_excl entry points) */
#define B4C_MAX_CAND 1024   /* longest candidate list per row (b4c_sample_candidates, b4c_candidate_score, b4c_candidate_rank_rows) */

#define B4C_ACT_NONE 0
#define B4C_ACT_RELU 1
#define B4C_ACT_GELU 2       /* x Phi(x), Phi through erf (Keras / torch default)                    */
#define B4C_ACT_GELU_TANH 3  /* 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) (the BERT4Rec code)  */

#define B4C_CE_TF 0    /* clip[1e-7,1-1e-7] -> log -> log-softmax (tf.keras.backend, TF 2.3.1) */
#define B4C_CE_PLAIN 1 /* -log p_y                                                            */

/* What b4c_abi_version() returns.  Additive entry points (new names, no signature changed) keep it.  13: the contrastive loss,
 * the contrastive views and the long attention were three extension headers with a version and a version getter each
 * (b4c_*_version); they are sections of this header now and the three getters left the library, so a C caller built against an
 * extension header no longer links -- a removal, which is what this number reports.  No signature changed from 12. */
#define B4C_ABI_VERSION 13

int b4c_abi_version(void);
const char *b4c_last_error(void);

/* ---- R6 + R4: embedding stage ------------------------------------------------------
 * replaces transformer.py:376-398 (Embedding per feature -> concat -> * sqrt(d) -> + PE)
 * and create_padding_mask :38-41, plus Encoder.call's input dropout :263.
 *   out[t, off_f + j] = drop( table_f[ids_f[t], j] * scale + pe[s, off_f + j] )
 *   key_pad[t] = (ids_0[t] == 0)
 * h_ids / h_tables / h_dims / h_rows: HOST arrays of n_feat entries (device pointers inside).
 * ids are int64 (B*S); ids outside [0, rows) are clamped.  pe: fp32 [>=S][d_model].
 * The features are concatenated when their dims add up to d_model (the reference, :384-388).  SUMMED FEATURES (no reference
 * counterpart; BASELINE.json configs[3] words the two-feature input as "gather + sum"): n_feat >= 2 and EVERY h_dims[f] ==
 * d_model -- out[t, j] = drop( (sum_f table_f[ids_f[t], j]) * scale + pe[s, j] ), rows added in feature order in fp32, and
 * the backward entry points give every table the gradient of the one d_model-wide row.
 * dropout: keep(e) from the counter hash b4c_keep(seed, e), e = t*d_model + col; rate 0 = off. */
int b4c_embed_concat_pe_fwd(int n_feat, const int64_t *const *h_ids, const float *const *h_tables,
                            const int *h_dims, const int64_t *h_rows, const float *pe, float scale,
                            void *out, int ld_out, uint8_t *key_pad, int B, int S, int d_model,
                            float dropout_rate, uint64_t seed, int dtype, void *stream);

/* gradient of the above w.r.t. the tables (fp32, accumulated with float atomics into
 * h_dtables[f], which the caller zeroes): dtable_f[id, j] += scale * dropmask * dout[t, off_f+j] */
int b4c_embed_concat_pe_bwd(int n_feat, const int64_t *const *h_ids, float *const *h_dtables,
                            const int *h_dims, const int64_t *h_rows, float scale, const void *dout,
                            int ld_dout, int B, int S, int d_model, float dropout_rate, uint64_t seed,
                            int dtype, void *stream);
/* LEARNED POSITIONS (no reference counterpart; the reference's table is the fixed sinusoid): gradient of the embedding stage
 * w.r.t. the positional table `pe` of b4c_embed_concat_pe_fwd / _fwd_packed,
 *   dpe[s][j] += sum over sequences b with cu[b+1] - cu[b] > s of  keep(e) / (1 - rate) * dout[cu[b] + s][j],   s < S,
 * e = (cu[b] + s) * d_model + j: the element index, and so the dropout mask, of the forward pass (and of b4c_embed_concat_pe_bwd).
 * cu int32 [B+1]: row of every sequence's first token in dout -- b * S in the dense layout (pad rows then count: the forward adds
 * pe there too); sequences longer than S contribute their first S rows.  row_of (int32 [B*S], or NULL): when given, the row of
 * position s of sequence b is row_of[b*S + s] (negative: none) and cu is not read -- packed_of of b4c_nonpad_positions, for the
 * packed layout, whose forward takes row t's position from token_src[t] % S: pads need not be at a sequence's end (the Cloze
 * batches keep the closing [SEP] at S - 1).  Rows outside [0, n_rows), n_rows = rows of dout, are skipped.  dpe fp32 [>= S][d_model], ADDED to; rows >= S are not touched.  dout T [.][ld_dout],
 * rows * ld_dout may exceed 2^31.  d_model % 8 == 0, <= 2048.  No float atomics: workgroups sum contiguous blocks of sequences
 * in sequence order into the workspace, and the blocks are added in block order -- the same bits on every launch. */
int64_t b4c_pos_table_bwd_workspace_bytes(int B, int S, int d_model);
int b4c_pos_table_bwd(const void *dout, int ld_dout, int64_t n_rows, const int32_t *cu, const int32_t *row_of, int B, int S,
                      int d_model, float dropout_rate, uint64_t seed, float *dpe, void *workspace, int64_t workspace_bytes,
                      int dtype, void *stream);
/* same, given for every feature the token indices sorted by id (order[f][p], int32, any order among equal ids):
 * runs of one id are summed in registers and written once -- two float atomics per distinct id and wave boundary
 * instead of one per token and column.  The sort is the caller's (one radix sort of B*S keys per feature). */
int b4c_embed_concat_pe_bwd_sorted(int n_feat, const int64_t *const *h_ids, const int32_t *const *h_order,
                                   float *const *h_dtables, const int *h_dims, const int64_t *h_rows, float scale,
                                   const void *dout, int ld_dout, int B, int S, int d_model, float dropout_rate,
                                   uint64_t seed, int dtype, void *stream);
/* (ABI 9) the same with a caller scratch: workspace != NULL selects the DETERMINISTIC form -- runs that cross the 64-entry ranges
 * of the kernel's waves are summed in range order through the scratch instead of meeting through float atomics, so two launches
 * on the same inputs give the same bits.  workspace == NULL: the form above. */
int64_t b4c_embed_concat_pe_bwd_sorted_workspace_bytes(int n_feat, const int *h_dims, int B, int S);
int b4c_embed_concat_pe_bwd_sorted_ws(int n_feat, const int64_t *const *h_ids, const int32_t *const *h_order,
                                      float *const *h_dtables, const int *h_dims, const int64_t *h_rows, float scale,
                                      const void *dout, int ld_dout, int B, int S, int d_model, float dropout_rate,
                                      uint64_t seed, void *workspace, int64_t workspace_bytes, int dtype, void *stream);

/* ---- dense layers (R8 projections, R9 FFN, R12 head) --------------------------------
 * replaces tf.keras.layers.Dense call sites transformer.py:112-116,165-166; head.py:35-36.
 * pack: fp32 Keras kernel [K][N] -> compute copy in T.
 *   transpose=1: dst[n][k] = src[k][n]  (dst is [N][ld_dst], forward operand)
 *   transpose=0: dst[k][n] = src[k][n]  (dst is [K][ld_dst], backward-dX operand)
 * Only the K x N valid elements are written: the caller zero-initialises padded buffers once
 * (pad rows / columns never change afterwards). */
int b4c_pack_weight(const float *src, int K, int N, void *dst, int ld_dst, int transpose, int dtype,
                    void *stream);

/* All layers' compute copies in one launch.  One descriptor per Keras kernel; fused layers (Q|K|V) use
 * several descriptors writing at different col_off of the same wt / wc / bias buffers.
 *   wt[(col_off + n)][k]  (pitch ld_t)   = src[k][n]      forward operand, may be NULL
 *   wc[k][col_off + n]    (pitch ld_c)   = src[k][n]      backward-dX operand, may be NULL
 *   bias_dst[col_off + n]                = bias_src[n]    fp32, may be NULL
 * d_desc is a DEVICE array; max_tiles = max over descriptors of ceil(K/32)*ceil(N/32). */
typedef struct {
    const float *src;
    const float *bias_src;
    void *wt;
    void *wc;
    float *bias_dst;
    int32_t K, N, ld_t, ld_c, col_off, _pad;
} b4c_pack_desc;
int b4c_pack_weights_batched(const b4c_pack_desc *d_desc, int n_desc, int max_tiles, int dtype, void *stream);
/* (max_tiles: the largest ceil(K / 64) * ceil(N / 64) over the descriptors -- the launch is max_tiles x n_desc workgroups) */

/* C[M][N] = epilogue( A[M][K] . Bt[N][K]^T )     (both operands K-contiguous)
 *   v = acc + bias[n]            (bias fp32 or NULL)
 *   v = relu(v)                  if act == B4C_ACT_RELU;   v = gelu(v) if act == B4C_ACT_GELU / B4C_ACT_GELU_TANH (fp32)
 *   v = v * (gate[m][n] > 0)     if gate != NULL   (ReLU backward: gate = saved activation, pitch ldg)
 *   v = v + residual[m][n]       if residual != NULL (T, pitch ldr)
 * out_dtype chooses C's element type (T of `dtype`, or B4C_F32 for fp32 logits from bf16 inputs).
 * K % 8 == 0, lda/ldb % 8 == 0 (bf16) or % 4 (fp32).  LIMIT: A and Bt are staged tile by tile through a buffer
 * descriptor of less than 2^30 bytes, so 128 * lda and 128 * ldb elements must span less than 2^30 bytes
 * (B4C_EINVAL otherwise; b4c_gemm_nt_softmax alike).  M * ldc -- C, gate and residual -- may exceed 2^31 elements. */
int b4c_gemm_nt(const void *A, int lda, const void *Bt, int ldb, void *C, int ldc, int M, int N, int K,
                const float *bias, int act, const void *gate, int ldg, const void *residual, int ldr,
                int dtype, int out_dtype, void *stream);
/* b4c_gemm_nt with two more operands (no reference counterpart: the GELU feed-forward block of the BERT4Rec paper):
 *   pre [M][ldp] (T, or NULL): the pre-activation u = acc + bias is written as well -- what the backward of a GELU needs, which
 *     cannot be recovered from gelu(u).  Bit-identical to C of b4c_gemm_nt(..., act = B4C_ACT_NONE) with out_dtype == dtype on
 *     the same operands (N < 2048 or K > 128: the wide-N route of the plain launch rounds on its own); C is the same with or
 *     without it.  M * ldp may exceed 2^31 elements.
 *   gate_act: how `gate` is applied.  B4C_ACT_RELU: v * (gate > 0), as b4c_gemm_nt.  B4C_ACT_GELU / B4C_ACT_GELU_TANH:
 *     v * act'(gate), gate = the saved pre-activation u; the derivative is evaluated in fp32 (erf: Phi(u) + u phi(u)). */
int b4c_gemm_nt_act(const void *A, int lda, const void *Bt, int ldb, void *C, int ldc, int M, int N, int K,
                    const float *bias, int act, const void *gate, int ldg, int gate_act, const void *residual, int ldr,
                    void *pre, int ldp, int dtype, int out_dtype, void *stream);

/* R9/R10 fused with the GEMM that feeds them (bf16, N <= 256; N > 128 runs 64-row x 256-column workgroups):
 *   y = A . Bt^T + bias;  z = x + dropout(y);  out = LayerNorm(z) * gamma + beta;  stats = (mean, rstd)
 * == b4c_gemm_nt followed by b4c_add_dropout_layernorm_fwd, bit for bit, without y in HBM.
 * z / out [M][N] bf16 (pitch N), stats [M][2] fp32, x pitch ldx. */
int b4c_gemm_nt_add_ln(const void *A, int lda, const void *Bt, int ldb, const float *bias, const void *x, int ldx,
                       const float *gamma, const float *beta, void *z, void *out, float *stats, int M, int N, int K,
                       float eps, float dropout_rate, uint64_t seed, int dtype, void *stream);

/* dW[K][N] += A[M][K]^T . G[M][N]   and  db[N] += colsum(G)   (fp32 outputs ADDED to what is there: the
 * caller zeroes or accumulates; db may be NULL).  The reduction over the M (token) axis is split over
 * workgroups when the output has few 128x128 tiles; the partial tiles are then summed
 *   - through `workspace` (device memory, 16-B aligned, >= b4c_gemm_tn_workspace_bytes(M,K,N,dtype)) in a
 *     fixed order: deterministic, no atomics.  The workspace is scratch: it may be shared by every call on
 *     the same stream;
 *   - with float atomics if workspace is NULL or too small (order-dependent rounding). */
int64_t b4c_gemm_tn_workspace_bytes(int M, int K, int N, int dtype);
int b4c_gemm_tn(const void *A, int lda, const void *G, int ldg, float *dW, int ldw, float *db, int M, int K,
                int N, int dtype, void *workspace, int64_t workspace_bytes, void *stream);
/* same with N = n_seg * seg_width cut into n_seg (<= 4) column segments, each accumulated into its own
 * dW_i [K][seg_width] / db_i [seg_width] (HOST arrays of device pointers): the fused Q|K|V projection
 * adds straight into the three gradient tensors. */
int b4c_gemm_tn_seg(const void *A, int lda, const void *G, int ldg, int n_seg, float *const *h_dW,
                    float *const *h_db, int seg_width, int M, int K, int dtype, void *workspace,
                    int64_t workspace_bytes, void *stream);

/* (ABI 9) the whole backward of one Dense layer of the encoder in ONE pass over its output gradient (transformer.py:112-116,
 * 158, 163-167 seen from the backward pass):   dX = G Wc^T (+ residual)   dW_s += X^T G_s   db_s += colsum(G_s)
 * X [M][128] the layer's input, G [M][128 n_seg] (n_seg = 3: q | k | v column blocks, 2: k | v, 1: a plain layer), Wc [128][128 n_seg]
 * (row = input feature, the dX operand of b4c_gemm_nt), residual [M][128] or NULL, dX [M][128]; dW_s fp32 [128][ld_dw] Keras
 * layout, db_s fp32 [128] or NULL (h_dW / h_db: HOST arrays of n_seg device pointers).  bf16, 128-wide layers only; G is read from
 * HBM once (as b4c_gemm_nt + b4c_gemm_tn it is read twice).  Deterministic: per-workgroup partial sums meet in workgroup order
 * through the caller's scratch. */
int64_t b4c_gemm_dxdw_workspace_bytes(int64_t M, int n_seg);
int b4c_gemm_dxdw(const void *X, int ldx, const void *G, int ldg, const void *Wc, int ldw, const void *residual, int ldr,
                  void *dX, int ldo, int n_seg, float *const *h_dW, float *const *h_db, int ld_dw, int64_t M,
                  void *workspace, int64_t workspace_bytes, void *stream);

/* (ABI 10) the whole backward of the position-wise feed-forward block of one encoder layer (transformer.py:154-170 seen from the
 * backward pass: LayerNormalization, dropout, residual add, Dense(d_model), Dense(dff, relu)) in ONE pass:
 *   dz, dy   = LayerNorm / dropout backward of dout (as b4c_add_dropout_layernorm_bwd: z [M][128] the saved LayerNorm input,
 *              stats [M][2], gamma [128]; dropout_rate / seed of the forward pass's mask)          -- never written to HBM
 *   dW2 += H^T dy,  db2 += colsum(dy),  dh = (dy W2c^T) o [H > 0]                                  -- dh never written to HBM
 *   dW1 += X^T dh,  db1 += colsum(dh),  dX = dh W1c^T + dz,   dgamma / dbeta += the LayerNorm's parameter gradients
 * H [M][ldh] = relu(X W1 + b1) with Fp stored columns (F valid, Fp = F rounded up to 8, <= 128), X [M][ldx] (128 columns),
 * W2c [Fp][ldw2] (row = hidden column, 128 entries) and W1c [128][ldw1] (row = input feature, Fp entries): the dX operands of
 * b4c_gemm_nt for the two layers.  dW1 fp32 [128][ld_dw1], dW2 fp32 [F][ld_dw2] (Keras layouts), db1 [F] / db2 [128] or NULL.
 * bf16, d_model = 128 only.  Reads dout, z, H, X once and writes dX: 1,240 B per token against 3,340 for the five kernels it
 * replaces.  Deterministic (no float atomics: per-workgroup partial sums meet in a fixed order through the caller's scratch). */
int64_t b4c_ffn_bwd_workspace_bytes(int64_t M);
int b4c_ffn_bwd(const void *dout, const void *z, const float *stats, const float *gamma, float dropout_rate, uint64_t seed,
                const void *H, int ldh, const void *X, int ldx, const void *W2c, int ldw2, const void *W1c, int ldw1,
                int F, int Fp, void *dX, int ldo, float *dW1, int ld_dw1, float *db1, float *dW2, int ld_dw2, float *db2,
                float *dgamma, float *dbeta, int64_t M, void *workspace, int64_t workspace_bytes, void *stream);

/* (ABI 11) the backward of the attention block's tail (transformer.py:158-162, 204-207 seen from the backward pass: LayerNormalization,
 * dropout, residual add, the output projection Dense(d_model)) in ONE pass:
 *   dz, dy = LayerNorm / dropout backward of dout (z, stats, gamma, dropout_rate, seed as b4c_add_dropout_layernorm_bwd);
 *   dZ [M][128] = dz (the residual branch's gradient: the caller adds it to the block input's gradient);   dy never reaches HBM;
 *   dO [M][ld_do] = dy Wc^T,   dW += O^T dy,   db += colsum(dy),   dgamma / dbeta += the LayerNorm's parameter gradients.
 * O [M][ldo_in] the projection's input (128 columns), Wc [128][ldw] (row = input feature of the projection: the dX operand of
 * b4c_gemm_nt), dW fp32 [128][ld_dw] Keras layout, db fp32 [128] or NULL.  bf16, d_model = 128 only.  1,288 B per token against 1,800 for
 * b4c_add_dropout_layernorm_bwd + b4c_gemm_dxdw.  Deterministic (fixed-order reduction through the caller's scratch). */
int64_t b4c_attn_out_bwd_workspace_bytes(int64_t M);
int b4c_attn_out_bwd(const void *dout, const void *z, const float *stats, const float *gamma, float dropout_rate, uint64_t seed,
                     const void *O, int ldo_in, const void *Wc, int ldw, void *dZ, void *dO, int ld_do,
                     float *dW, int ld_dw, float *db, float *dgamma, float *dbeta, int64_t M,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* (ABI 12) the forward of the position-wise feed-forward block (transformer.py:154-170) in ONE pass:
 *   H = relu(X W1 + b1) [M][ldh] (Fp stored columns, F valid; the backward pass reads it),   Z = X + dropout(H W2 + b2) (or NULL),
 *   Out = LayerNorm(Z) gamma + beta,   stats [M][2] = (mean, 1 / std) of Z's rows (or NULL).
 * W1t [Fp][ldw1] (row = hidden column, 128 entries) and W2t [128][ldw2] (row = output column, Fp entries): the forward operands of
 * b4c_gemm_nt for the two layers; b1 [Fp], b2 / gamma / beta [128] fp32.  bf16, d_model = 128, F <= 128 only.  X is read once and H is
 * not read back: 446 MB per launch at 456 k rows against 658 for b4c_gemm_nt + b4c_gemm_nt_add_ln. */
int b4c_ffn_fwd(const void *X, int ldx, const void *W1t, int ldw1, const float *b1, const void *W2t, int ldw2, const float *b2,
                const float *gamma, const float *beta, int F, int Fp, void *H, int ldh, void *Z, void *Out, float *stats,
                int64_t M, float eps, float dropout_rate, uint64_t seed, void *stream);

/* (ABI 12, additive) b4c_ffn_fwd / b4c_ffn_bwd for a feed-forward block with a GELU activation: act = B4C_ACT_GELU or
 * B4C_ACT_GELU_TANH, anything else is refused (B4C_ACT_RELU is b4c_ffn_fwd / b4c_ffn_bwd).  Every other argument, the shapes they
 * take (bf16, d_model = 128, F <= 128; backward 2 <= M < 2^24) and the accumulate-into-gradients contract are those of the ReLU pair.
 * Both round where b4c_gemm_nt_act's bf16 epilogue rounds (the fp32 sum to bf16, the rest in fp32, the result to bf16), so that a
 * model computes the same step on either route, up to the order of the fp32 sums.
 * Forward:   u = bf16(X W1) + b1;   H = bf16(act(u)) [M][ldh],   U = bf16(u) [M][ldu] (Fp stored columns each): C and `pre` of
 *   b4c_gemm_nt_act;   Z, Out, stats those of b4c_gemm_nt_add_ln (y = bf16(bf16(H W2) + b2)).  U is required when Z is given (a training call: GELU is not monotone, the
 *   backward pass gates with act'(u)) and may be NULL at inference (Z NULL), which then writes neither.
 * Backward:  dh = bf16(bf16(dy W2c^T) * act'(U)): C of b4c_gemm_nt_act(gate = U, gate_act = act);   dW2 += H^T dy as before: it
 *   reads both H and U, 1,240 + 2 Fp B per token.  Memory past a row's Fp columns of H or U (a pitch above Fp) is never used,
 *   whatever it holds.  workspace: b4c_ffn_bwd_workspace_bytes(M). */
int b4c_ffn_act_fwd(const void *X, int ldx, const void *W1t, int ldw1, const float *b1, const void *W2t, int ldw2,
                    const float *b2, const float *gamma, const float *beta, int F, int Fp, int act, void *H, int ldh,
                    void *U, int ldu, void *Z, void *Out, float *stats, int64_t M, float eps, float dropout_rate,
                    uint64_t seed, void *stream);
int b4c_ffn_act_bwd(const void *dout, const void *z, const float *stats, const float *gamma, float dropout_rate, uint64_t seed,
                    int act, const void *H, int ldh, const void *U, int ldu, const void *X, int ldx, const void *W2c, int ldw2,
                    const void *W1c, int ldw1, int F, int Fp, void *dX, int ldo, float *dW1, int ld_dw1, float *db1,
                    float *dW2, int ld_dw2, float *db2, float *dgamma, float *dbeta, int64_t M, void *workspace,
                    int64_t workspace_bytes, void *stream);

/* several dW problems over the SAME M tokens in one launch (bf16; the four weight gradients of an encoder layer):
 * the ~256 workgroups of the split are shared by all problems, so every output tile has ~256 / (total tiles)
 * partial sums, and the group needs one main + one reduce kernel.  Problem i: dW_i[K][n_seg * seg_width] split into
 * n_seg column segments as b4c_gemm_tn_seg.  h_desc is a HOST array.  Always deterministic (workspace required). */
typedef struct {
    const void *A;          /* [M][lda], K columns used */
    const void *G;          /* [M][ldg], n_seg * seg_width columns used */
    float *dW[4];           /* device pointers, [K][ldw] each */
    float *db[4];           /* all n_seg of them, or db[0] NULL: no column sums for this problem */
    int32_t lda, ldg, K, n_seg, seg_width, ldw;
} b4c_tn_desc;
int64_t b4c_gemm_tn_group_workspace_bytes(const b4c_tn_desc *h_desc, int n_prob, int M);
int b4c_gemm_tn_group(const b4c_tn_desc *h_desc, int n_prob, int M, int dtype, void *workspace, int64_t workspace_bytes,
                      void *stream);

/* ---- R8: attention -------------------------------------------------------------------
 * replaces MultiHeadAttention.split_heads + scaled_dot_product_attention + merge
 * (transformer.py:64-97, 130-156).  qkv: [B*S][ld_qkv] with q | k | v column blocks of d_model
 * each (head h = columns h*dh..), key_pad [B*S] from the embedding stage (key-side mask, -1e9).
 *   o[B*S][ld_o] = softmax(q k^T / sqrt(dh) + pad * -1e9) v   (heads merged)
 *   lse[B][H][S] = log-sum-exp of the masked, scaled logits (saved for backward) */
int b4c_attn_fwd(const void *qkv, int ld_qkv, const uint8_t *key_pad, void *o, int ld_o, float *lse, int B,
                 int S, int H, int dh, int dtype, void *stream);
/* dqkv [B*S][ld_dqkv] from do; delta[B][H][S] is scratch (fp32): the row kernels keep rowsum(dO o O) there, the
 * bf16 MFMA kernel computes it in LDS and uses the first word as the work counter of its persistent grid. */
int b4c_attn_bwd(const void *qkv, int ld_qkv, const uint8_t *key_pad, const void *o, int ld_o,
                 const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv, int B,
                 int S, int H, int dh, int dtype, void *stream);

/* same with a caller-provided scratch: bf16 sequences of 256 < S <= 512 run the MFMA backward block by block of 256 keys
 * (one launch) and sum the partial dQ in an fp32 accumulator of b4c_attn_bwd_workspace_bytes(B, S, H, dh, dtype) bytes (0 when no
 * workspace is needed).  Without it those shapes fall back to the fp32-math row kernels (a notice is printed once). */
int64_t b4c_attn_bwd_workspace_bytes(int B, int S, int H, int dh, int dtype);
int b4c_attn_bwd_ws(const void *qkv, int ld_qkv, const uint8_t *key_pad, const void *o, int ld_o,
                    const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv, int B,
                    int S, int H, int dh, void *workspace, int64_t workspace_bytes, int dtype, void *stream);

/* ---- R10: residual + dropout + LayerNorm ---------------------------------------------
 * replaces EncoderLayer.call's  LN(x + dropout(y))  (transformer.py:204-206, 209-211),
 * LayerNormalization(epsilon) :183-184 (biased variance, eps inside rsqrt).
 *   z = x + drop(y);  out = (z - mean) * rstd * gamma + beta;  stats[row] = {mean, rstd}
 * z (T, pitch d) is saved for backward; d % 8 == 0. */
int b4c_add_dropout_layernorm_fwd(const void *x, const void *y, const float *gamma, const float *beta,
                                  void *z, void *out, float *stats, int64_t rows, int d, float eps,
                                  float dropout_rate, uint64_t seed, int dtype, void *stream);
/* dz -> residual branch; dy = dropmask * dz (written only if dropout_rate > 0, else may be NULL);
 * dgamma/dbeta fp32 [d], accumulated with atomics (caller zeroes). */
int b4c_add_dropout_layernorm_bwd(const void *dout, const void *z, const float *stats, const float *gamma,
                                  void *dz, void *dy, float *dgamma, float *dbeta, int64_t rows, int d,
                                  float dropout_rate, uint64_t seed, int dtype, void *stream);
/* (ABI 9) the same with a caller scratch (b4c_add_dropout_layernorm_bwd_workspace_bytes): workspace != NULL selects the
 * DETERMINISTIC form of dgamma / dbeta -- per-workgroup sums in a fixed order, added block by block -- instead of float atomics. */
int64_t b4c_add_dropout_layernorm_bwd_workspace_bytes(int64_t rows, int d);
int b4c_add_dropout_layernorm_bwd_ws(const void *dout, const void *z, const float *stats, const float *gamma,
                                     void *dz, void *dy, float *dgamma, float *dbeta, int64_t rows, int d,
                                     float dropout_rate, uint64_t seed, void *workspace, int64_t workspace_bytes, int dtype,
                                     void *stream);

/* PLAIN LAYERNORM over rows (no reference counterpart: the transform of the paper's masked-item head, head.py `transform`):
 *   out = (x - mean) * rstd * gamma + beta;  stats[row] = {mean, rstd}   (biased variance, eps inside the root)
 * no residual, no dropout; x, out `dtype` [rows][d], d % 8 == 0, d <= 1024; the row body of b4c_add_dropout_layernorm_fwd.
 * b4c_layernorm_bwd: dx = rstd * (a - mean_j(a) - xhat * mean_j(a * xhat)), a = dout * gamma, xhat from the saved stats;
 *   dgamma += sum_rows dout * xhat, dbeta += sum_rows dout (fp32 [d], ADDED to) through per-workgroup sums in the workspace
 *   (b4c_layernorm_bwd_workspace_bytes, required) added in a fixed order: no float atomics, the same bits on every launch.
 *   gate (or NULL): dx is multiplied by act'(gate[row][j]) (pitch ld_gate) before it is stored -- the activation in FRONT of
 *   the norm: gate_act B4C_ACT_RELU = (gate > 0), gate = the activation or its pre-activation; a GELU = its derivative at the
 *   saved pre-activation (the `pre` output of b4c_gemm_nt_act), evaluated in fp32 as b4c_gemm_nt_act's gate is. */
int b4c_layernorm_fwd(const void *x, const float *gamma, const float *beta, void *out, float *stats, int64_t rows, int d,
                      float eps, int dtype, void *stream);
int64_t b4c_layernorm_bwd_workspace_bytes(int64_t rows, int d);
int b4c_layernorm_bwd(const void *dout, const void *x, const float *stats, const float *gamma, void *dx, float *dgamma,
                      float *dbeta, int64_t rows, int d, const void *gate, int ld_gate, int gate_act, void *workspace,
                      int64_t workspace_bytes, int dtype, void *stream);

/* ---- R11: [MASK]-position index generation and row gather -----------------------------
 * replaces _gather_output_by_raw_value (clickstream_transformer.py:260-297):
 * tf.where(raw == value) row-major, ragged per batch row, gather_nd, to_tensor(0).
 * counts[B], offsets[B+1] (exclusive scan; offsets[B] = R), flat_idx[cap] = b*S+s in row-major
 * order (entries >= R untouched), maxcount[1].  All int32 except ids (int64).
 * More matches than `cap` (a caller-limited row count, e.g. B x max_masked_per_row of the sync-free Cloze path): the
 * offsets are clamped to cap -- consumers that size their row tensors by cap never index past them -- maxcount[0] comes
 * back as -(longest row) - 1 (negative even when that is 0) and `poison` (optional int32 flag) is set to -1, for the caller to
 * fold into the loss as NaN. */
int b4c_mask_positions(const int64_t *ids, int B, int S, int64_t value, int32_t *counts, int32_t *offsets,
                       int32_t *flat_idx, int32_t cap, int32_t *maxcount, int32_t *poison, void *stream);
/* padded_idx[B*M] = flat index of the m-th match of row b, or -1 (pad slot). */
int b4c_padded_index(const int32_t *counts, const int32_t *offsets, const int32_t *flat_idx, int B, int M,
                     int32_t *padded_idx, void *stream);
/* out[r][:] = idx[r] >= 0 ? in[idx[r]][:] : 0      (width % 8 == 0) */
int b4c_gather_rows(const void *in, int ld_in, const int32_t *idx, void *out, int ld_out, int64_t n_out,
                    int width, int dtype, void *stream);
/* dst (n_dst rows) = 0, then dst[idx[r]][:] = src[r][:] for idx[r] >= 0 (indices unique). */
int b4c_scatter_rows(const void *src, int ld_src, const int32_t *idx, void *dst, int ld_dst, int64_t n_src,
                     int64_t n_dst, int width, int dtype, void *stream);

/* ---- R12 tail, R13, R14: softmax, masked sparse cross-entropy --------------------------
 * replaces Dense(V, softmax)'s activation (head.py:36), cloze_output_adaptor + MaskedLoss with
 * tf.keras.backend.sparse_categorical_crossentropy (utils.py:56-134, losses.py:31-98, main.py:89).
 * probs[r][0..V) = softmax(logits[r][0..V)); pad columns V..ld are written 0. */
int b4c_softmax_rows(const void *logits, int ld_in, void *probs, int ld_out, int64_t R, int V, int dtype,
                     void *stream);
/* per-row loss on PROBABILITIES (the reference's dataflow): labels fp32 as the reference keeps
 * them (-1 = pad -> loss 0, not counted).  item_loss[R], n_valid[1] (+= count). */
int b4c_sparse_ce_from_probs(const void *probs, int ld, const float *labels, float *item_loss,
                             float *n_valid, int64_t R, int V, int variant, int dtype, void *stream);
/* fused training form: logits -> per-row loss and, IN PLACE, dlogits = grad_scale[0] * d loss/d logits
 * (grad_scale is a device scalar, e.g. 1/R_valid).  labels int32 label-space ids; label < 0 or >= V
 * -> row ignored (zero gradient).  pad columns get 0. */
int b4c_softmax_ce_fwd_bwd(void *logits, int ld, const int32_t *labels, float *item_loss,
                           const float *grad_scale, int64_t R, int V, int variant, int dtype, void *stream);

/* ---- R12-R14 without the logits in HBM (bf16 training path) -------------------------------
 * replaces, for training, Dense(V, softmax) (head.py:36) + cloze_output_adaptor + MaskedLoss +
 * sparse_categorical_crossentropy (utils.py:56-134, losses.py:31-98, main.py:89) AND their backward:
 * the (R x V) logits are recomputed tile by tile in MFMA accumulators instead of being stored.
 *   h [R][ld_h] bf16 (head input), wt [V][ld_w] bf16 (vocabulary-major projection weights, K columns),
 *   bias [V] fp32 or NULL, labels [R] int32 (< 0: ignored row), grad_scale: device scalar d total / d row loss.
 * b4c_vocab_ce_fwd:  item_loss[R], dh [R][ld_dh] bf16 = grad_scale * d row_loss / d h, rowscal [R][8] fp32
 *   (scratch handed to b4c_vocab_ce_dw); workspace >= b4c_vocab_ce_workspace_bytes(R, V, K), 16-B aligned.
 * b4c_vocab_ce_dw:   dW [K][ldw] fp32 += d loss / d kernel (Keras layout [in][out]), db [V] += (or NULL);
 *   same workspace (scratch, contents not carried over).
 * K in {64, 128}; variant B4C_CE_TF (clip-renormalised, as the TF backend) or B4C_CE_PLAIN. */
int64_t b4c_vocab_ce_workspace_bytes(int64_t R, int V, int K);
int b4c_vocab_ce_fwd(const void *h, int ld_h, const void *wt, int ld_w, const float *bias, const int32_t *labels,
                     const float *grad_scale, float *item_loss, void *dh, int ld_dh, float *rowscal,
                     void *workspace, int64_t workspace_bytes, int64_t R, int V, int K, int variant, void *stream);
int b4c_vocab_ce_dw(const void *h, int ld_h, const void *wt, int ld_w, const float *bias, const int32_t *labels,
                    const float *rowscal, float *dW, int ldw, float *db, void *workspace, int64_t workspace_bytes,
                    int64_t R, int V, int K, int deterministic, void *stream);
/* (ABI version 8) `deterministic` != 0 (b4c_vocab_ce_dw and its pieces): dW / db are summed in a fixed order, without float
 * atomics -- the same bits on every run of the same inputs.  b4c_vocab_ce_dw keeps the sweep's token split: split 0 adds into
 * dW / db, the later splits store partial sums in the workspace and one pass adds them in split order (a workspace of
 * b4c_vocab_ce_dw_workspace_bytes(R, V, K, 1) holds them; a smaller one, at least b4c_vocab_ce_workspace_bytes, costs the
 * sweep splits); b4c_vocab_ce_dw_sweep (no workspace) has one workgroup per vocabulary tile walk every token.  The label
 * term goes through a stable sort of the rows by label, summed in chunks of 32 sorted rows whose shares of a run are then
 * added in chunk order. */
int64_t b4c_vocab_ce_dw_workspace_bytes(int64_t R, int V, int K, int deterministic);
/* (ABI version 5) b4c_vocab_ce_dw in pieces, so that the sweep can run BESIDE the HBM-bound encoder backward:
 * b4c_vocab_ce_dw_sweep adds the dlogit part of dW / db for the 128-id vocabulary tiles [tile_begin, tile_end) only
 * (tiles own disjoint columns of dW: any partition of [0, ceil(V / 128)) over any number of calls gives the full sweep);
 * background_workgroups > 0 launches it as a background kernel -- at most that many 256-thread workgroups (one wave per
 * SIMD, 220 registers) that walk the units, leaving the rest of every CU's registers and issue slots to the kernels of
 * another stream -- 0 launches the foreground form of b4c_vocab_ce_dw.  b4c_vocab_ce_dw_labels adds the label term
 * (dW[:, y] -= yd h_row, db[y] -= yd) once; workspace >= V * K * 4 bytes.  Sweep + labels == b4c_vocab_ce_dw. */
int b4c_vocab_ce_dw_sweep(const void *h, int ld_h, const void *wt, int ld_w, const float *bias, const float *rowscal,
                          float *dW, int ldw, float *db, int64_t R, int V, int K, int tile_begin, int tile_end,
                          int background_workgroups, int deterministic, void *stream);
int b4c_vocab_ce_dw_labels(const void *h, int ld_h, const int32_t *labels, const float *rowscal, float *dW, int ldw,
                           float *db, void *workspace, int64_t workspace_bytes, int64_t R, int V, int K, int deterministic,
                           void *stream);
/* ---- (ABI version 4) R12 for scoring: Dense(V, softmax) (head.py:36) with ONE pass over the (R x V) tensor ------------------
 * replaces the materialised projection + softmax (b4c_gemm_nt + b4c_softmax_rows: write, read, write) of the
 * bf16 path: b4c_vocab_lse recomputes the logits in MFMA accumulators (nothing reaches HBM) and leaves
 * lse2[row] = log2 sum_j 2^(x_j log2 e); b4c_gemm_nt_softmax then writes probs [R][ldc] bf16 =
 * 2^((h wt^T + bias) log2 e - lse2[row]) straight from its accumulators.  K in {64, 128} (lse) / K <= 128 (projection),
 * N and ldc multiples of 8, operands 16-B aligned; workspace >= b4c_vocab_ce_workspace_bytes(R, V, K). */
int b4c_vocab_lse(const void *h, int ld_h, const void *wt, int ld_w, const float *bias, float *lse2, void *workspace,
                  int64_t workspace_bytes, int64_t R, int V, int K, void *stream);
int b4c_gemm_nt_softmax(const void *A, int lda, const void *Bt, int ldb, void *C, int ldc, int M, int N, int K,
                        const float *bias, const float *lse2, void *stream);

/* ---- (ABI version 8) R15 without the (R x V) scores in memory: ranking over the vocabulary for the bf16 scoring path -----
 * replaces tf.math.top_k + the Recall / NDCG bookkeeping (utils.py:161-190, 225-255) on MATERIALISED probabilities
 * (b4c_gemm_nt_softmax + b4c_topk_rows: 4.1 GB written and read back at C2) by sweeps that keep the logits tile in MFMA
 * accumulators.  Softmax is monotone: the logits rank as the probabilities do.  h [R][ld_h] bf16 (trunk output), wt
 * [>= V][ld_w] bf16 vocabulary-major, bias fp32 [V] or NULL, K in {64, 128}; workspace >= b4c_vocab_rank_workspace_bytes.
 * Scores are formed as b4c_gemm_nt forms them (sum over k from zero, bias last).
 *   b4c_vocab_rank: rank[r] = number of items ranked before the label y_r = #{j : x_j > x_y} + #{j < y : x_j == x_y}
 *     (ties -> lower index first, as tf.math.top_k); negative for rows without a valid label (y < 0 or y >= V).
 *     HitRate@k = [rank < k], NDCG@k = [rank < k] / log2(rank + 2) for every k: b4c_rank_metrics.
 *   b4c_vocab_topk: idx [R][k] int32 = the k best item ids in order (k <= B4C_MAX_TOPK), optional hit / ndcg [R] of `labels`.
 *     Rows with more than 128 candidates at the selection threshold (mass ties) get ids -1 (hit / ndcg NaN) and are counted
 *     in overflow[0]: the caller ranks those rows on materialised scores (b4c_gemm_nt + b4c_topk_rows). */
int64_t b4c_vocab_rank_workspace_bytes(int64_t R, int V, int K);
int b4c_vocab_rank(const void *h, int ld_h, const void *wt, int ld_w, const float *bias, const int32_t *labels, int32_t *rank,
                   void *workspace, int64_t workspace_bytes, int64_t R, int V, int K, void *stream);
int b4c_rank_metrics(const int32_t *rank, int64_t R, int k, float *hit, float *ndcg, void *stream);
int b4c_vocab_topk(const void *h, int ld_h, const void *wt, int ld_w, const float *bias, int k, int32_t *idx,
                   const int32_t *labels, float *hit, float *ndcg, int32_t *overflow, void *workspace,
                   int64_t workspace_bytes, int64_t R, int V, int K, void *stream);

/* ---- (ABI version 4) scalar bookkeeping of the masked mean (losses.py:80-98) and of the head's backward, fused:
 * b4c_label_scale: out[0] = 1 / n_valid (0 if none), out[1] = n_valid, valid = 0 <= label < V (the mask of losses.py:80).
 * b4c_sum_scaled:  out[0] = scale[0] * sum item[0..R) in a fixed order; NaN if poison != NULL and poison[0] < 0.
 * b4c_vocab_ce_apply_grad: folds the upstream gradient g (device scalar) into what b4c_vocab_ce_fwd left for the
 *   backward: dh_out = g * dh, rowscal_out = rowscal with its gradient-linear columns times g.
 * b4c_relu_gate:   out = act > 0 ? g : 0 (n elements, a multiple of 8): relu'(Dense) of head.py:35 on a gradient. */
int b4c_label_scale(const int32_t *labels, int64_t R, int V, float *out, void *stream);
int b4c_sum_scaled(const float *item, int64_t R, const float *scale, const int32_t *poison, float *out, void *stream);
int b4c_vocab_ce_apply_grad(const void *dh, int ld, const float *rowscal, const float *g, void *dh_out, int ld_out,
                            float *rowscal_out, int64_t R, int K, void *stream);
int b4c_relu_gate(const void *g, const void *act, void *out, int64_t n, int dtype, void *stream);

/* ---- R15: top-k ids, HitRate@k / NDCG@k -------------------------------------------------
 * replaces tf.math.top_k + the Recall / NDCG update_state arithmetic (utils.py:161-190, 225-255).
 * topk_idx[R][k] int32, largest first, ties -> lower index.  labels (int32, may be NULL):
 * hit[r] = any(topk == label), ndcg[r] = sum_k (topk[k]==label) / log2(k+2). */
int b4c_topk_rows(const void *scores, int ld, int64_t R, int V, int k, int32_t *topk_idx,
                  const int32_t *labels, float *hit, float *ndcg, int dtype, void *stream);

/* same with a scratch int32 [R] (`redo`): rows are first handled by a threshold-selection kernel that reads each row
 * from HBM once (per-thread maxima -> k-th best of them -> the ~k candidates not worse than it -> ordered pick);
 * rows with more than 1024 candidates (massive ties) are flagged there and redone by the list kernel.  Same results. */
int b4c_topk_rows_ws(const void *scores, int ld, int64_t R, int V, int k, int32_t *topk_idx,
                     const int32_t *labels, float *hit, float *ndcg, int32_t *redo, int dtype, void *stream);

/* ---- exclusions: rank / top-k over the items NOT in a per-row list (filtered evaluation, "not seen yet" serving) ----------
 * A list belongs to one ranked row and holds item ids of the label space.  An excluded item is absent from that row's ranking:
 * it is never among the ids and never counts before the label; every other item keeps its order (score descending, ties ->
 * lower index) and its score (nothing is renormalised).  Fewer than k items left: the tail ids are -1.  The label itself is
 * never excluded.
 * b4c_exclusions_prep: ex_in [R][ld_in] int32, any ids (out of range, negative, duplicate: ignored) -> ex_out [R][E] in the
 *   canonical form every *_excl entry point takes (and does not check again): the ids of [0, V) other than labels[r] (labels
 *   may be NULL), ascending, no duplicates, then -1.  E <= B4C_MAX_EXCL (one workgroup per row, sorted in LDS).
 * b4c_vocab_rank_excl / b4c_vocab_topk_excl: b4c_vocab_rank / b4c_vocab_topk of the excluded scores; the lists act inside the
 *   sweeps (an excluded entry reaches neither a class maximum nor the candidates nor the count), so the threshold is that of
 *   the items that remain.  Rows with mass ties are still handed back with ids -1 and counted in overflow[0].
 * b4c_topk_rows_excl: b4c_topk_rows_ws on materialised scores (fp32 probabilities / logits, bf16) with the lists; `scores` is
 *   only read.  redo may be NULL (per-thread-list kernel for every row).
 * E == 0: the entry points without exclusions, unchanged. */
int b4c_exclusions_prep(const int32_t *ex_in, int ld_in, int64_t R, int E, int V, const int32_t *labels, int32_t *ex_out, void *stream);
int b4c_vocab_rank_excl(const void *h, int ld_h, const void *wt, int ld_w, const float *bias, const int32_t *labels, int32_t *rank,
                        void *workspace, int64_t workspace_bytes, int64_t R, int V, int K, const int32_t *excl, int ld_e, int E,
                        void *stream);
int b4c_vocab_topk_excl(const void *h, int ld_h, const void *wt, int ld_w, const float *bias, int k, int32_t *idx,
                        const int32_t *labels, float *hit, float *ndcg, int32_t *overflow, void *workspace, int64_t workspace_bytes,
                        int64_t R, int V, int K, const int32_t *excl, int ld_e, int E, void *stream);
int b4c_topk_rows_excl(const void *scores, int ld, int64_t R, int V, int k, int32_t *topk_idx, const int32_t *labels, float *hit,
                       float *ndcg, int32_t *redo, int dtype, const int32_t *excl, int ld_e, int E, void *stream);

/* ---- candidate lists: score and rank a per-row list of items (sampled-negative evaluation, re-ranking) ---------------------
 * Item ids are in the label space [0, V) (input id - NUM_RESERVED_TOKENS), the space of the exclusion lists.
 * cand [R][C] int32 (pitch ld_c), 1 <= C <= B4C_MAX_CAND: an entry < 0 or >= V is ABSENT -- it never ranks and its `scores`
 *   entry is NaN.  A duplicated id counts once for rank and top-k; every position still gets its own score.
 * Score: s(r, c) = sum_k h[r][k] * wt[c][k] (fp32 accumulation) + bias[c]; h / wt bf16 or fp32 (dtype), K % 8 == 0, K <= 1024.
 *   The label's score and a listed item's score come from the same arithmetic: a listed copy of the label compares equal to
 *   the label, and no summation order creates or breaks a tie between them.
 * Rank: rank[r] = #{distinct present c of cand[r], c != y_r : s_c > s_y or (s_c == s_y and c < y_r)}; the label y_r is scored
 *   whether it is listed or not; negative for a row without a valid label (y < 0 or y >= V).  The tie rule of b4c_vocab_rank:
 *   with the list 0 .. V-1 the rank is the full-vocabulary rank wherever both compute the same fp32 scores.  HitRate@k /
 *   NDCG@k: b4c_rank_metrics.
 * Top-k: idx [R][k] (k <= B4C_MAX_TOPK) = the k best distinct present items of the list, score descending, ties -> lower id;
 *   fewer than k: the tail is -1.  The label appears only if it is listed.
 * b4c_sample_candidates: cand [R][1 + N] (pitch ld_c), cand[r][0] = y_r, then N <= B4C_MAX_CAND - 1 negatives in acceptance
 *   order.  Attempt j of row r draws x = b4c_rand64(seed, ((row_base + r) << 20) | j) (csrc/common.h) and the item
 *   mulhi64(x, V) (cdf == NULL: uniform) or min{i : cdf[i] > mulhi64(x, total)} (popularity: cdf [V] the inclusive int64 prefix
 *   sum of per-item counts, total = cdf[V-1] > 0 -- not checked: a total <= 0 draws nothing; items of count 0 are never drawn),
 *   mulhi64 = the high 64 bits of the 128-bit product.  An attempt is accepted iff its item is != y_r, not in the row's exclusion list (b4c_exclusions_prep
 *   form, E may be 0) and not accepted before; the first N accepted attempts in j order are kept.  Attempts stop at
 *   j = 64 N: a row still short has -1 in its tail and is counted in short_count[0] (zeroed here).  Rows without a valid label
 *   get -1 throughout and draw nothing.  A pure function of (seed, row_base + r, labels, exclusions, cdf): row_base keeps the
 *   draws independent of how the rows are split into batches or ranks.
 * b4c_candidate_score: scores [R][ld_s] fp32 (may be NULL), rank [R] (may be NULL; needs labels), idx [R][k] (k = 0 / NULL:
 *   no top-k).  One wave per row; the scores live in LDS and reach memory only when `scores` is given.
 * b4c_candidate_rank_rows: rank / top-k of the same definition on MATERIALISED scores [R][ld] (fp32 probabilities or logits,
 *   bf16 logits; dtype): the listed columns are gathered; `scores` is only read. */
int b4c_sample_candidates(const int32_t *labels, int64_t R, int V, int N, uint64_t seed, int64_t row_base, const int32_t *excl,
                          int ld_e, int E, const int64_t *cdf, int32_t *cand, int ld_c, int32_t *short_count, void *stream);
int b4c_candidate_score(const void *h, int ld_h, const void *wt, int ld_w, const float *bias, const int32_t *cand, int ld_c,
                        int64_t R, int C, int V, int K, int dtype, const int32_t *labels, float *scores, int ld_s, int32_t *rank,
                        int k, int32_t *idx, void *stream);
int b4c_candidate_rank_rows(const void *scores, int ld, int dtype, const int32_t *cand, int ld_c, int64_t R, int C, int V,
                            const int32_t *labels, int32_t *rank, int k, int32_t *idx, void *stream);

/* ---- Cloze batches: model inputs and padded labels built on the device from a CSR data set --------------------------------
 * replaces the host batch construction of input_pipeline.py:21-133 (drop / mask / pad) for integer item indices.
 * The data set: items int32 [N] (label-space item indices, input id = index + NUM_RESERVED_TOKENS = index + 10), offsets
 *   int64 [n_seq + 1]; sequence g is items[offsets[g] : offsets[g+1]], of length n_g.  seq_idx int32 [B] names the sequence
 *   of every batch row (not range-checked against n_seq: the caller's; a negative entry is an empty row).
 * The masking rule of a row that names sequence g:
 *   TRAIN (mode 0): L = max(n_g - 1, 0) (the last item is held out);
 *     n = min(max((int)((float)L * masked_percentage), 0), max_masked)  (float32 product, then truncation);
 *     position p in [0, L) has the key k_p = b4c_rand64(seed, ((uint64_t)g << 10) | p) (csrc/common.h); the masked set is the
 *     n positions smallest in (k_p, p) lexicographic order: p is masked iff #{q < L : (k_q, q) < (k_p, p)} < n.  A uniform draw
 *     without replacement, and a total function of its inputs (equal keys: the lower position first).
 *   EVAL (mode 1): L = n_g, the masked set is {L - 1} (empty for L = 0); no draw, max_masked / masked_percentage are not read.
 * Outputs: items_out int64 [B][W] (pitch ld_items >= W; columns past W are not written): column p < L is MASK_ID (1) where
 *   masked, else items[offsets[g] + p] + 10; columns L .. W-1 are INPUT_PAD (0) -- the {'asin': items} input of the model,
 *   which chains [CLS] [SEP] .. [SEP] itself (S = W + 3).  labels_out fp32 [B][M] (pitch ld_lab >= M): the masked positions'
 *   item indices in ascending position order, then LABEL_PAD (-1.0).  n_masked_out int32 [B] (may be NULL): the row's n.
 * A row is a pure function of (seed, g, the sequence, mode, masked_percentage, max_masked): not of the batch, the rank or the
 *   row's place in the batch.
 * Limits: 1 <= W <= 1021 (p < 1024 in the counter), g < 2^54, 0 <= max_masked <= M <= 64 (EVAL: 1 <= M <= 64),
 *   0 <= masked_percentage <= 1.  A sequence longer than W is the caller's error: L is clamped to W, nothing is written
 *   outside the row.  B = 0 is a no-op.
 * b4c_cloze_choose is the TRAIN rule on the HOST (no device work): pos[0 .. n) = the n masked positions of [0, L) for
 *   sequence g, ascending; 0 <= n <= L <= 1021. */
#define B4C_MAX_BATCH_WIDTH 1021   /* widest row W of every device-built batch: S = W + 3 <= 1024, p < 1024 in the counter */
#define B4C_MAX_CLOZE_LABELS 64    /* most label columns M of a Cloze batch */
int b4c_cloze_batch(const int32_t *items, const int64_t *offsets, const int32_t *seq_idx, int B, int W, int mode,
                    float masked_percentage, int max_masked, uint64_t seed, int64_t *items_out, int ld_items,
                    float *labels_out, int ld_lab, int M, int32_t *n_masked_out, void *stream);
int b4c_cloze_choose(uint64_t seed, int64_t g, int L, int n, int32_t *pos);

/* ---- Cloze batches over windows: the paper's data protocol (sliding training windows, last-item rows, history lists) -------
 * b4c_cloze_batch_windows: one row per WINDOW.  A window is (g, a, L): sequence g, start a inside it and L <= W items
 *   items[offsets[g] + a .. + L).  The window table is on the device: win_seq, win_start, win_len int32 [n_win].  row_win int32 [B]
 *   names the window of every batch row (NULL: row b is window b; a negative entry is an empty row, like a negative seq_idx
 *   above).  Neither row_win against n_win nor a window against its sequence is range-checked: the caller's.  The other
 *   arguments are those of b4c_cloze_batch, and last_thr in [0, 2^24].
 * The masking rule of a row that names window (g, a, L):
 *   window seed: seed_a = seed when a == 0, else b4c_rand64(seed ^ 0x9E3779B97F4A7C15, a).
 *   TRAIN (mode 0), ordinary row: n = min(max((int)((float)L * masked_percentage), 0), max_masked) as above, keys
 *     k_p = b4c_rand64(seed_a, ((uint64_t)g << 10) | p) for p in [0, L) (p counts from the window's start); the masked set is
 *     the n positions smallest in (k_p, p) order, as above.  A window (g, 0, n_g - 1) with last_thr = 0 is b4c_cloze_batch's
 *     TRAIN row of sequence g, bit for bit.
 *   TRAIN, last-only row: a row is last-only iff (b4c_rand64(seed_a ^ 0xD1B54A32D192ED03, g) >> 40) < last_thr and L > 0.  Then the
 *     masked set is {L - 1} and n = 1, whatever max_masked and masked_percentage are (so last_thr > 0 needs M >= 1).  The
 *     threshold is an integer (rate * 2^24, rounded by the caller) so that host and device cannot disagree on a float product.
 *   EVAL (mode 1): the masked set is {L - 1} (empty for L = 0); nothing is drawn, last_thr is not read.
 * Outputs, pad columns, label order, the -1.0 label pad and n_masked_out are exactly those of b4c_cloze_batch.
 * A row is a pure function of (seed, g, a, the window's items, mode, masked_percentage, max_masked, last_thr).
 * Limits: W and M as in b4c_cloze_batch, a >= 0 (a < 2^31: int32); win_len is clamped to [0, W]; nothing is written outside
 *   the row (columns past W are untouched).  B = 0 is a no-op.
 * b4c_cloze_choose_window is the TRAIN rule of one window on the HOST (no device work): pos[0 .. n_out[0]) = the masked
 *   positions of [0, L), ascending; pos has room for max(max_masked, 1) entries; 0 <= L <= 1021.  With a = 0 and last_thr = 0
 *   it is b4c_cloze_choose(seed, g, L, n(L), pos).
 * b4c_cloze_history: the items of a sequence that precede its target, as an exclusion list of filtered evaluation.
 *   out int32 [B][E] (pitch ld >= E, 1 <= E <= B4C_MAX_EXCL; columns past E are not written).  Row b names sequence
 *   g = seq_idx[b]; its history is h = items[offsets[g] .. offsets[g+1] - drop) with drop >= 1 (the target is item n_g - drop), of
 *   H = max(n_g - drop, 0) items.  out[b][e] = h[max(H - E, 0) + e] for e < min(H, E) (more than E items: the most recent E
 *   are kept), -1 after them.  A negative seq_idx gives an all -1 row.  The form b4c_exclusions_prep takes as ex_in. */
int b4c_cloze_batch_windows(const int32_t *items, const int64_t *offsets, const int32_t *win_seq, const int32_t *win_start,
                            const int32_t *win_len, const int32_t *row_win, int B, int W, int mode, float masked_percentage,
                            int max_masked, uint64_t seed, uint32_t last_thr, int64_t *items_out, int ld_items, float *labels_out,
                            int ld_lab, int M, int32_t *n_masked_out, void *stream);
int b4c_cloze_choose_window(uint64_t seed, int64_t g, int64_t a, int L, float masked_percentage, int max_masked, uint32_t last_thr,
                            int32_t *pos, int32_t *n_out);
int b4c_cloze_history(const int32_t *items, const int64_t *offsets, const int32_t *seq_idx, int B, int drop, int E, int32_t *out,
                      int ld, void *stream);

/* ---- R16: Adam (Keras semantics, eps outside the sqrt) ------------------------------------
 * replaces tf.keras.optimizers.Adam(1e-3, .9, .999, 1e-9) (main.py:87), dense update over a flat
 * fp32 arena: m,v EMA; p -= lr_t * m / (sqrt(v) + eps), lr_t = lr*sqrt(1-b2^t)/(1-b1^t) (host).
 * grad_mul scales g first (1/world_size for mean reduction; 1 for the reference's sum). */
int b4c_adam_step(float *p, const float *g, float *m, float *v, int64_t n, float lr_t, float beta1,
                  float beta2, float eps, float grad_mul, void *stream);

/* Adam for a row-sparse table inside the arena (config 5: 2M-row tables, < 0.1 % of the rows touched per step) -- the same
 * dense-equivalent Keras update (main.py:87), evaluated lazily per row: stamp[row] (int32, 0 = never touched) is the last
 * step the row is current through; a row is brought up to date by replaying the zero-gradient steps it missed with the
 * fp32 operations of b4c_adam_step in the same order (lr_hist[s] = the lr_t the host used at step s, s = 1 .. t), so
 * the table equals the dense kernel's bit for bit once every row is caught up.
 *   mode 0: bring the rows to step t (zero-gradient steps only): before anything reads them.
 *   mode 1: bring the rows to step t - 1, take step t with the gradient rows of g, zero those gradient rows.
 * ids (int64 [n], clamped to the table; a row named several times is handled once) or, ids == NULL, the rows
 * [row_lo, row_lo + n).  p, g, m, v: the table's [rows][width] slices of the four arenas (width % 4 == 0). */
int b4c_adam_rows(float *p, float *g, float *m, float *v, int32_t *stamp, const int64_t *ids, int64_t n, int64_t row_lo,
                  int64_t rows, int width, const float *lr_hist, int t, float beta1, float beta2, float eps,
                  float grad_mul, int mode, void *stream);

/* keep-mask hash used by every dropout site (exposed so hosts/tests can regenerate masks):
 * returns 1 if element e is kept under (seed, rate). */
int b4c_keep(uint64_t seed, uint64_t e, float rate);

/* ==== round-2 additions (ABI version 3) ================================================== */

/* ---- stand-alone dropout: Encoder.call's input dropout (transformer.py:263) when the Encoder is used
 * without the embedding stage that normally fuses it.  y[e] = keep(seed, e) ? x[e] / (1 - rate) : 0, e = flat
 * element index; applied to a gradient it is its own backward.  n % 8 == 0. */
int b4c_dropout(const void *x, void *y, int64_t n, float rate, uint64_t seed, int dtype, void *stream);

/* ---- backward of the materialised-probability route: the reference trains through
 * loss(y, model(x)) with model(x) = (B, M, V) probabilities (main.py:159-165, head.py:36-47, losses.py:31-98).
 * softmax:  dlogits_j = p_j (g_j - sum_i g_i p_i); pad columns V..ldx of dlogits are written 0.
 * sparse CE on probabilities (b4c_sparse_ce_from_probs): dprobs = gscale[0] * d item_loss / d probs for rows
 * whose label is not the pad (-1), 0 for pad rows; gscale is a DEVICE scalar (upstream gradient / n_valid). */
int b4c_softmax_rows_bwd(const void *probs, int ldp, const void *dprobs, int ldg, void *dlogits, int ldx,
                         int64_t R, int V, int dtype, void *stream);
int b4c_sparse_ce_from_probs_bwd(const void *probs, int ld, const float *labels, const float *gscale, void *dprobs,
                                 int ld_dp, int64_t R, int V, int variant, int dtype, void *stream);

/* ---- the other heads (head.py:4-26, 50-69): Dense(activation='sigmoid') and its backward
 * (dx = dy * y * (1 - y), y = the forward's output).  n % 8 == 0. */
int b4c_sigmoid_fwd(const void *x, void *y, int64_t n, int dtype, void *stream);
int b4c_sigmoid_bwd(const void *y, const void *dy, void *dx, int64_t n, int dtype, void *stream);

/* MaskedLoss with tf.keras.backend.binary_crossentropy on probabilities and the optional pos_weight
 * (losses.py:31-98): o = clip(p, 1e-7, 1 - 1e-7); bce = -(t log(o + 1e-7) + (1 - t) log(1 - o + 1e-7));
 * weight = pos_weight where t == 1 (pos_weight <= 0: none).  labels fp32, -1 = pad (loss 0, not counted).
 * sums[0] += sum of weighted item losses, sums[1] += number of non-pad items (caller zeroes);
 * item_loss [n] and dprobs [n] (fp32, = weight * d bce / d p, unscaled) may be NULL. */
int b4c_masked_bce(const void *probs, const float *labels, float pos_weight, float *item_loss, float *sums,
                   float *dprobs, int64_t n, int dtype, void *stream);

/* counts behind PositiveRate, PredictedPositives and F1Score (metrics.py:5-87) in one pass; out6 += :
 * [0] sum mask*y_true  [1] sum mask  [2] sum mask*round(y_pred)  [3] tp  [4] condition_true  [5] predicted_true
 * (mask = y_true != -1; tf.round = half to even; the F1 counts are not masked, as in the reference). */
int b4c_binary_counts(const float *y_true, const void *y_pred, float *out6, int64_t n, int dtype, void *stream);

/* ---- labels of the sync-free Cloze step: padded (B, M) fp32 labels (-1 pad; row b's labels are its first
 * counts[b] entries, input_pipeline.py:198-214) -> compact int32 [cap] in the row-major order of
 * b4c_mask_positions; entries at and beyond R = offsets[B] are set to -1 in `out` (ignored rows) and, when
 * flat_idx is given, to -1 there too (b4c_gather_rows then yields zero rows). */
int b4c_compact_labels(const float *labels, int B, int M, const int32_t *counts, const int32_t *offsets,
                       int32_t *out, int32_t *flat_idx, int32_t cap, void *stream);

/* ---- attention weights on request: the second result of MultiHeadAttention.call /
 * scaled_dot_product_attention (transformer.py:64-97, 137-160), which the encoder discards (:203).
 * weights fp32 [B][H][S][S] = exp(q k^T / sqrt(dh) + pad * -1e9 - lse). */
int b4c_attn_weights(const void *qkv, int ld_qkv, const uint8_t *key_pad, const float *lse, float *weights, int B,
                     int S, int H, int dh, int dtype, void *stream);

/* ---- tied-weight head (north-star extension, no reference counterpart): dst[n][k] += src[k][n], fp32 --
 * the projection gradient [K][V] added into rows of the embedding-table gradient [V][K]. */
int b4c_transpose_add(const float *src, int ld_src, float *dst, int ld_dst, int K, int N, void *stream);

/* ---- row-sparse gradient exchange: gather the touched rows of an fp32 gradient table
 * (idx int64, < 0 -> zero row) and add received rows back (float atomics; idx < 0 skipped).  width % 4 == 0. */
int b4c_rows_gather_f32(const float *src, int ld_src, const int64_t *idx, float *out, int ld_out, int64_t n,
                        int width, void *stream);
int b4c_rows_scatter_add_f32(const float *src, int ld_src, const int64_t *idx, float *dst, int ld_dst, int64_t n,
                             int width, void *stream);

/* ---- sampled-softmax head (BASELINE.json configs[4], SURVEY D10: north_star extension, NO reference counterpart) ----
 * Shared negatives from a log-uniform sampler WITH replacement over [0, range_max): P(c) = log((c+2)/(c+1)) / log(range_max+1)
 * (the distribution of tf.random.log_uniform_candidate_sampler), expected count Q(c) = n P(c).  Sample i uses the 24-bit
 * uniform (b4c rand64(seed, i) >> 40) / 2^24, so a host can regenerate the ids.  ids int64 [n], logq fp32 [n] = log Q(id). */
int b4c_log_uniform_sample(uint64_t seed, int n, int64_t range_max, int64_t *ids, float *logq, void *stream);
/* out[r] = sum_c a[r][c] b[r][c]  (fp32; width % 8 == 0): the true-class logits h_r . w_{y_r}. */
int b4c_row_dot(const void *a, int lda, const void *b, int ldb, float *out, int64_t R, int width, int dtype, void *stream);
/* tf.nn.sampled_softmax_loss semantics (remove_accidental_hits): Z [R][ld] holds the K negatives' logits with bias - logQ
 * folded in, ztrue[r] = h_r . w_y + b_y; the kernel subtracts logQ(y), drops negatives equal to the row's label, and
 * writes loss_r = logsumexp(z_true, z_neg) - z_true to item_loss, grad_scale[0] * softmax over the negatives IN PLACE of
 * Z, and grad_scale[0] * (softmax_true - 1) to dtrue.  Rows with label < 0 or >= range_max are ignored. */
int b4c_sampled_ce_fwd_bwd(void *Z, int ld, const float *ztrue, const int64_t *samples, const int32_t *labels,
                           int64_t range_max, float *item_loss, float *dtrue, const float *grad_scale, int64_t R,
                           int K, int dtype, void *stream);
/* dst[idx[i]] += src[i] (fp32 atomics, idx < 0 skipped);  out[r][:] = scale[r] * src[r][:] (fp32 out). */
int b4c_scatter_add_1d(const float *src, const int64_t *idx, float *dst, int64_t n, void *stream);
int b4c_row_scale_f32(const void *src, int ld, const float *scale, float *out, int ld_out, int64_t R, int width,
                      int dtype, void *stream);

/* ---- packed (padding-free) token layout -------------------------------------------------------------------------------
 * The reference pads every sequence to the batch maximum and runs the encoder on the pads too (transformer.py:376-402); pad
 * KEYS are masked out (:38-41, :90-91), pad QUERIES produce rows nobody reads, and under the Cloze loss their gradient is
 * exactly zero.  The throughput path therefore drops the pad positions: the encoder runs on the T_real real tokens only,
 * every row-wise kernel (GEMM, LayerNorm, embedding, Adam) unchanged on [T_real][d] tensors, attention per sequence through
 * cu_seqlens.  Results at real positions are those of the dense layout.
 * b4c_nonpad_positions: counts[B] real tokens per sequence, cu_seqlens[B+1] (exclusive scan, cu[B] = T_real),
 *   token_src[cap] = b*S + s of every real token in row-major order, packed_of[B*S] = packed row of a dense position or -1
 *   (may be NULL), maxcount[1] = longest sequence (may be NULL).  `cap` is the caller's token count: cu_seqlens are
 *   clamped to it (a wrong count can truncate sequences but never index past tensors sized by it), and when the true total
 *   differs from it maxcount[0] is written as -(longest) - 1: a poison flag.
 * b4c_remap_index: out[i] = idx[i] >= 0 ? map[idx[i]] : -1 ([MASK] positions of the dense layout -> packed rows).
 * b4c_embed_concat_pe_fwd_packed: b4c_embed_concat_pe_fwd writing only rows t < n_tokens, row t taken from dense position
 *   token_src[t] (ids and positional row s = token_src[t] % S); the dropout counter is the packed element index.
 * b4c_attn_{fwd,bwd}_varlen: attention with sequence b in rows cu_seqlens[b] .. cu_seqlens[b+1] (bf16, head depth 32 / 64,
 *   max_len <= 512); lse / delta keep the shape [B][H][max_len]; workspace as b4c_attn_bwd_ws (max_len > 256). */
int b4c_nonpad_positions(const int64_t *ids, int B, int S, int64_t pad_value, int32_t *counts, int32_t *cu_seqlens,
                         int32_t *token_src, int32_t cap, int32_t *packed_of, int32_t *maxcount, void *stream);
int b4c_remap_index(const int32_t *idx, const int32_t *map, int32_t *out, int64_t n, void *stream);
int b4c_embed_concat_pe_fwd_packed(int n_feat, const int64_t *const *h_ids, const float *const *h_tables,
                                   const int *h_dims, const int64_t *h_rows, const float *pe, float scale,
                                   void *out, int ld_out, uint8_t *key_pad, int B, int S, int d_model,
                                   float dropout_rate, uint64_t seed, const int32_t *token_src, int64_t n_tokens,
                                   int dtype, void *stream);
/* EMBEDDING STAGE WITH LAYERNORM (no reference counterpart: the input stage of the BERT4Rec paper), one pass.  The arguments
 * of b4c_embed_concat_pe_fwd_packed (token_src == NULL: the dense layout, T = B*S rows) plus gamma, beta (fp32 [d_model]), eps
 * and stats (fp32 [T][2] = {mean, rstd}, may be NULL).  Per output row t, in fp32:
 *   pre  = scale * (concat_f | sum_f) table_f[ids_f[ts]] + pe[ts % S],  ts = token_src ? token_src[t] : t
 *   mean = sum(pre) / d,  var = sum((pre - mean)^2) / d  (biased),  rstd = 1 / sqrt(var + eps)
 *   out  = keep(e) / (1 - rate) * (gamma * (pre - mean) * rstd + beta),  e = t*d_model + col  (the numbering of the plain stage)
 * key_pad as b4c_embed_concat_pe_fwd.  pre never reaches memory and is not rounded to `dtype` before the statistics; pad rows of
 * the dense layout are normalised like any other.  d_model % 8 == 0, d_model <= 1024 (the rows of b4c_add_dropout_layernorm_fwd).
 * b4c_embed_ln_bwd: dout [T][ld_dout] -> dpre [T][ld_dpre] (`dtype`), dgamma / dbeta (fp32 [d_model], ADDED to); pre is gathered
 * again from the same ids, tables, pe and scale, xhat = (pre - mean) * rstd from the saved stats:
 *   g = keep(e) / (1 - rate) * dout;  dbeta += sum_t g;  dgamma += sum_t g * xhat
 *   a = g * gamma;  dpre = rstd * (a - mean_j(a) - xhat * mean_j(a * xhat))
 * dgamma / dbeta as b4c_layernorm_bwd: fixed-order sums through the workspace (b4c_embed_ln_bwd_workspace_bytes(T, d_model),
 * required), no float atomics.  The tables' and a learned pe's gradients are those of the plain stage with dout = dpre and
 * dropout_rate = 0: b4c_embed_concat_pe_bwd(_sorted_ws) and b4c_pos_table_bwd. */
int b4c_embed_ln_fwd(int n_feat, const int64_t *const *h_ids, const float *const *h_tables, const int *h_dims,
                     const int64_t *h_rows, const float *pe, float scale, const float *gamma, const float *beta, float eps,
                     void *out, int ld_out, float *stats, uint8_t *key_pad, int B, int S, int d_model, float dropout_rate,
                     uint64_t seed, const int32_t *token_src, int64_t n_tokens, int dtype, void *stream);
int64_t b4c_embed_ln_bwd_workspace_bytes(int64_t rows, int d_model);
int b4c_embed_ln_bwd(int n_feat, const int64_t *const *h_ids, const float *const *h_tables, const int *h_dims,
                     const int64_t *h_rows, const float *pe, float scale, const float *gamma, const float *stats,
                     const void *dout, int ld_dout, void *dpre, int ld_dpre, float *dgamma, float *dbeta, int B, int S,
                     int d_model, float dropout_rate, uint64_t seed, const int32_t *token_src, int64_t n_tokens,
                     void *workspace, int64_t workspace_bytes, int dtype, void *stream);
int b4c_attn_fwd_varlen(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, void *o, int ld_o,
                        float *lse, int B, int max_len, int H, int dh, int dtype, void *stream);
int b4c_attn_bwd_varlen(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, const void *o,
                        int ld_o, const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv,
                        int B, int max_len, int H, int dh, void *workspace, int64_t workspace_bytes, int dtype,
                        void *stream);

/* ---- (ABI version 4) attention for a few query rows per sequence: the LAST encoder layer of the Cloze path ------------
 * The reference runs every layer on every position (transformer.py:262-270) and keeps the rows at the [MASK] positions
 * (clickstream_transformer.py:281-295); in the last layer all other rows are never read.  There the queries are the masked
 * rows of a sequence, the keys / values all of its tokens (transformer.py:64-97 for those rows, fp32 math, both dtypes):
 *   q / o / dq [R][ld]: head h in columns h*dh..;  kv / dkv [T][ld]: k in columns h*dh.., v in H*dh + h*dh..;
 *   sequence b = token rows cu_seqlens[b] .. cu_seqlens[b+1] and query rows q_offsets[b] .. q_offsets[b+1];
 *   key_pad [T] (1 = padded key, may be NULL); lse [R][H] (natural log of the row's softmax denominator).
 * b4c_attn_mq_bwd writes dq for the R query rows and dk | dv for EVERY token row (zeros where no query reads them).
 * dh in {32, 64}; max_len = longest sequence (LDS sizing). */
/* order[i] = position (0..n-1) of the i-th smallest id, ties in position order (a stable sort of the token positions by
 * table row: the order b4c_embed_concat_pe_bwd_sorted walks); ids are clamped to [0, n_rows - 1] as the embedding kernels
 * clamp them.  LSD radix, 8-bit digits, 2 launches per pass (3 past 1 M keys); workspace >= b4c_sort_ids_workspace_bytes(n, n_rows), 4-B aligned. */
int64_t b4c_sort_ids_workspace_bytes(int64_t n, int n_rows);
int b4c_sort_ids(const int64_t *ids, int64_t n, int n_rows, int32_t *order, void *workspace, int64_t workspace_bytes, void *stream);
int b4c_gather_i64(const int64_t *src, const int32_t *idx, int64_t *out, int64_t n, void *stream);   /* out[i] = src[idx[i]] */
/* (ABI version 7) b4c_zero: nbytes of zeros at p (stream-ordered).  b4c_chain_ids: out[b] = [cls, sep, seq_0[b], sep, seq_1[b],
 * sep, ...] -- TransformerInputPrep._chain_sequences (clickstream_transformer.py:38-63) for already-mapped int64 ids;
 * seqs / lens / pitches are HOST arrays of n_seq (<= 8) device pointers, row lengths and row pitches (elements);
 * out has 2 + sum(lens) + n_seq columns on a pitch of ld_out. */
int b4c_zero(void *p, int64_t nbytes, void *stream);
int b4c_chain_ids(const int64_t *const *seqs, const int *lens, const int *pitches, int n_seq, int B, int64_t cls,
                  int64_t sep, int64_t *out, int ld_out, void *stream);
int b4c_rows_add(void *dst, int ld_dst, const int32_t *idx, const void *src, int ld_src, int64_t n_src, int width, int dtype,
                 int src_dtype, void *stream);   /* dst[idx[r]] += src[r] (idx distinct, < 0 skipped; src may be fp32 beside a
                                                  * bf16 dst): the query rows' gradient joins that of all token rows */
int b4c_poison_rows(void *x, int ld, int64_t rows, int width, const int32_t *flag, int dtype, void *stream);
                                                 /* x[rows][width] := NaN (B4C_I32: -1) when flag[0] < 0 (the negated maxcount of
                                                  * b4c_nonpad_positions / b4c_mask_positions: a caller-given count that the
                                                  * device's own contradicts), untouched otherwise: the scoring paths' answer to
                                                  * a wrong n_real_tokens, without a read-back (the loss paths fold the flag
                                                  * into the loss: b4c_sum_scaled) */
int b4c_attn_mq_fwd(const void *q, int ld_q, const void *kv, int ld_kv, const uint8_t *key_pad, const int32_t *cu_seqlens,
                    const int32_t *q_offsets, void *o, int ld_o, float *lse, int B, int max_len, int H, int dh, int dtype,
                    void *stream);
int b4c_attn_mq_bwd(const void *q, int ld_q, const void *kv, int ld_kv, const uint8_t *key_pad, const int32_t *cu_seqlens,
                    const int32_t *q_offsets, const void *o, int ld_o, const void *d_o, int ld_do, const float *lse,
                    void *dq, int ld_dq, void *dkv, int ld_dkv, int B, int max_len, int H, int dh, int dtype, void *stream);

/* ---- global-norm gradient clipping (Adam(global_clipnorm=...); the reference never clips: no oracle, the BERT4Rec paper's
 * recipe) -- additive to ABI 12: no existing signature changed, b4c_abi_version() stays 12 ------------------------------
 * The squared L2 norm of the fp32 gradient arena g[0, n) with a POSITION-DEFINED reduction (csrc/gradnorm.hip): the arena is
 * cut into chunks of B4C_GRAD_CHUNK consecutive elements counted from g; partial[c] (float64, ceil(n / B4C_GRAD_CHUNK)
 * entries) is the sum of the squares of the WHOLE chunk c in a fixed order, whoever computes it.
 *   b4c_grad_sumsq       writes partial[c] of every chunk that overlaps [lo, hi) (each over its whole extent).
 *   b4c_grad_sumsq_rows  one wave per id (int64, repeats allowed, clamped to [0, rows) as b4c_adam_rows clamps them) rewrites
 *                        the partial of every chunk that row of the (rows x width) table at g + table_lo overlaps; the caller
 *                        zero-fills the partials of chunks nobody names (their gradient is all zeros).
 *   b4c_grad_clip_coef   total = fixed tree over partial[0, n_chunks) (group_sums: scratch of n_groups =
 *                        ceil(n_chunks / B4C_GRAD_GROUP) doubles); *total (may be NULL) = it; norm_coef[0] = sqrt(total) |grad_mul|
 *                        in fp32, norm_coef[1] = norm > clip ? clip / norm : exactly 1.0f; NaN when the norm is not finite.
 * b4c_adam_step_clipped / b4c_adam_rows_clipped: b4c_adam_step / b4c_adam_rows with the gradient scaled by
 * grad_mul * *coef (coef: device fp32, e.g. norm_coef + 1) -- no host read-back anywhere. */
#define B4C_GRAD_CHUNK 1024
#define B4C_GRAD_GROUP 4096
int b4c_grad_sumsq(const float *g, int64_t n, int64_t lo, int64_t hi, double *partial, void *stream);
int b4c_grad_sumsq_rows(const float *g, int64_t n, int64_t table_lo, int64_t rows, int width, const int64_t *ids, int64_t n_ids,
                        double *partial, void *stream);
int b4c_grad_clip_coef(const double *partial, int64_t n_chunks, double *group_sums, int64_t n_groups, float clip, float grad_mul,
                       double *total, float *norm_coef, void *stream);
int b4c_adam_step_clipped(float *p, const float *g, float *m, float *v, int64_t n, float lr_t, float beta1, float beta2, float eps,
                          float grad_mul, const float *coef, void *stream);
int b4c_adam_rows_clipped(float *p, float *g, float *m, float *v, int32_t *stamp, const int64_t *ids, int64_t n, int64_t row_lo,
                          int64_t rows, int width, const float *lr_hist, int t, float beta1, float beta2, float eps, float grad_mul,
                          const float *coef, int mode, void *stream);

/* ---- decoupled weight decay (Adam(weight_decay=...), Keras AdamW; the reference never decays: no oracle, the BERT4Rec paper's
 * recipe) -- additive to ABI 12 ------------------------------------------------------------------------------------------------
 * A decayed element takes  p <- p - decay * p  (one fp32 product, one subtraction) and then the Adam update of b4c_adam_step,
 * unchanged.  decay = fp32(lr(t - 1) * weight_decay): the plain learning rate of the step, not lr_t, rounded once by the host.
 * The decay does not go through the gradient (grad_mul and coef do not touch it).  coef may be NULL in both entry points: the
 * clipped and the unclipped step share them.
 *   b4c_adamw_step  over a dense range: decay_blocks[i] != 0 (uint8, ceil(n / 64) entries) marks the 64-element block
 *                   p[64 i, 64 i + 64) as decayed; elements of the other blocks take exactly the update of b4c_adam_step.
 *   b4c_adamw_rows  b4c_adam_rows for a table that decays as a whole: decay_hist[s] is the decay factor of step s beside
 *                   lr_hist[s].  A row is replayed from its stamp even when that is 0 and when its moments are zero, one
 *                   step at a time, so the table still equals the dense kernel's bit for bit. */
int b4c_adamw_step(float *p, const float *g, float *m, float *v, int64_t n, float lr_t, float beta1, float beta2, float eps,
                   float grad_mul, const float *coef, float decay, const uint8_t *decay_blocks, void *stream);
int b4c_adamw_rows(float *p, float *g, float *m, float *v, int32_t *stamp, const int64_t *ids, int64_t n, int64_t row_lo,
                   int64_t rows, int width, const float *lr_hist, const float *decay_hist, int t, float beta1, float beta2,
                   float eps, float grad_mul, const float *coef, int mode, void *stream);

/* ---- attention-probability dropout (BERT's attention_probs_dropout_prob, nn.MultiheadAttention(dropout=); the reference's
 * attention has none: no oracle, the BERT4Rec paper's recipe) -- additive to ABI 12 --------------------------------------------
 * With P the masked softmax of b4c_attn_fwd, for sequence b, head h, query q, key k:
 *   P~[q][k] = keep(b, h, q, k) ? P[q][k] / (1 - rate) : 0;   o = P~ v;   lse is that of P (the row sum takes the undropped p).
 * Backward, with dP~ = dO V^T and delta = rowsum(dO o O) (O already holds the dropped probabilities):
 *   dV = P~^T dO;   dS = P o (keep / (1 - rate) * dP~ - delta);   dQ = dS K / sqrt(dh);   dK = dS^T Q / sqrt(dh).
 * THE KEEP RULE (one rule for every kernel; csrc/common.h): the probability of (b, h, q, k) is element
 *   e = ((b*H + h) * S_arg + q) * S4 + k,   S4 = S_arg rounded up to a multiple of 4,
 * of the keep-mask stream of b4c_keep: kept iff b4c_keep(seed, e, rate).  q and k are the row indices INSIDE the sequence as the
 * kernel sees them (dense layout: the position; packed layout: row - cu_seqlens[b]); S_arg is the pitch of the launch (S, or the
 * packed layout's max_len).  Four consecutive keys k0 .. k0+3 (k0 % 4 == 0) of one query share one hash.
 * b4c_attn_keep is that rule on the host (1 = kept), so tests and other hosts regenerate the masks without a GPU.
 * The four entry points are b4c_attn_fwd, b4c_attn_bwd_ws, b4c_attn_fwd_varlen and b4c_attn_bwd_varlen with (dropout_rate, seed)
 * appended; the workspace is b4c_attn_bwd_workspace_bytes'.  dropout_rate == 0 launches the very kernels of those entry points;
 * a rate outside [0, 1) is B4C_EINVAL.  b4c_attn_weights keeps returning the undropped softmax.
 * The masked-query kernels: b4c_attn_mq_fwd_drop / b4c_attn_mq_bwd_drop are b4c_attn_mq_fwd / _bwd with (q_rows, dropout_rate,
 * seed) appended.  q_rows (int32 [R]) is the token row of each query row: the keep rule's q of query row r of sequence b is
 * q_rows[r] - cu_seqlens[b] and S_arg is max_len, so with the same seed the masks are those the full layer's entry points draw
 * for these rows, in the dense (cu_seqlens[b] = b*S) and the packed layout.  q_rows is read for the rows q_offsets names only (an
 * unused row may hold -1) and no address depends on it.  dropout_rate == 0 launches the very kernels of b4c_attn_mq_fwd / _bwd and
 * q_rows may be NULL; a rate outside [0, 1), or a rate > 0 with a NULL q_rows, is B4C_EINVAL. */
int b4c_attn_keep(uint64_t seed, int b, int h, int q, int k, int H, int S_arg, float rate);
int b4c_attn_fwd_drop(const void *qkv, int ld_qkv, const uint8_t *key_pad, void *o, int ld_o, float *lse, int B,
                      int S, int H, int dh, int dtype, void *stream, float dropout_rate, uint64_t seed);
int b4c_attn_bwd_drop_ws(const void *qkv, int ld_qkv, const uint8_t *key_pad, const void *o, int ld_o,
                         const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv, int B,
                         int S, int H, int dh, void *workspace, int64_t workspace_bytes, int dtype, void *stream,
                         float dropout_rate, uint64_t seed);
int b4c_attn_fwd_varlen_drop(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, void *o, int ld_o,
                             float *lse, int B, int max_len, int H, int dh, int dtype, void *stream, float dropout_rate,
                             uint64_t seed);
int b4c_attn_bwd_varlen_drop(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, const void *o,
                             int ld_o, const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv,
                             int B, int max_len, int H, int dh, void *workspace, int64_t workspace_bytes, int dtype,
                             void *stream, float dropout_rate, uint64_t seed);
int b4c_attn_mq_fwd_drop(const void *q, int ld_q, const void *kv, int ld_kv, const uint8_t *key_pad, const int32_t *cu_seqlens,
                         const int32_t *q_offsets, void *o, int ld_o, float *lse, int B, int max_len, int H, int dh, int dtype,
                         void *stream, const int32_t *q_rows, float dropout_rate, uint64_t seed);
int b4c_attn_mq_bwd_drop(const void *q, int ld_q, const void *kv, int ld_kv, const uint8_t *key_pad, const int32_t *cu_seqlens,
                         const int32_t *q_offsets, const void *o, int ld_o, const void *d_o, int ld_do, const float *lse,
                         void *dq, int ld_dq, void *dkv, int ld_dkv, int B, int max_len, int H, int dh, int dtype, void *stream,
                         const int32_t *q_rows, float dropout_rate, uint64_t seed);

/* ==== the attention entry points that take everything (additive to ABI 12) ====================================================== */

/* ---- causal (left-to-right) self-attention (the "look ahead" mask of the reference's scaled_dot_product_attention,
 * transformer.py:64-97, which its encoder never builds; SASRec and the BERT4Rec paper's unidirectional arm) -- additive to ABI 12 ----
 * One entry point per direction that takes everything: the layout (cu_seqlens == NULL: dense, S rows per sequence; otherwise the
 * packed layout with S = max_len and its limits: bf16, head depth 32 / 64, max_len <= 512), attention dropout (dropout_rate, seed
 * as in the *_drop entry points; 0 = none) and flags.  flags == 0 reaches exactly the launches of b4c_attn_fwd[_varlen][_drop] /
 * b4c_attn_bwd_ws / _drop_ws / _varlen[_drop] / b4c_attn_weights; an unknown flag bit is B4C_EINVAL.  The backward workspace is
 * b4c_attn_bwd_workspace_bytes'.
 * B4C_ATTN_CAUSAL: key k is visible to query q iff k <= q, both counted inside the sequence as the keep rule counts them (dense:
 * the position; packed: row - cu_seqlens[b]).  Over the visible keys
 *   P[q][k] = softmax_{k <= q}(q . k / sqrt(dh) + pad[k] * -1e9),   lse[q] = the log-sum-exp over the visible keys,
 * and the keys behind q are excluded outright (-inf, not -1e9): exactly zero weight and exactly zero gradient whatever the padding
 * looks like.  Key q is always visible to query q, so no row is empty.  A query whose visible keys are all padded (leading pads
 * only) comes out finite; its value is not otherwise pinned, as for a sequence without a live key in b4c_attn_fwd.
 * Dropout: a causal launch draws, for every visible (q, k), the bit b4c_attn_keep(seed, b, h, q, k, H, S, rate) that the
 * bidirectional launch draws.  b4c_attn_weights_ex returns the undropped P, 0 for k > q, from the lse of a causal forward.
 * The masked-query kernels (b4c_attn_mq_*) take the same flag through b4c_attn_mq_fwd_ex / b4c_attn_mq_bwd_ex (below).
 * Not covered: general [Sq][Sk] masks. */
#define B4C_ATTN_CAUSAL 1u
int b4c_attn_fwd_ex(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens /* NULL: dense */, void *o,
                    int ld_o, float *lse, int B, int S /* or max_len */, int H, int dh, int dtype, void *stream,
                    float dropout_rate, uint64_t seed, uint32_t flags);
int b4c_attn_bwd_ex(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens /* NULL: dense */,
                    const void *o, int ld_o, const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv,
                    int ld_dqkv, int B, int S /* or max_len */, int H, int dh, void *workspace, int64_t workspace_bytes,
                    int dtype, void *stream, float dropout_rate, uint64_t seed, uint32_t flags);
int b4c_attn_weights_ex(const void *qkv, int ld_qkv, const uint8_t *key_pad, const float *lse, float *weights, int B, int S,
                        int H, int dh, int dtype, void *stream, uint32_t flags);

/* ==== sampled-negative training: the loss over a per-row candidate list and its backward (additive to ABI 12) =================== */

/* ---- the definition ----------------------------------------------------------------------------------------------------------
 * h     [R][K] (pitch ld_h) bf16 or fp32 (dtype), K % 8 == 0, 8 <= K <= 1024, rows 16-byte aligned.
 * table the fp32 MASTER table [rows][ld_t] (ld_t % 4 == 0, 16-byte aligned); item id is row row_off + id: the vocabulary-major
 *       projection with row_off = 0, the tied item-embedding table with row_off = its id offset.  row_off + V <= rows.
 * bias  fp32 [V].
 * cand  int32 [R][C] (pitch ld_c), 1 <= C <= B4C_MAX_CAND, label-space ids.  Column 0 is the row's TARGET (the layout
 *       b4c_sample_candidates writes).  An entry < 0 or >= V is ABSENT: no term, coefficient exactly 0.  A row whose column 0 is
 *       absent is an IGNORED row: loss exactly 0, exactly zero gradient everywhere.  Every present position is its own term: a
 *       repeated id is not merged.
 * Score: s_c = sum_k h[k] * w_c[k] + bias[c], fp32 accumulation; for bf16 h every table element is rounded to bf16 (nearest
 *       even) before the product -- the value the packed copy of the table would hold.  The master table is what is read, so
 *       the kernels work under the row-lazy optimizer and on a table that is never packed.
 * kind  B4C_CAND_BCE:     l = softplus(-s_0) + sum_{c >= 1 present} softplus(s_c);   g_0 = sigma(s_0) - 1,  g_c = sigma(s_c)
 *       B4C_CAND_SOFTMAX: l = logsumexp_{present c} s_c - s_0 (max-subtracted);       g_c = p_c - [c == 0]
 *                         (C == 1: loss and coefficient exactly 0)
 *       softplus / sigma in their stable forms (|s| = 100: a finite loss, a coefficient in [0, 1]); expf, log1pf and logf, not the
 *       fast intrinsics.  Any other kind is B4C_EINVAL.
 * The model loss is sum_r l_r / max(#rows with a present target, 1), formed by the caller.
 *
 * b4c_candidate_loss_fwd: item_loss [R] and the coefficients g [R][ld_g] (0 at absent entries and in ignored rows), fp32;
 *   scores [R][ld_s] only when given (NaN at absent entries and throughout an ignored row, whose list is not read).  One wave
 *   per row; the V logits never exist.
 * b4c_candidate_loss_bwd: with gs = gscale[0] (a DEVICE scalar: 1 / valid rows, times the upstream gradient)
 *     dh[r][:]                  = gs * sum_c g[r][c] * w_c[:]      fp32 accumulation, stored once in h's dtype (ld_dh, aligned as h)
 *     dtable[row_off + id][:]  += gs * g[r][c] * h[r][:]           fp32 gradient sinks: ACCUMULATED, no-return float atomics,
 *     dbias[id]                += gs * g[r][c]                     one table row segment per wave-instruction
 *   An entry whose gs * g is exactly 0 adds nothing.  Two list entries of a launch that name the same item make dtable / dbias
 *   depend on the arrival order in the last bits; with pairwise disjoint lists every element receives one add and the result is
 *   reproducible.  dtable [rows][ld_dt] is addressed like table.
 * R == 0 is a no-op.  Null pointers, K, C, a pitch below its width, a misaligned operand, kind and dtype are B4C_EINVAL before
 * any launch. */
#define B4C_CAND_BCE 0
#define B4C_CAND_SOFTMAX 1
#define B4C_CAND_KINDS 2   /* kinds are 0 .. B4C_CAND_KINDS - 1 */
int b4c_candidate_loss_fwd(const void *h, int ld_h, const float *table, int ld_t, int64_t rows, int64_t row_off, const float *bias,
                           const int32_t *cand, int ld_c, int64_t R, int C, int V, int K, int dtype, int kind, float *item_loss,
                           float *g, int ld_g, float *scores /* may be NULL */, int ld_s, void *stream);
int b4c_candidate_loss_bwd(const void *h, int ld_h, const float *table, int ld_t, int64_t rows, int64_t row_off,
                           const int32_t *cand, int ld_c, const float *g, int ld_g, const float *gscale, int64_t R, int C, int V,
                           int K, int dtype, void *dh, int ld_dh, float *dtable, int ld_dt, float *dbias, void *stream);

/* ==== next-item batches built on the device (additive to ABI 12): every real position of a left-to-right row predicts the item
 * that follows it, each target against its own negatives, none of them an item of the user's ================================== */

/* ---- the rule ----------------------------------------------------------------------------------------------------------------
 * Data: the CSR data set of the Cloze batches (above, "Cloze batches"): items int32 [n_items] label-space indices, offsets int64
 * [n_seq + 1]; s_g is sequence g, n_g its length, offsets[g] its start.  Input id = item + 10, pad 0; no [MASK] anywhere.
 *
 * TRAIN row of the window (g, a, L) of the table (win_seq, win_start, win_len), with the training view [0, T_g),
 *   T_g = max(n_g - holdout, 0):  first = a > 0 ? a - 1 : 0,  n_in = a > 0 ? L : max(L - 1, 0)  (a later window takes one extra
 *   input in front, so abutting windows make every item of the view but the first a target exactly once).
 *   Input p is s_g[first + p], target p is s_g[first + p + 1], 0 <= p < n_in.  n_in is cut at W and at T_g - first - 1 (a target
 *   never leaves the view; a table built by the window rule is never cut).
 * EVAL row of sequence g (row_win names SEQUENCES here; the window table is not read), drop = `holdout` argument (1: the last
 *   item is the target, 2: the penultimate):  t = n_g - drop,  n_in = min(t, max_len, W),  first = t - n_in.  One target, at the
 *   last input position p = n_in - 1, label s_g[t].  t < 1: no input and no target.
 * A negative row_win[b] (or sequence) is an empty row.
 *
 * Compact rows: target number q of batch row b (TRAIN: q = p; EVAL: q = 0) is compact row r = row_off[b] + q; row_off int32
 *   [B + 1] is the exclusive prefix sum of the rows' target counts (the caller forms it from its host-known table; nothing is
 *   read back), row_off[B] = R.  flat_idx[r] = b * (W + 3) + 2 + p: the position of input p in the chained layout
 *   [CLS] [SEP] items .. [SEP] of a one-feature model; B * (W + 3) < 2^31.  labels[r] = the target's item index.
 *   The outputs hold `rows` >= R compact rows: rows R .. rows get flat_idx = -1, label = -1, candidates -1 (the "zero row" of
 *   b4c_remap_index and of the row gather; a label the losses ignore).  A compact row >= `rows` is never written.
 *
 * Negatives (0 <= N < B4C_MAX_CAND; N == 0: no sampler, cand is not written and may be NULL): cand[r] = [y, N negatives] is
 *   what b4c_sample_candidates returns for ONE row with label y = labels[r], row_base + row = i, where
 *   i = offsets[g] + first + p + 1 is the CSR index of the target token, the same seed and cdf (NULL: uniform), and the
 *   exclusion list X_g minus {y}: attempt j draws b4c_rand64(seed, (i << 20) | j), the first N distinct accepted items are kept
 *   in attempt order, at most 64 N attempts; a short row keeps -1 in its tail and adds one to short_count[0] (zeroed here).
 *   X_g, excl = B4C_NEXT_EXCL_HISTORY: the items of s_g[max(0, T - B4C_MAX_EXCL) .. T), T = T_g (TRAIN: the training view, never
 *   a held-out item, the whole sequence's view and not the window's) or t (EVAL: everything in front of the target).
 *   excl = B4C_NEXT_EXCL_NONE: empty.
 * The result is a pure function of (seed, data set, g, position, N, cdf, excl): independent of the batch, of the row's place in
 * it, of the batch size and of the rank.
 *
 * b4c_next_item_batch: one workgroup per batch row; X_g is sorted into LDS once and shared by the row's targets, one wave per
 *   target at a time.  items_out int64 [B][ld_items >= W]: columns 0 .. W of every row are written.  Every refusal -- null
 *   pointers, W outside 1 .. 1021, N, V, max_len (EVAL), holdout, the pitches, rows, B (W + 3) >= 2^31, mode, excl -- is
 *   B4C_EINVAL before any launch; B == 0 launches nothing (short_count is still zeroed when given, tails are NOT written).
 * b4c_next_item_row: the same rule for ONE row on the host, into host arrays -- seq = s_g (n_g items), seq_off = offsets[g];
 *   (a, L) the window (TRAIN; ignored for EVAL).  inputs_out int64 [W] (ids, 0 past n_in), labels_out int32 [W],
 *   pos_out int32 [W] (the input position p of each target), cand_out int32 [n_targets][ld_c] (N > 0), counts_out int32 [3] =
 *   (n_in, n_targets, short rows).  cdf is a HOST array here. */
#define B4C_NEXT_TRAIN 0
#define B4C_NEXT_EVAL 1
#define B4C_NEXT_EXCL_NONE 0
#define B4C_NEXT_EXCL_HISTORY 1
int b4c_next_item_batch(const int32_t *items, const int64_t *offsets, const int32_t *win_seq, const int32_t *win_start,
                        const int32_t *win_len, const int32_t *row_win, const int32_t *row_off, int B, int W, int mode, int holdout,
                        int max_len, int V, int N, uint64_t seed, int excl, const int64_t *cdf /* may be NULL */, int64_t *items_out,
                        int ld_items, int32_t *flat_idx, int32_t *labels, int32_t *cand /* NULL iff N == 0 */, int ld_c, int64_t rows,
                        int32_t *short_count /* NULL iff N == 0 */, void *stream);
int b4c_next_item_row(const int32_t *seq, int n_g, int64_t seq_off, int a, int L, int W, int mode, int holdout, int max_len, int V, int N,
                      uint64_t seed, int excl, const int64_t *cdf /* may be NULL */, int64_t *inputs_out, int32_t *labels_out,
                      int32_t *pos_out, int32_t *cand_out /* NULL iff N == 0 */, int ld_c, int32_t *counts_out);

/* ==== side features beside the items of a device-built batch (additive to ABI 12): for every row that b4c_cloze_batch_windows or
 * b4c_next_item_batch has just written, the ids of up to B4C_MAX_FEATURES further embedded features (an action per event, a
 * category per item, ...), masked where the item row is and the feature would give the target away ============================= */

/* ---- the rule ----------------------------------------------------------------------------------------------------------------
 * Data: the CSR data set of the Cloze batches (above, "Cloze batches"): items int32 [n_items] label-space indices, offsets int64
 * [n_seq + 1]; s_g is sequence g, n_g its length.
 *
 * Sources: feature f of n_feat (1 <= n_feat <= B4C_MAX_FEATURES) is an int32 device array src_f and two codes.
 *   kind B4C_FEAT_EVENT: src_f [n_items] is aligned with `items`, the value of token i is src_f[i]            (an action, a dwell bucket)
 *   kind B4C_FEAT_ITEM:  src_f [V] is a table over the items, the value of token i is src_f[items[i]]         (a category, a brand)
 *   on_mask B4C_FEAT_MASKED: a [MASK] position of the item row is a [MASK] position of this feature (a function of the item
 *   would give the target away);  B4C_FEAT_KEPT: the value stays visible there.
 *
 * Row geometry: batch row b covers the n tokens of sequence g from position `first` on; a negative row_win[b] is an empty row
 * (n = 0); row_win NULL: w = b.  The three layouts restate the rows of the builders the item row came from:
 *   B4C_FEAT_CLOZE       b4c_cloze_batch_windows' row (above): w = row_win[b] names a window of the table (win_seq, win_start,
 *                        win_len): g = win_seq[w], first = win_start[w], n = clamp(win_len[w], 0, W).  TRAIN and EVAL rows alike
 *                        (an evaluation row is a window that ends at its target).
 *   B4C_FEAT_NEXT_TRAIN  the TRAIN row of b4c_next_item_batch: the window (g, a, L) as above, T_g = max(n_g - holdout, 0):
 *                        first = a > 0 ? a - 1 : 0,  n = a > 0 ? L : max(L - 1, 0), cut at W and at T_g - first - 1.
 *   B4C_FEAT_NEXT_EVAL   the EVAL row of b4c_next_item_batch: w = row_win[b] names SEQUENCE g = w (the table is not read),
 *                        t = n_g - holdout:  n = min(t, max_len, W), first = t - n;  t < 1: n = 0.
 *
 * Output: out_f int64 [B][ld_out >= W]; columns 0 .. W of every row are written and nothing past them.  Column p, with
 * i = offsets[g] + first + p:
 *   p >= n                                                        0        (INPUT_PAD)
 *   p <  n, on_mask_f is MASKED and items_in[b][p] == 1           1        (MASK_ID)
 *   otherwise                                                     value + 10  (NUM_RESERVED_TOKENS)
 * items_in int64 [B][ld_items >= W] is the row the item builder has just written; it is read only to learn which positions are
 * [MASK] -- no draw is repeated here, so the two cannot disagree.  A row is a pure function of its item row and the data set:
 * independent of the batch, of the row's place in it and of the rank.
 * Nothing is range-checked on the device -- row_win against the table, a window against its sequence, an item against V, a
 * value against the feature's vocabulary: the caller's (cloze_batches.DeviceCloze checks all of them on the host, once).
 *
 * b4c_batch_features: ONE launch for all features, one workgroup per batch row.  src, kind, on_mask and out are HOST arrays of
 *   n_feat device pointers / codes (the form of b4c_chain_ids); they travel by value in the kernel's arguments.  V: the entries
 *   of an ITEM table (> 0 when a feature is one; otherwise unused).  Every refusal -- null pointers, n_feat, W outside 1 .. 1021,
 *   a pitch below W, an unknown layout / kind / on_mask code, a missing table pointer in the layouts CLOZE and NEXT_TRAIN,
 *   holdout < 1 in the next-item layouts, max_len < 1 in NEXT_EVAL, B < 0 -- is B4C_EINVAL before any launch; B == 0 launches
 *   nothing.
 * b4c_batch_features_row: the same rule for ONE row and ONE feature on the host, into host arrays -- seq = s_g (n_g items),
 *   seq_off = offsets[g]; (a, L) the window (ignored for NEXT_EVAL); src the WHOLE source array (EVENT: [n_items], read at
 *   seq_off + first + p; ITEM: [V], an item outside [0, V) is refused); items_in int64 [W] the item row; out int64 [W];
 *   geom_out int32 [2] = (first, n). */
#define B4C_FEAT_EVENT 0
#define B4C_FEAT_ITEM 1
#define B4C_FEAT_MASKED 0
#define B4C_FEAT_KEPT 1
#define B4C_FEAT_CLOZE 0
#define B4C_FEAT_NEXT_TRAIN 1
#define B4C_FEAT_NEXT_EVAL 2
int b4c_batch_features(const int32_t *items, const int64_t *offsets, const int32_t *win_seq, const int32_t *win_start,
                       const int32_t *win_len, const int32_t *row_win /* may be NULL */, int B, int W, int layout, int holdout, int max_len,
                       int V, const int64_t *items_in, int ld_items, int n_feat, const int32_t *const *src, const int *kind,
                       const int *on_mask, int64_t *const *out, int ld_out, void *stream);
int b4c_batch_features_row(const int32_t *seq, int n_g, int64_t seq_off, int a, int L, int W, int layout, int holdout, int max_len, int V,
                           const int32_t *src, int kind, int on_mask, const int64_t *items_in, int64_t *out, int32_t *geom_out);

/* ==== sampled-negative training, the extended forward (additive to ABI 12): BPR, a weighted target term for the binary
 * cross-entropy (gSASRec's gBCE) and a per-item score correction (the sampled-softmax logQ correction) for the loss over a per-row
 * candidate list.  The operands, the list conventions and the backward are those of b4c_candidate_loss_fwd / _bwd ============== */

/* ---- the definition ----------------------------------------------------------------------------------------------------------
 * h, table, rows, row_off, bias, cand, R, C, V, K, dtype, item_loss, g, scores, stream: exactly those of b4c_candidate_loss_fwd
 *       (above), with its conventions: an entry < 0 or >= V is ABSENT (no term, coefficient exactly 0); a row whose
 *       column 0 is absent is IGNORED (nothing of it is read past column 0, loss 0, g = 0, scores = NaN); every present position is
 *       its own term, a repeated id is not merged; R == 0 is a no-op.
 * Score: s_c = sum_k h[k] * w_c[k] + bias[c], exactly the score of b4c_candidate_loss_fwd.
 * corr  fp32 [V] or NULL, read only at present entries.  The CORRECTED score is
 *           z_c = s_c - corr[id_c]      at every present entry c >= 1
 *           z_0 = s_0 - corr[id_0]      when flags has B4C_CANDX_CORR_TARGET, else z_0 = s_0
 *       one more fp32 subtraction on s; corr == NULL: z = s everywhere.  With corr[v] = log(expected count of v in a drawn list)
 *       this is the logQ correction of the sampled softmax; the target is in its list with probability 1, hence the flag.
 *       scores, when given, still receives the UNCORRECTED s.  dz / ds = 1: g is the derivative by z AND by s, and
 *       b4c_candidate_loss_bwd consumes it unchanged.
 * kind  B4C_CANDX_BCE:     l = beta * softplus(-z_0) + sum_{c >= 1 present} softplus(z_c)
 *                          g_0 = beta * (sigma(z_0) - 1) = -(beta * sigma(-z_0)),  g_c = sigma(z_c)
 *                          beta finite and >= 0 (gSASRec's generalised BCE; beta = 1: SASRec's)
 *       B4C_CANDX_SOFTMAX: l = logsumexp_{present c} z_c - z_0 (max-subtracted);  g_c = p_c - [c == 0];  beta is ignored
 *       B4C_CANDX_BPR:     l = sum_{c >= 1 present} softplus(z_c - z_0);  g_c = sigma(z_c - z_0),  g_0 = -sum_c g_c;  beta is ignored.
 *                          A row with no present negative (C == 1 included): loss and every coefficient exactly 0.
 *       softplus(x) = max(x, 0) + log1p(exp(-|x|)) and sigma in their stable forms; expf, log1pf and logf, not the fast intrinsics.
 * With kind BCE or SOFTMAX, beta == 1, corr == NULL and flags == 0 the result is bit for bit that of b4c_candidate_loss_fwd --
 * item_loss, g, scores and the untouched padding: the two entries launch one kernel.
 * The model loss is sum_r l_r / max(#rows with a present target, 1), formed by the caller.
 *
 * B4C_EINVAL before any launch: everything b4c_candidate_loss_fwd refuses (null pointers, K, C, a pitch below its width -- ld_g
 * and ld_s below C included --, a misaligned operand, dtype), a kind outside 0 .. B4C_CANDX_KINDS - 1, flags with an unknown
 * bit, B4C_CANDX_CORR_TARGET without corr, a beta that is negative or not finite. */
#define B4C_CANDX_BCE 0
#define B4C_CANDX_SOFTMAX 1
#define B4C_CANDX_BPR 2
#define B4C_CANDX_KINDS 3   /* kinds are 0 .. B4C_CANDX_KINDS - 1 */
#define B4C_CANDX_CORR_TARGET 1   /* flags bit: the target's score is corrected too */
int b4c_candidate_loss_fwd_ex(const void *h, int ld_h, const float *table, int ld_t, int64_t rows, int64_t row_off,
                              const float *bias, const int32_t *cand, int ld_c, int64_t R, int C, int V, int K, int dtype, int kind,
                              float beta, const float *corr /* may be NULL */, int flags, float *item_loss, float *g, int ld_g,
                              float *scores /* may be NULL */, int ld_s, void *stream);

/* ==== the masked-query attention entry points that take flags (additive to ABI 12): the causal (left-to-right) form of the last
 * encoder layer evaluated at a few query rows per sequence.  The operands and layouts are those of b4c_attn_mq_fwd_drop /
 * b4c_attn_mq_bwd_drop; the flag bit is B4C_ATTN_CAUSAL ========================================================================= */

/* b4c_attn_mq_fwd_drop / b4c_attn_mq_bwd_drop with a trailing `flags`.  flags == 0 reaches exactly the launches of those entry
 * points; an unknown flag bit is B4C_EINVAL; B4C_ATTN_CAUSAL with q_rows == NULL is B4C_EINVAL at any rate.
 * B4C_ATTN_CAUSAL: query row r of sequence b sits at position p = q_rows[r] - cu_seqlens[b] and sees the keys 0 .. p of its
 * sequence.  Over the visible keys
 *   P[r][k] = softmax_{k <= p}(q_r . k / sqrt(dh) + pad[k] * -1e9),   lse[r] = the log-sum-exp over the visible keys,
 * and the keys behind p are excluded outright (-inf, not -1e9): exactly zero weight and exactly zero gradient whatever the padding
 * or the (finite) k | v rows behind p look like; the kernels do not read the key rows behind the largest position of a query chunk
 * (fp32: 16 rows) or tile (bf16: 32 rows).  p >= the sequence's length sees every key.
 * Dropout: for every visible pair, the bit b4c_attn_keep(seed, b, h, p, k, H, max_len, rate) that the full causal layer
 * (b4c_attn_fwd_ex) draws for that (b, h, p, k).
 * A query row inside a sequence's range with q_rows[r] < cu_seqlens[b] (the -1 of an unused slot) has no visible key: its o row is
 * exactly 0, its lse 0, its dq row exactly 0, and it adds exactly nothing to dk | dv; nothing is NaN in either direction.  (The
 * launches without the flag keep treating such a slot as a query over every key.)
 * A query whose visible keys are all padded (leading pads only) comes out finite; its value is not otherwise pinned, as in
 * b4c_attn_fwd_ex.
 * b4c_attn_mq_bwd_ex writes every token row of dkv, as b4c_attn_mq_bwd does: the rows behind a sequence's last query position and
 * the rows of a sequence without a query are exact zeros.
 * Not covered: general [Sq][Sk] masks. */
int b4c_attn_mq_fwd_ex(const void *q, int ld_q, const void *kv, int ld_kv, const uint8_t *key_pad, const int32_t *cu_seqlens,
                       const int32_t *q_offsets, void *o, int ld_o, float *lse, int B, int max_len, int H, int dh, int dtype,
                       void *stream, const int32_t *q_rows, float dropout_rate, uint64_t seed, uint32_t flags);
int b4c_attn_mq_bwd_ex(const void *q, int ld_q, const void *kv, int ld_kv, const uint8_t *key_pad, const int32_t *cu_seqlens,
                       const int32_t *q_offsets, const void *o, int ld_o, const void *d_o, int ld_do, const float *lse,
                       void *dq, int ld_dq, void *dkv, int ld_dkv, int B, int max_len, int H, int dh, int dtype, void *stream,
                       const int32_t *q_rows, float dropout_rate, uint64_t seed, uint32_t flags);

/* ==== pre-LN encoder blocks (additive to ABI 12): the backward of a pre-LN encoder half's input norm -- the LayerNorm backward of
 * the sublayer-input gradient with the residual stream's gradient added as it is stored.
 *
 * A pre-LN half is  x' = x + drop(sublayer(LN(x; gamma, beta))).  With g the gradient of x' and dn the gradient of the normalised
 * rows that the sublayer's backward leaves,  dx = g + LNbwd(dn; x, stats, gamma):  the forward needs no kernel of its own
 * (b4c_layernorm_fwd, b4c_gemm_nt_add_ln / b4c_add_dropout_layernorm_fwd with the NEXT norm's gamma / beta), this sum does. ===== */

/* dx[row][j] = res[row][j] + rstd * (a - mean_j(a) - xhat * mean_j(a * xhat)),  a = dout * gamma, xhat = (x - mean) * rstd from the
 * saved stats [rows][2] = {mean, rstd}: b4c_layernorm_bwd (gate == NULL) with `res` added in fp32 before the one rounding of the
 * store.  dout, x, dx: [rows][d] contiguous; res: [rows][d] with pitch ld_res elements (>= d, a multiple of 8; 16-byte aligned),
 * required.  dgamma += sum_rows dout * xhat, dbeta += sum_rows dout (fp32 [d], ADDED to) through per-workgroup sums in the
 * workspace (b4c_layernorm_bwd_add_workspace_bytes, required), added in a fixed order: no float atomics, the same bits on every
 * launch, and the bits of b4c_layernorm_bwd on the same operands.  res == 0 everywhere gives b4c_layernorm_bwd's dx bit for bit.
 * fp32 and bf16; d a multiple of 8, <= 1024; rows is a 64-bit count.  dx must not overlap an input.  Bad arguments: B4C_EINVAL,
 * nothing is launched. */
int64_t b4c_layernorm_bwd_add_workspace_bytes(int64_t rows, int d);
int b4c_layernorm_bwd_add(const void *dout, const void *x, const float *stats, const float *gamma, const void *res, int ld_res,
                          void *dx, float *dgamma, float *dbeta, int64_t rows, int d, void *workspace, int64_t workspace_bytes,
                          int dtype, void *stream);

/* The same with dout = A . Bt^T formed in the kernel (matrix cores), so that the sublayer-input gradient never reaches memory:
 *   dn = bf16(A . Bt^T)  -- the accumulator rounded to the bf16 value b4c_gemm_nt (act NONE, no bias) would have stored --
 *   dx = res + LNbwd(dn; x, stats, gamma),  dgamma += sum_rows dn * xhat,  dbeta += sum_rows dn.
 * A [M][K] (pitch lda), Bt [N][K] (pitch ldb: the dX operand of b4c_gemm_nt), x / dx [M][N] contiguous, res [M][N] with pitch
 * ld_res; bf16 only; N = d_model <= 256, N and K multiples of 8 (K covers 3 d and the padded dff); lda, ldb >= K, multiples of 8,
 * and a 128-row tile of either spans less than 2^30 bytes (b4c_gemm_nt's rule); every operand 16-byte aligned.  A workgroup
 * owns complete rows, so the two row sums of the LayerNorm backward are taken in its epilogue; taking this kernel or b4c_gemm_nt +
 * b4c_layernorm_bwd_add differs by the order of fp32 sums only.  Deterministic: per-workgroup dgamma / dbeta sums through the
 * workspace (b4c_gemm_nt_ln_bwd_add_workspace_bytes, required) in a fixed order.  Bad arguments: B4C_EINVAL, nothing is launched. */
int64_t b4c_gemm_nt_ln_bwd_add_workspace_bytes(int M, int N);
int b4c_gemm_nt_ln_bwd_add(const void *A, int lda, const void *Bt, int ldb, const void *x, const float *stats, const float *gamma,
                           const void *res, int ld_res, void *dx, float *dgamma, float *dbeta, int M, int N, int K, void *workspace,
                           int64_t workspace_bytes, int dtype, void *stream);

/* ==== the in-batch contrastive loss (additive to ABI 12): NT-Xent / InfoNCE over the rows of a batch; the auxiliary loss of
 * CL4SRec and DuoRec ============================================================================================================== */

/* No reference counterpart (the reference trains with the Cloze loss alone); the float64 restatement is tests/nce_ref.py, written
 * from the definition below.
 *
 * Definition.  z is [N][ld_z] of T (bf16 or fp32), K columns used; pos int32 [N]; group int32 [N] or NULL.
 *   Score     s_ij = inv_temp * (zh_i . zh_j), accumulated in fp32.  zh = z by default; with flags & B4C_NCE_COSINE
 *             zh_i = z_i * rnorm[i], rnorm[i] = 1 / max(||z_i||_2, 1e-12) (fp32, the norm of the stored values).  The scaling
 *             is applied to the fp32 score, not to the operands: s_ij = inv_temp * (rnorm[i] * rnorm[j]) * (z_i . z_j); for bf16
 *             the matrix-core operands are the stored values.  b4c_nce_fwd writes rnorm, b4c_nce_bwd reads it; it may be NULL
 *             without the flag.
 *   Live rows live(i) iff 0 <= pos[i] < N and pos[i] != i.  Only live rows are queries; every other row has item_loss = 0,
 *             lse = 0 and a dz contribution from being someone's positive only.
 *   Keys      key(i, j) iff j != i and at least one of
 *               j == pos[i];
 *               live(j) and (group == NULL or group[i] < 0 or group[j] < 0 or group[i] != group[j]).
 *             (DuoRec: two sequences with the same target item are not each other's negatives.)
 *   Forward   lse[i] = log sum_{j : key(i, j)} exp(s_ij), a max-shifted log-sum-exp in fp32;
 *             item_loss[i] = lse[i] - s_{i, pos[i]}.
 *   Backward  G_ij = [key(i, j)] exp(s_ij - lse[i]) - [j == pos[i]] for live i, else 0;
 *             dzh_i = gscale[0] * inv_temp * sum_j (G_ij + G_ji) zh_j;
 *             dz_i = dzh_i without the flag, rnorm[i] * (dzh_i - zh_i (zh_i . dzh_i)) with it.
 *             dz ([N][ld_dz] of T) is written, not accumulated.  pos need not be an involution: G_ji is evaluated from lse[j],
 *             pos[j] and group[j].  S is symmetric, so one score tile serves G and its transpose: one sweep of 4 N^2 K flops.
 *             bf16: the coefficient (G_ij + G_ji) * rnorm[j] (rnorm = 1 without the flag) is rounded to bf16, the operand of the
 *             second matrix-core product (a 32 x 32 block of scores that holds a -[j == pos[i]] term also adds the product with
 *             the rounding residual: its coefficients carry 16 bits); the sum over j is fp32 and dz is rounded once when stored.
 *   Deterministic: no atomics; a workgroup owns a tile of rows and walks the column tiles in ascending order, a row's sums are
 *             taken in an order that depends on N alone.  Two launches on the same inputs give the same bits.
 *
 * Limits: K % 8 == 0, 8 <= K <= 128; 0 <= N < 2^24; z, dz 16-byte aligned, rows included (ld % 8 == 0 for bf16, % 4 for fp32),
 * ld >= K, and all N * ld elements addressable (the tile loader reads whole 16-byte chunks of a row's pitch).
 * Checks, in this order and before any pointer is looked at: K, dtype, inv_temp (finite, > 0), flags (B4C_NCE_COSINE is the one
 * bit), N -- B4C_EINVAL with a message that names the argument; then N == 0 returns B4C_OK; then rnorm missing with the flag, the
 * other pointers, pitches and alignment.  Nothing is launched or written after a refusal. */
#define B4C_NCE_COSINE 1u   /* flags bit: cosine similarity (scores scaled by rnorm[i] * rnorm[j]) */
#define B4C_NCE_MAX_N 16777216   /* N < 2^24 */
int b4c_nce_fwd(const void *z, int ld_z, int64_t N, int K, int dtype, const int32_t *pos, const int32_t *group,
                float inv_temp, uint32_t flags, float *rnorm, float *lse, float *item_loss, void *stream);
int b4c_nce_bwd(const void *z, int ld_z, int64_t N, int K, int dtype, const int32_t *pos, const int32_t *group,
                float inv_temp, uint32_t flags, const float *rnorm, const float *lse, const float *gscale,
                void *dz, int ld_dz, void *stream);

/* ==== the contrastive views of a device-built batch (additive to ABI 12): CL4SRec's item crop, item mask and item reorder;
 * DuoRec's supervised positive, the row of another sequence in front of the same target item =================================== */

/* No reference counterpart (the reference trains with the Cloze loss alone); the integer restatement is tests/augment_ref.py,
 * written from the definition below.
 *
 * Definition.  The data set is b4c_batch_features' CSR pair (items int32 [n_tok], offsets int64 [n_seq + 1]) with the window table
 * (win_seq, win_start, win_len) and row_win int32 [B] (NULL: row b is window b; a negative entry, or a negative sequence or start
 * in the table: an empty row).  Row b's window is (g, a, L); o0 = offsets[g], n_g = offsets[g + 1] - o0.
 *   Source    src = s_g[first .. first + n), s_g = items + o0, by the row rule of b4c_batch_features for `layout`:
 *               B4C_FEAT_CLOZE       first = a, n = min(L, W): the UNMASKED window (holdout and max_len are not read for it);
 *               B4C_FEAT_NEXT_TRAIN  the input row of b4c_next_item_batch's TRAIN mode: T = max(n_g - holdout, 0),
 *                                    first = a > 0 ? a - 1 : 0, n = max(min(a > 0 ? L : L - 1, W, T - first - 1), 0).
 *             i = o0 + first is the CSR index of the row's first token.
 *   Random    rand64 = b4c_rand64 (Threefry-2x32, 12 rounds: key, counter).  For view v = 0 .. n_views - 1:
 *               seed_v = rand64(seed ^ 0xA0761D6478BD642F, v);
 *               h_op   = rand64(seed_v ^ 0xE7037ED1A0B428DB, i);   h_at = rand64(seed_v ^ 0x8EBC6AF09C88C6E3, i);
 *               k_p    = rand64(seed_v, (i << 10) | p), the key of position p of the row.
 *             mulhi(x, m) = the high 64 bits of the 128-bit product x * m (uniform in [0, m)).  (k_p, p) < (k_q, q) is
 *             lexicographic: ties of the key go to the lower position.  "(int)((float)n * r)" is a float32 product of the float32
 *             n and r, then truncation.  Ids: out = item + 10, [MASK] = 1, pad = 0.
 *   A row and a view write items_out[v][b][0 .. W), src_tok[v][b][0 .. W) (the CSR index of the token each output position came
 *   from), n_out[v][b], op_out[v][b], target_out[v][b]:
 *   1. Empty  n = 0 (an empty row, an empty window): all pad, n_out = 0, op_out = 0, target_out = -1.
 *   2. Op     the bits set in ops_mask in ascending order are e_0 .. e_{m-1}; op = e_{mulhi(h_op, m)}; op_out = the op's bit.
 *   3. CROP   Lc = max(1, (int)((float)n * crop_ratio)), c = mulhi(h_at, n - Lc + 1); out[p] = src[c + p] + 10 for p < Lc;
 *             n_out = Lc.
 *   4. MASK   m = min(n, (int)((float)n * mask_ratio)); the positions of the m smallest (k_p, p), p in [0, n), are [MASK], the
 *             others src[p] + 10; n_out = n.
 *   5. REORDER  Lr = min(n, (int)((float)n * reorder_ratio)), r0 = mulhi(h_at, n - Lr + 1); for p in the span [r0, r0 + Lr):
 *             rho(p) = #{q in the span : (k_q, q) < (k_p, p)} and out[r0 + rho(p)] = src[p] + 10; outside the span
 *             out[p] = src[p] + 10; n_out = n.
 *   6. SAME_TARGET (B4C_FEAT_NEXT_TRAIN only)  t = i + n is the CSR index of the row's target (inside the training view by the
 *             row rule), y = items[t].  The index: tgt_first int64 [V + 1], tgt_tok int64 [n_tgt], tgt_seq int32 [n_tgt]; y's
 *             list is tgt_tok[tgt_first[y] .. tgt_first[y + 1]), CSR indices of tokens that hold y, ascending, cnt entries (y
 *             outside [0, V): an empty list); tgt_seq[k] is the sequence of token tgt_tok[k].  own = the number of entries of
 *             the list below t (its lower-bound position), found = (t is in the list), others = cnt - found.
 *             others = 0: the view is the row's own inputs, out[p] = src[p] + 10, n_out = n, and self_count[0] is incremented
 *             (DuoRec's fallback).  Otherwise u = mulhi(h_at, others), k = tgt_first[y] + u + (found && u >= own ? 1 : 0),
 *             j = tgt_tok[k], g' = tgt_seq[k], q = j - offsets[g'] (the items of g' in front of its y);
 *             n_out = min(q, W, max_len) (max_len <= 0: no cap) and out[p] = s_g'[q - n_out + p] + 10 for p < n_out: the most
 *             recent n_out items in front of the partner's target.
 *   7. Every op  out[p] = 0 and src_tok = -1 for n_out <= p < W.  target_out = items[i + n] for B4C_FEAT_NEXT_TRAIN, -1 for
 *             B4C_FEAT_CLOZE.  src_tok follows the same moves (CROP: i + c + p; REORDER: i + the source position; SAME_TARGET:
 *             offsets[g'] + q - n_out + p or i + p); a [MASK] position keeps its source token.
 *   A row is a pure function of (seed, v, the window): not of its place in the batch, nor of B or n_views.
 *
 * b4c_augment_views: one 256-thread workgroup per (row, view), grid (B, n_views).  items_out int64 [n_views][B][ld_items];
 * src_tok int64 [n_views][B][ld_src] or NULL; n_out, op_out int32 [n_views][B]; target_out int32 [n_views][B] or NULL;
 * self_count int32 [1], set to 0 by the entry before the launch and incremented once per self row (required with
 * B4C_AUG_SAME_TARGET, else it may be NULL).  Stream-ordered; nothing is read back; neither the rows nor the index are checked
 * against the data set.
 * Checks, in this order and before any pointer is looked at -- B4C_EINVAL with a message that names the argument: B and W
 * (1 .. B4C_MAX_BATCH_WIDTH), layout (one of the three B4C_FEAT_* row layouts), holdout (NEXT_TRAIN: >= 0), ld_items >= W, layout
 * once more (B4C_FEAT_NEXT_EVAL: views of evaluation rows are not built), n_views (1 .. B4C_AUG_MAX_VIEWS), ops_mask (a non-empty
 * subset of the four bits), crop_ratio in (0, 1], mask_ratio and reorder_ratio in [0, 1] (a NaN or an infinity is outside),
 * B4C_AUG_SAME_TARGET with another layout than NEXT_TRAIN, ld_src >= W (src_tok given); then B == 0 returns B4C_OK;
 * then the index missing with B4C_AUG_SAME_TARGET (tgt_first, tgt_tok, tgt_seq, V > 0, self_count), then the other pointers.  Nothing is launched or written after a refusal.
 *
 * b4c_augment_row: the same rule for ONE (row, view) on the host, from the same functions; every pointer is a HOST pointer.
 * items / offsets: the whole CSR pair (n_seq sequences); (g, a, L): the window, g < 0: an empty row; out int64 [W];
 * src_tok_out int64 [W]; head_out int32 [4] = {n_out, op, target, self (1: a same-target row that fell back to itself)}. */
#define B4C_AUG_CROP 1u         /* ops_mask / op_out bits */
#define B4C_AUG_MASK 2u
#define B4C_AUG_REORDER 4u
#define B4C_AUG_SAME_TARGET 8u
#define B4C_AUG_MAX_VIEWS 4
int b4c_augment_views(const int32_t *items, const int64_t *offsets, const int32_t *win_seq, const int32_t *win_start,
                      const int32_t *win_len, const int32_t *row_win, int B, int W, int layout, int holdout, int max_len,
                      int n_views, uint32_t ops_mask, float crop_ratio, float mask_ratio, float reorder_ratio, uint64_t seed,
                      const int64_t *tgt_first, const int64_t *tgt_tok, const int32_t *tgt_seq, int V, int64_t *items_out,
                      int ld_items, int64_t *src_tok, int ld_src, int32_t *n_out, int32_t *op_out, int32_t *target_out,
                      int32_t *self_count, void *stream);
int b4c_augment_row(const int32_t *items, const int64_t *offsets, int64_t n_seq, int64_t g, int a, int L, int W, int layout,
                    int holdout, int max_len, int view, uint32_t ops_mask, float crop_ratio, float mask_ratio,
                    float reorder_ratio, uint64_t seed, const int64_t *tgt_first, const int64_t *tgt_tok, const int32_t *tgt_seq,
                    int V, int64_t *out, int64_t *src_tok_out, int32_t *head_out);

/* ==== long-sequence attention (additive to ABI 12): bf16 matrix-core self-attention for sequences longer than the resident
 * kernels of b4c_attn_fwd_ex / b4c_attn_bwd_ex hold (S <= 512, all K and V of a (sequence, head) in LDS): the keys are streamed == */

/* Arguments, layouts and semantics are exactly those of b4c_attn_fwd_ex / b4c_attn_bwd_ex with dtype = B4C_BF16:
 *   qkv [rows][ld_qkv] = Q | K | V of H heads of depth dh; key_pad uint8 [rows] (1 = padded key); cu_seqlens NULL: dense, B
 *   sequences of S rows each; else int32 [B + 1], sequence b owns rows cu_seqlens[b] .. cu_seqlens[b + 1] and S is max_len, an
 *   upper bound of the longest one.  o [rows][ld_o]; lse, delta fp32 [B][H][S] (delta is scratch of the backward);
 *   dqkv [rows][ld_dqkv] is written, not accumulated.
 *   A padded key adds -1e9 to its score (a sequence without a live key: uniform weights over all its keys); flags &
 *   B4C_ATTN_CAUSAL: key k is visible to query q iff k <= q, the others get exactly zero weight and zero gradient.
 *   dropout_rate in [0, 1): keep rule b4c_attn_keep(seed, b, h, q, k, H, S, rate), lse is that of the undropped softmax.
 *   The dK / dV rows of padded keys are exact zeros.
 * Rounding: P is rounded to bf16 once, in front of P V; o once, when stored; lse is fp32.  Backward: P and dS once each in front
 *   of their products, dQ once after the fp32 sum over all key blocks (workspace), dK / dV once.
 * Deterministic: no atomics, no workgroup waits for another; two launches on the same inputs give the same bits.
 *
 * Limits: head depth 32 or 64; 1 <= S <= B4C_ATTN_LONG_MAX_S; pitches multiples of 8 elements, rows 16-byte aligned.
 * b4c_attn_long_bwd needs a workspace of b4c_attn_long_bwd_workspace_bytes(rows, H, dh) = rows * H * dh * 4 bytes, rows = B * S
 * (dense) or cu_seqlens[B] (packed): the fp32 dQ accumulator.  (-1 for arguments outside the limits.)
 * Checks, in this order and before any pointer is looked at: flags, dropout_rate, head depth, S, the other shape arguments and
 * the pitches, workspace_bytes (backward, dense layout: against B * S rows; the packed layout's row count lives on the device and
 * is the caller's to size for) -- B4C_EINVAL with a message that names the argument; then the pointers.  Nothing is launched or
 * written after a refusal. */
#define B4C_ATTN_LONG_MAX_S 2048
int b4c_attn_long_fwd(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, void *o, int ld_o,
                      float *lse, int B, int S, int H, int dh, void *stream, float dropout_rate, uint64_t seed, uint32_t flags);
int64_t b4c_attn_long_bwd_workspace_bytes(int64_t rows, int H, int dh);
int b4c_attn_long_bwd(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, const void *o, int ld_o,
                      const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv, int B, int S, int H,
                      int dh, void *workspace, int64_t workspace_bytes, void *stream, float dropout_rate, uint64_t seed,
                      uint32_t flags);

#ifdef __cplusplus
}
#endif

#endif /* B4C_H */
