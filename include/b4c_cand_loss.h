/* b4c_cand_loss.h -- sampled-negative training: the loss over a per-row candidate list and its backward.  An ADD-ON header of
 * include/b4c.h (which includes it; a caller includes b4c.h).  Additive to ABI 12: no signature of b4c.h or of its extension
 * header changed, b4c_abi_version() stays 12.  The error codes (B4C_EINVAL, ...), the dtype codes and B4C_MAX_CAND are b4c.h's.
 * (The ctypes binding reads the add-on headers beside b4c.h: bert4clickpath_amd/_lib.py, ADDON_HEADER_PATHS.) */
#ifndef B4C_CAND_LOSS_H
#define B4C_CAND_LOSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* B4C_CAND_LOSS_H */
