/* b4c_cand_loss_ex.h -- sampled-negative training, the extended forward: BPR, a weighted target term for the binary
 * cross-entropy (gSASRec's gBCE) and a per-item score correction (the sampled-softmax logQ correction) for the loss over a per-row
 * candidate list.  An ADD-ON header of include/b4c.h (which includes it; a caller includes b4c.h).  Additive to ABI 12: no
 * signature of b4c.h, of its extension header or of another add-on header changed, b4c_abi_version() stays 12.  The error codes,
 * the dtype codes and B4C_MAX_CAND are b4c.h's; the operands, the list conventions and the backward are b4c_cand_loss.h's.
 * (The ctypes binding reads the add-on headers beside b4c.h: bert4clickpath_amd/_lib.py, ADDON_HEADER_PATHS.) */
#ifndef B4C_CAND_LOSS_EX_H
#define B4C_CAND_LOSS_EX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the definition ----------------------------------------------------------------------------------------------------------
 * h, table, rows, row_off, bias, cand, R, C, V, K, dtype, item_loss, g, scores, stream: exactly those of b4c_candidate_loss_fwd
 *       (b4c_cand_loss.h), with its conventions: an entry < 0 or >= V is ABSENT (no term, coefficient exactly 0); a row whose
 *       column 0 is absent is IGNORED (nothing of it is read past column 0, loss 0, g = 0, scores = NaN); every present position is
 *       its own term, a repeated id is not merged; R == 0 is a no-op.
 * Score: s_c = sum_k h[k] * w_c[k] + bias[c], exactly the score of b4c_cand_loss.h.
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

#ifdef __cplusplus
}
#endif
#endif /* B4C_CAND_LOSS_EX_H */
