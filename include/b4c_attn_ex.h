/* b4c_attn_ex.h -- the attention entry points that take everything: an extension header of include/b4c.h (which includes it; a
 * caller includes b4c.h).  Additive to ABI 12: no signature of b4c.h changed, b4c_abi_version() stays 12.  The operands, the error
 * codes (B4C_EINVAL, ...) and the dtype codes are b4c.h's. */
#ifndef B4C_ATTN_EX_H
#define B4C_ATTN_EX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

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
 * The masked-query kernels (b4c_attn_mq_*) take the same flag through b4c_attn_mq_fwd_ex / b4c_attn_mq_bwd_ex (b4c_attn_mq_ex.h).
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

#ifdef __cplusplus
}
#endif
#endif /* B4C_ATTN_EX_H */
