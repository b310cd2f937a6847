/* b4c_attn_mq_ex.h -- the masked-query attention entry points that take flags: the causal (left-to-right) form of the last encoder
 * layer evaluated at a few query rows per sequence.  An ADD-ON header of include/b4c.h (which includes it; a caller includes
 * b4c.h).  Additive to ABI 12: no signature of b4c.h, of its extension header or of another add-on header changed,
 * b4c_abi_version() stays 12.  The operands, layouts, error codes and dtype codes are b4c.h's (b4c_attn_mq_fwd_drop /
 * b4c_attn_mq_bwd_drop); the flag bit is B4C_ATTN_CAUSAL of b4c_attn_ex.h.  (The ctypes binding reads the add-on headers beside
 * b4c.h: bert4clickpath_amd/_lib.py, ADDON_HEADER_PATHS.) */
#ifndef B4C_ATTN_MQ_EX_H
#define B4C_ATTN_MQ_EX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* B4C_ATTN_MQ_EX_H */
