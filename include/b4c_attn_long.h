/*
 * b4c_attn_long.h -- extension header of libb4c_hip.so: bf16 matrix-core self-attention for sequences longer than the resident
 * kernels of b4c_attn_fwd_ex / b4c_attn_bwd_ex hold (S <= 512, all K and V of a (sequence, head) in LDS): the keys are streamed.
 *
 * Why another header: include/b4c.h is one ABI version (B4C_ABI_VERSION) with one signature table, and both are frozen while this
 * family is added; an extension carries its own version (B4C_ATTN_LONG_VERSION, b4c_attn_long_version()) so that neither moves.
 * The grammar, the conventions (device pointers, the caller's stream, no allocation, 0 or a negative B4C_E* code,
 * b4c_last_error()) and the constants (B4C_OK, B4C_EINVAL, B4C_ATTN_CAUSAL) are those of b4c.h, which this header includes.
 * A C caller:
 *     #include "b4c.h"
 *     #include "b4c_attn_long.h"
 * and links the same libb4c_hip.so.  No name is declared in two headers.
 *
 * Arguments, layouts and semantics are exactly those of b4c_attn_fwd_ex / b4c_attn_bwd_ex (b4c.h) with dtype = B4C_BF16:
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
 * written after a refusal.
 */
#ifndef B4C_ATTN_LONG_H
#define B4C_ATTN_LONG_H

#include <stdint.h>

#include "b4c.h"

#ifdef __cplusplus
extern "C" {
#endif

#define B4C_ATTN_LONG_VERSION 1   /* what b4c_attn_long_version() returns */
#define B4C_ATTN_LONG_MAX_S 2048

int b4c_attn_long_version(void);
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

#endif /* B4C_ATTN_LONG_H */
