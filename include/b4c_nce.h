/*
 * b4c_nce.h -- extension header of libb4c_hip.so: the in-batch contrastive loss (NT-Xent / InfoNCE over the rows of a batch; the
 * auxiliary loss of CL4SRec and DuoRec).
 *
 * Why a second header: include/b4c.h is one ABI version (B4C_ABI_VERSION) with one signature table, and both are frozen while
 * this family is added; an extension carries its own version (B4C_NCE_VERSION, b4c_nce_version()) so that neither moves.  The
 * grammar, the conventions (device pointers, the caller's stream, no allocation, 0 or a negative B4C_E* code, b4c_last_error())
 * and the constants (B4C_F32 / B4C_BF16, B4C_OK, B4C_EINVAL) are those of b4c.h, which this header includes.  A C caller:
 *     #include "b4c.h"
 *     #include "b4c_nce.h"
 * and links the same libb4c_hip.so.  No name is declared in both headers.
 *
 * No reference counterpart (the reference trains with the Cloze loss alone); the float64 restatement is tests/nce_ref.py, written
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
 * other pointers, pitches and alignment.  Nothing is launched or written after a refusal.
 */
#ifndef B4C_NCE_H
#define B4C_NCE_H

#include <stdint.h>

#include "b4c.h"

#ifdef __cplusplus
extern "C" {
#endif

#define B4C_NCE_VERSION 1   /* what b4c_nce_version() returns */
#define B4C_NCE_COSINE 1u   /* flags bit: cosine similarity (scores scaled by rnorm[i] * rnorm[j]) */
#define B4C_NCE_MAX_N 16777216   /* N < 2^24 */

int b4c_nce_version(void);
int b4c_nce_fwd(const void *z, int ld_z, int64_t N, int K, int dtype, const int32_t *pos, const int32_t *group,
                float inv_temp, uint32_t flags, float *rnorm, float *lse, float *item_loss, void *stream);
int b4c_nce_bwd(const void *z, int ld_z, int64_t N, int K, int dtype, const int32_t *pos, const int32_t *group,
                float inv_temp, uint32_t flags, const float *rnorm, const float *lse, const float *gscale,
                void *dz, int ld_dz, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* B4C_NCE_H */
