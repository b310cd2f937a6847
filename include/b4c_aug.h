/*
 * b4c_aug.h -- extension header of libb4c_hip.so: the contrastive views of a device-built batch (CL4SRec's item crop, item mask
 * and item reorder; DuoRec's supervised positive, the row of another sequence in front of the same target item).
 *
 * Why another header: include/b4c.h is one ABI version with one signature table and include/b4c_nce.h is one extension with its
 * own; both are frozen while this family is added.  This extension carries its own version (B4C_AUG_VERSION, b4c_aug_version()).
 * The grammar, the conventions (device pointers, the caller's stream, no allocation, 0 or a negative B4C_E* code,
 * b4c_last_error()) and the constants (B4C_FEAT_CLOZE / B4C_FEAT_NEXT_TRAIN, B4C_MAX_BATCH_WIDTH, B4C_OK, B4C_EINVAL) are those of
 * b4c.h, which this header includes.  A C caller:
 *     #include "b4c.h"
 *     #include "b4c_aug.h"
 * and links the same libb4c_hip.so.  No name is declared in two headers.
 *
 * No reference counterpart (the reference trains with the Cloze loss alone); the integer restatement is tests/augment_ref.py,
 * written from the definition below.
 *
 * Definition.  The data set is b4c_batch_features' CSR pair (items int32 [n_tok], offsets int64 [n_seq + 1]) with the window table
 * (win_seq, win_start, win_len) and row_win int32 [B] (NULL: row b is window b; a negative entry, or a negative sequence or start
 * in the table: an empty row).  Row b's window is (g, a, L); o0 = offsets[g], n_g = offsets[g + 1] - o0.
 *   Source    src = s_g[first .. first + n), s_g = items + o0, by the row rule of b4c.h for `layout`:
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
 * (1 .. B4C_MAX_BATCH_WIDTH), layout (one of b4c.h's three), holdout (NEXT_TRAIN: >= 0), ld_items >= W, layout once more
 * (B4C_FEAT_NEXT_EVAL: views of evaluation rows are not built), n_views (1 .. B4C_AUG_MAX_VIEWS), ops_mask (a non-empty subset of the four bits), crop_ratio in (0, 1], mask_ratio and reorder_ratio in
 * [0, 1] (a NaN or an infinity is outside), B4C_AUG_SAME_TARGET with another layout than NEXT_TRAIN, ld_src >= W (src_tok given);
 * then B == 0 returns B4C_OK; then the index missing with B4C_AUG_SAME_TARGET (tgt_first, tgt_tok, tgt_seq, V > 0, self_count),
 * then the other pointers.  Nothing is launched or written after a refusal.
 *
 * b4c_augment_row: the same rule for ONE (row, view) on the host, from the same functions; every pointer is a HOST pointer.
 * items / offsets: the whole CSR pair (n_seq sequences); (g, a, L): the window, g < 0: an empty row; out int64 [W];
 * src_tok_out int64 [W]; head_out int32 [4] = {n_out, op, target, self (1: a same-target row that fell back to itself)}.
 */
#ifndef B4C_AUG_H
#define B4C_AUG_H

#include <stdint.h>

#include "b4c.h"

#ifdef __cplusplus
extern "C" {
#endif

#define B4C_AUG_VERSION 1       /* what b4c_aug_version() returns */
#define B4C_AUG_CROP 1u         /* ops_mask / op_out bits */
#define B4C_AUG_MASK 2u
#define B4C_AUG_REORDER 4u
#define B4C_AUG_SAME_TARGET 8u
#define B4C_AUG_MAX_VIEWS 4

int b4c_aug_version(void);
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

#ifdef __cplusplus
}
#endif

#endif /* B4C_AUG_H */
