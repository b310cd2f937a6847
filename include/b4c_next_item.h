/* b4c_next_item.h -- next-item batches built on the device: every real position of a left-to-right row predicts the item that
 * follows it, each target against its own negatives, none of them an item of the user's.  An ADD-ON header of include/b4c.h
 * (which includes it; a caller includes b4c.h).  Additive to ABI 12: no signature of b4c.h, of its extension header or of another
 * add-on changed, b4c_abi_version() stays 12.  The error codes, B4C_MAX_EXCL and B4C_MAX_CAND are b4c.h's.
 * (The ctypes binding reads the add-on headers beside b4c.h: bert4clickpath_amd/_lib.py, ADDON_HEADER_PATHS.) */
#ifndef B4C_NEXT_ITEM_H
#define B4C_NEXT_ITEM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule ----------------------------------------------------------------------------------------------------------------
 * Data: the CSR data set of the Cloze batches (b4c.h, "Cloze batches"): items int32 [n_items] label-space indices, offsets int64
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

#ifdef __cplusplus
}
#endif
#endif /* B4C_NEXT_ITEM_H */
