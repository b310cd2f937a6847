/* b4c_batch_features.h -- side features beside the items of a device-built batch: for every row that b4c_cloze_batch_windows or
 * b4c_next_item_batch has just written, the ids of up to B4C_MAX_FEATURES further embedded features (an action per event, a
 * category per item, ...), masked where the item row is and the feature would give the target away.  An ADD-ON header of
 * include/b4c.h (which includes it; a caller includes b4c.h).  Additive to ABI 12: no signature of b4c.h, of its extension header
 * or of another add-on changed, b4c_abi_version() stays 12.  The error codes and B4C_MAX_FEATURES are b4c.h's.
 * (The ctypes binding reads the add-on headers beside b4c.h: bert4clickpath_amd/_lib.py, ADDON_HEADER_PATHS.) */
#ifndef B4C_BATCH_FEATURES_H
#define B4C_BATCH_FEATURES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the rule ----------------------------------------------------------------------------------------------------------------
 * Data: the CSR data set of the Cloze batches (b4c.h, "Cloze batches"): items int32 [n_items] label-space indices, offsets int64
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
 *   B4C_FEAT_CLOZE       b4c_cloze_batch_windows' row (b4c.h): w = row_win[b] names a window of the table (win_seq, win_start,
 *                        win_len): g = win_seq[w], first = win_start[w], n = clamp(win_len[w], 0, W).  TRAIN and EVAL rows alike
 *                        (an evaluation row is a window that ends at its target).
 *   B4C_FEAT_NEXT_TRAIN  the TRAIN row of b4c_next_item.h: the window (g, a, L) as above, T_g = max(n_g - holdout, 0):
 *                        first = a > 0 ? a - 1 : 0,  n = a > 0 ? L : max(L - 1, 0), cut at W and at T_g - first - 1.
 *   B4C_FEAT_NEXT_EVAL   the EVAL row of b4c_next_item.h: w = row_win[b] names SEQUENCE g = w (the table is not read),
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

#ifdef __cplusplus
}
#endif
#endif /* B4C_BATCH_FEATURES_H */
