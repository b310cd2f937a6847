"""Host restatement of the side-feature rule (include/b4c.h, "the rule"), in numpy and Python integers, written from
the header's text.  Used by test_batch_features_cpu.py and test_gpu_batch_features.py.  Every real position asserts that the item
row holds [MASK] or the item the geometry points at: a geometry that disagrees with the item builder's fails here instead of
gathering from the wrong place."""
import numpy as np

import next_item_ref as nref

EVENT, ITEM = 0, 1
MASKED, KEPT = 0, 1
CLOZE, NEXT_TRAIN, NEXT_EVAL = 0, 1, 2
RESERVED, MASK_ID, PAD = 10, 1, 0
KINDS = {'event': EVENT, 'item': ITEM}
ON_MASK = {'mask': MASKED, 'keep': KEPT}


def geometry(layout, n_g, a=0, L=0, holdout=1, max_len=None, W=1021):
    """-> (first, n) of a row: the window (a, L) of a sequence of n_g items (NEXT_EVAL: the sequence alone)"""
    max_len = 1021 if max_len is None else max_len
    if layout == CLOZE:
        return a, max(min(L, W), 0)
    if layout == NEXT_TRAIN:
        T = max(n_g - holdout, 0)
        first = a - 1 if a > 0 else 0
        n = L if a > 0 else max(L - 1, 0)
        return first, max(min(n, W, T - first - 1), 0)
    assert layout == NEXT_EVAL
    t = n_g - holdout
    if t < 1:
        return 0, 0
    n = min(t, max_len, W)
    return t - n, n


def one_row(items, offsets, g, first, n, W, src, kind, on_mask, items_in):
    """-> int64 [W]: one feature of one row.  items_in: the item row, int64 [>= W]"""
    out = np.full(W, PAD, np.int64)
    for p in range(n):
        i = int(offsets[g]) + first + p
        assert i < int(offsets[g + 1]), 'the row leaves its sequence'
        assert int(items_in[p]) in (MASK_ID, int(items[i]) + RESERVED), (g, first, p, int(items_in[p]), int(items[i]))
        if on_mask == MASKED and int(items_in[p]) == MASK_ID:
            out[p] = MASK_ID
        else:
            out[p] = int(src[i] if kind == EVENT else src[int(items[i])]) + RESERVED
    assert (np.asarray(items_in[n:W]) == PAD).all(), 'the item row is longer than the geometry says'
    return out


def batch(items, offsets, layout, row_idx, W, items_in, sources, windows=None, holdout=1, max_len=None):
    """The features of the rows row_idx -- CLOZE / NEXT_TRAIN: indices into windows = (seq, start, len); NEXT_EVAL: sequences;
    negative: an empty row; None: row b is window b.  sources: [(src, kind code, on_mask code)].  -> [int64 [B, W] per source]"""
    items_in = np.asarray(items_in)
    B = items_in.shape[0]
    row_idx = np.arange(B) if row_idx is None else np.asarray(row_idx, np.int64)
    outs = [np.full((B, W), PAD, np.int64) for _ in sources]
    for b, w in enumerate(row_idx.tolist()):
        if w < 0:
            assert (items_in[b, :W] == PAD).all()
            continue
        g, a, L = (w, 0, 0) if layout == NEXT_EVAL else (int(windows[0][w]), int(windows[1][w]), int(windows[2][w]))
        first, n = geometry(layout, int(offsets[g + 1] - offsets[g]), a, L, holdout, max_len, W)
        for out, (src, kind, on_mask) in zip(outs, sources):
            out[b] = one_row(items, offsets, g, first, n, W, src, kind, on_mask, items_in[b])
    return outs


def case_data():
    """next_item_ref.case_data() with a seeded event column (7 actions) and a seeded item table (23 categories) on top"""
    items, offsets, V = nref.case_data()
    rng = np.random.default_rng(41)
    return items, offsets, V, rng.integers(0, 7, len(items)).astype(np.int32), rng.integers(0, 23, V).astype(np.int32)


EVENT_SIZE, ITEM_SIZE = 7, 23
