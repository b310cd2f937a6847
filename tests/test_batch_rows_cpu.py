"""The batch builders agree on what a row is (csrc/batch_rows.h), checked through their host rule entries, no GPU: a side feature
that copies the items ('event' source = the data set's items, on_mask 'keep') must come out as the item row the next-item builder
writes for the same window or sequence, column for column, at widths below, at and above the window length."""
import numpy as np
import pytest

import next_item_ref as ref

MAX_LEN = 5


def _windows(lengths, holdout):
    from bert4clickpath_amd.cloze_batches import window_table
    w = window_table(lengths, MAX_LEN, MAX_LEN, holdout)
    return list(zip(w.seq.tolist(), w.start.tolist(), w.len.tolist())) + [(4, 0, 0)]       # and a window without items


@pytest.mark.parametrize('W', [1, 5, 8])
@pytest.mark.parametrize('holdout', [1, 2])
def test_feature_rows_are_the_next_item_rows_and_the_cloze_windows(W, holdout):
    from bert4clickpath_amd import ops
    items, offsets, V = ref.case_data()
    blank = np.zeros(W, np.int64)
    some = 0
    for g, a, L in _windows(np.diff(offsets), holdout):
        seq, off = items[offsets[g]:offsets[g + 1]], offsets[g]
        row = ops.next_item_row_host(seq, off, W, ops.NEXT_TRAIN, V, a, L, holdout, MAX_LEN)
        out, first, n = ops.batch_features_row_host(seq, off, W, ops.FEAT_NEXT_TRAIN, items, 'event', 'keep', blank, a=a, L=L,
                                                    holdout=holdout, max_len=MAX_LEN)
        assert n == row['n_in'] and np.array_equal(out, row['inputs']), (g, a, L)
        some += n > 0
        out, first, n = ops.batch_features_row_host(seq, off, W, ops.FEAT_CLOZE, items, 'event', 'keep', blank, a=a, L=L)
        assert (first, n) == (a, min(L, W)), (g, a, L)
        assert np.array_equal(out[:n], items[off + a:off + a + n].astype(np.int64) + 10) and not out[n:].any()
    assert some > 10
    for g in range(len(offsets) - 1):                              # EVAL rows: holdout is the drop
        seq, off = items[offsets[g]:offsets[g + 1]], offsets[g]
        row = ops.next_item_row_host(seq, off, W, ops.NEXT_EVAL, V, holdout=holdout, max_len=MAX_LEN)
        out, first, n = ops.batch_features_row_host(seq, off, W, ops.FEAT_NEXT_EVAL, items, 'event', 'keep', blank, holdout=holdout,
                                                    max_len=MAX_LEN)
        assert n == row['n_in'] and np.array_equal(out, row['inputs']), g
