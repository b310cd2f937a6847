"""Next-item batches, the parts that need no GPU (NO REFERENCE ORACLE: an extension -- the restatement is tests/next_item_ref.py):
the entry points' declarations and their binding, the argument checks that refuse a launch, the rule on the host (b4c_next_item_row) against the
restatement, and DeviceCloze's host side."""
import numpy as np
import pytest

import abi_pin
import next_item_ref as ref

A = 1 << 20                                                       # a well-aligned, never dereferenced "pointer"
NAMES = ('b4c_next_item_batch', 'b4c_next_item_row')


def test_header_declares_the_entry_points_and_they_are_bound():
    from bert4clickpath_amd import _lib, ops
    c = _lib.ctypes
    lib = _lib.lib()
    declared = _lib.signatures()
    ptr, i32, i64, u64 = c.c_void_p, c.c_int, c.c_int64, c.c_uint64
    lists = {
        # (items, offsets, win_seq, win_start, win_len, row_win, row_off, B, W, mode, holdout, max_len, V, N, seed, excl, cdf, items_out,
        #  ld_items, flat_idx, labels, cand, ld_c, rows, short_count, stream)
        'b4c_next_item_batch': [ptr] * 7 + [i32] * 7 + [u64, i32, ptr, ptr, i32, ptr, ptr, ptr, i32, i64, ptr, ptr],
        # (seq, n_g, seq_off, a, L, W, mode, holdout, max_len, V, N, seed, excl, cdf, inputs_out, labels_out, pos_out, cand_out, ld_c,
        #  counts_out)
        'b4c_next_item_row': [ptr, i32, i64] + [i32] * 8 + [u64, i32, ptr, ptr, ptr, ptr, ptr, i32, ptr],
    }
    for name in NAMES:
        assert name in declared, name
        assert declared[name] == (c.c_int, lists[name]), name
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == lists[name] and getattr(lib, name).restype is c.c_int
    assert (ops.NEXT_TRAIN, ops.NEXT_EVAL) == (0, 1) and ops.NEXT_EXCLUDE == {None: 0, 'history': 1}
    assert _lib.ABI_VERSION == abi_pin.ABI_VERSION and lib.b4c_abi_version() == abi_pin.ABI_VERSION


def _launch(L, items=A, offsets=A, win_seq=A, win_start=A, win_len=A, row_win=A, row_off=A, B=4, W=8, mode=0, holdout=1, max_len=8, V=500,
            N=3, seed=1, excl=1, cdf=None, out=A, ld_items=8, flat=A, lab=A, cand=A, ld_c=4, rows=32, short=A):
    return L.b4c_next_item_batch(items, offsets, win_seq, win_start, win_len, row_win, row_off, B, W, mode, holdout, max_len, V, N, seed, excl,
                                 cdf, out, ld_items, flat, lab, cand, ld_c, rows, short, None)


BAD = [dict(items=None), dict(offsets=None), dict(win_seq=None), dict(win_start=None), dict(win_len=None), dict(row_off=None), dict(out=None),
       dict(flat=None), dict(lab=None), dict(cand=None), dict(short=None), dict(W=0), dict(W=1022, ld_items=1022), dict(B=-1), dict(N=-1),
       dict(N=1024, ld_c=1025), dict(V=0), dict(ld_items=7), dict(ld_c=3), dict(mode=2), dict(mode=-1), dict(excl=2), dict(excl=-1),
       dict(holdout=-1), dict(mode=1, holdout=0), dict(mode=1, max_len=0), dict(mode=1, row_win=None), dict(rows=-1),
       dict(B=1 << 22, W=1021, ld_items=1021)]


def test_bad_arguments_are_refused_without_a_launch():
    """(every call here would fault on its made-up pointers if it were launched, and there is no device to launch on)"""
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    for kw in BAD:
        assert _launch(L, **kw) == _lib._C['B4C_EINVAL'], kw
        assert b'next_item_batch' in L.b4c_last_error(), (kw, L.b4c_last_error())
    # nothing to do is not an error (and launches nothing); without negatives neither cand nor short_count is needed
    assert _launch(L, B=0, short=None, N=0) == 0
    assert _launch(L, B=0, N=0, cand=None, short=None, items=None) == 0


def test_host_wrappers_validate_before_the_device_is_needed():
    import torch
    from bert4clickpath_amd import ops
    it, off = torch.zeros(5, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    w = torch.zeros(1, dtype=torch.int32)
    ro = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ops.B4CError, match='int32'):
        ops.next_item_batch(it.long(), off, w, w, w, w, ro, 4, 0, 0, 10)
    with pytest.raises(ops.B4CError, match=r'\[B \+ 1\]'):
        ops.next_item_batch(it, off, w, w, w, w, ro[:1], 4, 0, 0, 10)
    with pytest.raises(ops.B4CError, match="'history' or None"):
        ops.next_item_batch(it, off, w, w, w, w, ro, 4, 0, 0, 10, exclude='window')
    with pytest.raises(ops.B4CError, match='num_negatives'):
        ops.next_item_batch(it, off, w, w, w, w, ro, 4, 0, 0, 10, num_negatives=1024)
    with pytest.raises(ValueError, match='rows = 2 for 3 targets'):
        ops.next_item_batch(it, off, w, w, w, w, ro, 4, 0, 3, 10, rows=2)
    with pytest.raises(ops.B4CError, match='HIP device only'):
        ops.next_item_batch(it, off, w, w, w, w, ro, 4, 0, 0, 10)


# ---- the rule on the host ---------------------------------------------------------------------------------------------------------
def _cdfs(V):
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 5, V)
    counts[::3] = 0                                               # zero-mass items
    return {'uniform': None, 'popularity': np.cumsum(counts).astype(np.int64), 'no_mass': np.zeros(V, np.int64)}


def _windows(lengths, max_len, stride, holdout):
    from bert4clickpath_amd.cloze_batches import window_table
    return window_table(lengths, max_len, stride, holdout)


@pytest.mark.parametrize('holdout', [1, 2])
@pytest.mark.parametrize('N, cdf', [(0, 'uniform'), (1, 'uniform'), (20, 'uniform'), (3, 'popularity'), (2, 'no_mass')])
def test_host_row_equals_the_restatement_on_every_train_window(holdout, N, cdf):
    from bert4clickpath_amd import ops
    items, offsets, V = ref.case_data()
    cdf = _cdfs(V)[cdf]
    win = _windows(np.diff(offsets), 5, 5, holdout)
    seen = set()
    for g, a, L in zip(*win):
        seq = items[offsets[g]:offsets[g + 1]]
        if g == 7 and a not in (0, 5, 50, 1090, 1094, 1095):   # the long sequence: a few windows are enough
            continue
        for exclude in ('history', None):
            want = ref.one_row(seq, offsets[g], ref.TRAIN, V, a, L, holdout, 5, 8, N, 77, exclude, cdf)
            got = ops.next_item_row_host(seq, offsets[g], 8, ops.NEXT_TRAIN, V, a, L, holdout, 5, N, 77, exclude, cdf)
            assert np.array_equal(got['inputs'], want['inputs']) and got['n_in'] == want['n_in'], (g, a, L)
            assert np.array_equal(got['labels'], want['labels']) and np.array_equal(got['pos'], want['pos']), (g, a, L)
            assert got['short'] == want['short'], (g, a, L)
            if N:
                assert np.array_equal(got['candidates'], want['candidates']), (g, a, L, exclude)
                if exclude == 'history':
                    neg = got['candidates'][:, 1:]
                    assert not (set(neg[neg >= 0].tolist()) & want['X'])
        seen.add((int(a > 0), min(int(L), 3)))
    assert {(0, 1), (0, 2), (0, 3), (1, 3)} <= seen               # L = 1, 2, more; a prepended input


def test_host_row_short_rows_and_the_cap_of_x():
    from bert4clickpath_amd import ops
    # V = 12, ten distinct items in the view: two items are left for three negatives
    seq = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 3, 11], np.int32)
    want = ref.one_row(seq, 40, ref.TRAIN, 12, 0, 11, 1, None, 16, 3, 5)
    got = ops.next_item_row_host(seq, 40, 16, ops.NEXT_TRAIN, 12, 0, 11, 1, None, 3, 5)
    assert want['short'] == len(want['labels']) == 10 and got['short'] == want['short']
    assert np.array_equal(got['candidates'], want['candidates']) and (got['candidates'][:, 3] == -1).all()
    # 1100 items: X_g is the last 1024 of the view, the window (0, 40) lies in front of it
    items, offsets, V = ref.case_data()
    seq = items[offsets[7]:offsets[8]]
    want = ref.one_row(seq, offsets[7], ref.TRAIN, V, 0, 40, 1, 40, 40, 20, 9)
    got = ops.next_item_row_host(seq, offsets[7], 40, ops.NEXT_TRAIN, V, 0, 40, 1, 40, 20, 9)
    assert want['X'] == set(seq[75:1099].tolist()) and np.array_equal(got['candidates'], want['candidates'])
    assert set(seq[:75].tolist()) - want['X']                     # some early item is not excluded ...
    assert np.array_equal(got['labels'], seq[1:40])


@pytest.mark.parametrize('drop', [1, 2])
def test_host_row_eval(drop):
    from bert4clickpath_amd import ops
    items, offsets, V = ref.case_data()
    n_t = []
    for g in range(len(offsets) - 1):
        seq = items[offsets[g]:offsets[g + 1]]
        want = ref.one_row(seq, offsets[g], ref.EVAL, V, holdout=drop, max_len=5, W=7, N=2, seed=3)
        got = ops.next_item_row_host(seq, offsets[g], 7, ops.NEXT_EVAL, V, holdout=drop, max_len=5, num_negatives=2, seed=3)
        for k in ('inputs', 'labels', 'pos', 'candidates'):
            assert np.array_equal(got[k], want[k]), (g, k)
        t = len(seq) - drop
        assert len(got['labels']) == (1 if t >= 1 else 0) and got['n_in'] == max(min(t, 5), 0)
        if t >= 1:
            assert got['labels'][0] == seq[t] and got['pos'][0] == got['n_in'] - 1
            assert np.array_equal(got['inputs'][:got['n_in']], seq[t - got['n_in']:t].astype(np.int64) + 10)
        n_t.append(t)
    assert {0, 1} <= set(n_t) and 10 in n_t                       # t = 0, 1 and max_len + 5


# ---- DeviceCloze, host side --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('holdout', [1, 2])
def test_device_cloze_host_side(holdout):
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    items, offsets, V = ref.case_data()
    dc = DeviceCloze(items, offsets, V=V, device=None, max_len=5, holdout=holdout)
    win = np.arange(dc.n_windows)
    want = ref.batch(items, offsets, ref.TRAIN, win, V, dc.windows, holdout, 5)
    assert dc.next_item_sizes(win) == (want['n_targets'], want['n_real_tokens'])
    assert np.array_equal(np.concatenate([[0], np.cumsum(dc.next_item_counts(win))]), want['row_off'])
    # stride == max_len: every item of every training view but its first is a target, exactly once where the windows abut (T a
    # multiple of max_len, or one window).  window_table anchors the windows at the view's END, so otherwise the window at 0
    # overlaps the one behind it, at a1 = T mod max_len, and the max_len - a1 targets they share come twice: counted exactly.
    hits = np.zeros(len(items), np.int64)
    np.add.at(hits, np.asarray(want['csr'], np.int64), 1)
    expect = np.zeros(len(items), np.int64)
    abutting = 0
    for g in range(dc.n_seq):
        T = max(int(dc.lengths[g]) - holdout, 0)
        expect[offsets[g] + 1:offsets[g] + T] = 1
        if T > 5 and T % 5:
            expect[offsets[g] + T % 5:offsets[g] + 5] += 1
        abutting += T > 5 and T % 5 == 0
    assert abutting >= 1 and np.array_equal(hits, expect) and hits.sum() == want['n_targets'] > 1000
    with pytest.raises(ValueError, match='rows = %d' % (want['n_targets'] - 1)):
        dc.next_item_window_batch(win, rows=want['n_targets'] - 1)
    with pytest.raises(ValueError, match='host side only'):
        dc.next_item_window_batch(win)
    if holdout == 1:
        with pytest.raises(ValueError, match="'valid' needs holdout=2"):
            next(dc.next_item_eval_batches(4, split='valid'))
