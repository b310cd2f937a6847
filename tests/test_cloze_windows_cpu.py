"""Host side of the paper's data protocol in DeviceCloze (no GPU): the vectorised window table against the loop of
tests/cloze_window_ref.py (count formula, coverage, no window reaches a held-out item), the windowed masking rule on the host
(b4c_cloze_choose_window) against b4c_cloze_choose and the restatement, the last-only draw and its rate, the data-parallel
slices over windows, the defaults, the argument errors, and the new symbols at the pinned ABI version."""
import numpy as np
import pytest
import torch

import abi_pin
import cloze_window_ref as ref

WS = (1, 4, 7, 50)
STRIDES = (1, 3, 'W')
HOLDOUTS = (1, 2)


def _lengths(W, stride, holdout):
    return [n + holdout for n in (0, 1, 2, 3, W - 1, W, W + 1, W + 2, W + stride, 2 * W, 2 * W + 1, 3 * W + 5)]


def _host_data(lengths, V=50, seed=2, **kw):
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    items, offsets = ref.synthetic_csr(lengths, V, seed=seed)
    return DeviceCloze(items, offsets, V=V, device=None, **kw)


def test_the_new_symbols_are_declared_and_exported_at_abi_12():
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    sig = _lib.signatures()
    for name, n_args in (('b4c_cloze_batch_windows', 20), ('b4c_cloze_choose_window', 9), ('b4c_cloze_history', 9)):
        assert name in sig and name in _lib.declared_symbols() and hasattr(L, name)
        assert len(sig[name][1]) == n_args
    assert len(sig['b4c_cloze_batch'][1]) == 16 and len(sig['b4c_cloze_choose'][1]) == 5      # the old lists are as they were
    assert _lib.ABI_VERSION == abi_pin.ABI_VERSION and L.b4c_abi_version() == abi_pin.ABI_VERSION


@pytest.mark.parametrize('holdout', HOLDOUTS)
@pytest.mark.parametrize('stride', STRIDES)
@pytest.mark.parametrize('W', WS)
def test_window_table_equals_the_loop_and_covers_the_training_view_without_a_leak(W, stride, holdout):
    stride = W if stride == 'W' else stride
    if stride > W:                                                 # (W = 1, stride = 3): not a stride DeviceCloze takes
        with pytest.raises(ValueError, match='stride'):
            _host_data([5, 6], max_len=W, stride=stride, holdout=holdout)
        return
    lengths = _lengths(W, stride, holdout)
    d = _host_data(lengths, max_len=W, stride=stride, holdout=holdout)
    seq, start, length = ref.window_table(lengths, W, stride, holdout)
    assert d.n_windows == len(seq)
    for got, want in zip(d.windows, (seq, start, length)):
        assert got.dtype == np.int32 and np.array_equal(got, want)
    for g, n in enumerate(lengths):
        T = max(n - holdout, 0)
        mine = np.flatnonzero(d.windows.seq == g)
        a, L = d.windows.start[mine].astype(int), d.windows.len[mine].astype(int)
        want_count = (1 if T > 0 else 0) if T <= W else 1 + -(-(T - W) // stride)
        assert len(mine) == want_count, (g, n)
        if T == 0:
            continue
        assert (a >= 0).all() and (L >= 1).all() and (L <= W).all()
        assert (a + L <= T).all()                                  # the leak check: no window index reaches T or beyond
        assert a[0] + L[0] == T                                    # the most recent window ends at T
        covered = np.zeros(T, bool)
        for s, l in zip(a, L):
            covered[s:s + l] = True
        assert covered.all(), (g, n)
        assert (L == min(T, W)).all() and len(set(a.tolist())) == len(a)


def test_stride_none_is_max_len_and_max_len_none_is_one_whole_window_each():
    lengths = [0, 1, 2, 9, 17, 40]
    a, b = _host_data(lengths, max_len=8), _host_data(lengths, max_len=8, stride=8)
    assert all(np.array_equal(x, y) for x, y in zip(a.windows, b.windows))
    d = _host_data(lengths)
    assert d.n_windows == d.n_seq == 6 and d.max_len is None and d.holdout == 1 and d.last_thr == 0
    assert np.array_equal(d.windows.seq, np.arange(6)) and not d.windows.start.any()
    assert np.array_equal(d.windows.len, [0, 0, 1, 8, 16, 39])
    d2 = _host_data(lengths, holdout=2)
    assert np.array_equal(d2.windows.len, [0, 0, 0, 7, 15, 38]) and d2.n_windows == 6
    assert np.array_equal(d.epoch_order(9, 1), np.random.default_rng([9, 1]).permutation(6))


@pytest.mark.parametrize('L', (0, 1, 2, 3, 5, 64, 65, 257, 1021))
def test_choose_window_at_start_0_without_last_rows_equals_choose(L):
    from bert4clickpath_amd import ops
    for seed in (0, 1234, 2 ** 63 + 12345):
        for g in (0, 7, 2 ** 31 + 5, 2 ** 54 - 1):
            for pct, mm in ((0.4, 10), (1.0, 64), (0.2, 3), (0.4, 0)):
                got = ops.cloze_choose_window_host(seed, g, 0, L, pct, mm, 0)
                n = ref.n_masked(L, pct, mm)
                assert got.dtype == np.int32 and np.array_equal(got, ops.cloze_choose_host(seed, g, L, n)), (L, seed, g, pct, mm)
                assert np.array_equal(got, ref.choose_window(seed, g, 0, L, pct, mm, 0))


def test_choose_window_equals_the_restatement_at_other_starts_and_thresholds():
    from bert4clickpath_amd import ops
    for L in (1, 4, 20, 200, 1021):
        for a in (1, 3, 50, 2 ** 31 - 1):
            for g in (0, 11, 2 ** 54 - 1):
                for thr in (0, 1 << 22, 1 << 23, 1 << 24):
                    got = ops.cloze_choose_window_host(77, g, a, L, 0.4, 10, thr)
                    assert np.array_equal(got, ref.choose_window(77, g, a, L, 0.4, 10, thr)), (L, a, g, thr)


def test_two_windows_of_one_sequence_use_different_seeds():
    from bert4clickpath_amd import ops
    assert ref.window_seed(5, 0) == 5 and ref.window_seed(5, 1) != ref.window_seed(5, 2) != 5
    base = ops.cloze_choose_window_host(5, 3, 0, 200, 0.4, 10, 0)
    seen = {tuple(base.tolist())}
    for a in (1, 2, 20, 180):
        pos = ops.cloze_choose_window_host(5, 3, a, 200, 0.4, 10, 0)
        assert np.array_equal(pos, ops.cloze_choose_window_host(5, 3, a, 200, 0.4, 10, 0))
        assert np.array_equal(pos, ops.cloze_choose_host(ref.window_seed(5, a), 3, 200, 10))      # the window seed keys the draw
        seen.add(tuple(pos.tolist()))
    assert len(seen) == 5


def _windows_20000():
    d = _host_data(np.tile([3, 9, 21, 30, 47, 64, 100, 12], 500), max_len=20, stride=5)
    assert d.n_windows >= 20000
    return d.windows.seq[:20000], d.windows.start[:20000], d.windows.len[:20000]


def test_last_only_rows_all_none_and_a_quarter():
    """masked_percentage = 0 leaves an ordinary row without a masked position, so the rows with one are the last-only rows.
    Rate 0.25 over 20,000 windows: the share is within 0.02 (6.5 binomial standard deviations of 0.0031); the draw is a fixed
    function of the seed, and at seed 2024 the share is 0.2456."""
    from bert4clickpath_amd import ops
    seq, start, length = _windows_20000()
    assert ops.cloze_last_thr(1.0) == 1 << 24 and ops.cloze_last_thr(0.0) == 0 and ops.cloze_last_thr(0.25) == 1 << 22
    some_empty = [(0, 0, 0), (5, 3, 0)]
    for g, a, L in list(zip(seq[:300], start[:300], length[:300])) + some_empty:
        every = ops.cloze_choose_window_host(2024, g, a, L, 0.4, 10, 1 << 24)
        assert np.array_equal(every, [L - 1] if L > 0 else [])
        none = ops.cloze_choose_window_host(2024, g, a, L, 0.0, 10, 0)
        assert len(none) == 0
        assert not ref.last_only(2024, int(g), int(a), int(L), 0) and ref.last_only(2024, int(g), int(a), int(L), 1 << 24) == (L > 0)
    thr = ops.cloze_last_thr(0.25)
    picked = np.array([len(ops.cloze_choose_window_host(2024, g, a, L, 0.0, 10, thr)) for g, a, L in zip(seq, start, length)])
    assert set(picked.tolist()) == {0, 1}
    share = picked.mean()
    print('last-only share at rate 0.25 over 20000 windows: %.4f' % share)
    assert abs(share - 0.25) < 0.02, share
    for i in range(0, 20000, 97):                                  # the restatement's draw, window by window
        assert ref.last_only(2024, int(seq[i]), int(start[i]), int(length[i]), thr) == bool(picked[i])


@pytest.mark.parametrize('world', (2, 3))
def test_rank_slices_over_windows_unite_to_the_world_1_slices(world):
    d = _host_data([0, 1, 2, 5, 9, 3, 7, 26, 27, 4, 6, 11, 2, 8, 5, 30, 1, 12, 3, 4, 10, 6, 7], max_len=4, stride=3, holdout=2)
    assert d.n_windows > d.n_seq
    for epoch in (0, 1):
        order = d.epoch_order(9, epoch)
        assert np.array_equal(order, np.random.default_rng([9, epoch]).permutation(d.n_windows))
        o1, one = d.rank_slices(4 * world, 9, epoch)
        parts = [d.rank_slices(4, 9, epoch, rank=r, world=world) for r in range(world)]
        assert one == [(s, s + 4 * world) for s in range(0, d.n_windows - 4 * world + 1, 4 * world)] and len(one) >= 2
        for i, (lo, hi) in enumerate(one):
            assert all(np.array_equal(o, order) for o, _ in parts)
            assert np.array_equal(order[lo:hi], np.concatenate([order[s[i][0]:s[i][1]] for _, s in parts]))
        assert all(len(s) == len(one) for _, s in parts)
    assert d.rank_slices(d.n_windows + 1, 9, 0)[1] == []


def test_defaults_are_one_window_per_sequence_and_bad_arguments_raise():
    lengths = [0, 1, 2, 5, 9, 30]
    d = _host_data(lengths)
    assert d.n_windows == d.n_seq
    for kw, word in ((dict(max_len=4, stride=0), 'stride'), (dict(max_len=4, stride=5), 'stride'), (dict(stride=2), 'stride'),
                     (dict(holdout=3), 'holdout'), (dict(holdout=0), 'holdout'), (dict(last_item_rate=-0.1), 'last_item_rate'),
                     (dict(last_item_rate=1.5), 'last_item_rate'), (dict(max_len=0), 'max_len'), (dict(max_len=1022), 'max_len')):
        with pytest.raises(ValueError, match=word):
            _host_data(lengths, **kw)
    with pytest.raises(ValueError, match='valid'):
        d.row_lengths([1, 2], 'eval', split='valid')
    with pytest.raises(ValueError, match='valid'):
        next(d.eval_batches(4, split='valid'))
    with pytest.raises(ValueError, match='split'):
        d.n_real_tokens([1], 'eval', split='dev')
    two = _host_data(lengths, holdout=2, max_len=4)
    assert np.array_equal(two.row_lengths(np.arange(6), 'eval', split='valid'), [0, 0, 1, 4, 4, 4])
    assert np.array_equal(two.row_lengths(np.arange(6), 'eval', split='test'), [0, 1, 2, 4, 4, 4])
    assert np.array_equal(two.row_lengths(np.arange(6), 'train'), [0, 0, 0, 3, 4, 4])
    with pytest.raises(ValueError, match='training windows'):
        two.batch([3, 4], 'train')                                 # sequence 4: T = 7 > 4, two windows
    with pytest.raises(ValueError, match='outside'):
        two.window_batch([two.n_windows])
    with pytest.raises(ValueError, match='device=None'):
        two.window_batch([0])


def test_item_counts_leave_out_the_held_out_items():
    lengths = [0, 1, 2, 5, 9, 30]
    for holdout in (1, 2):
        d = _host_data(lengths, holdout=holdout, max_len=4)
        want = np.zeros(50, np.int64)
        for g in range(d.n_seq):
            np.add.at(want, d.items[d.offsets[g]:d.offsets[g + 1]][:max(lengths[g] - holdout, 0)], 1)
        got = d.item_counts()
        assert got.dtype == np.int64 and got.shape == (50,) and np.array_equal(got, want)
    with pytest.raises(ValueError, match='train'):
        d.item_counts(split='test')


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    EINVAL = -1

    def windows(B=4, W=8, mode=0, pct=0.4, mm=10, thr=0, ld_items=None, ld_lab=None, M=10):
        return L.b4c_cloze_batch_windows(None, None, None, None, None, None, B, W, mode, pct, mm, 0, thr, None,
                                         W if ld_items is None else ld_items, None, M if ld_lab is None else ld_lab, M, None, None)

    for kw, word in ((dict(W=0), b'W = 0'), (dict(W=1022), b'W = 1022'), (dict(M=9), b'max_masked'), (dict(M=65, mm=65), b'M = 65'),
                     (dict(mode=2), b'mode 2'), (dict(mode=1, M=0), b'M = 0'), (dict(ld_items=7), b'ld_items'), (dict(ld_lab=9), b'ld_lab'),
                     (dict(pct=1.5), b'masked_percentage'), (dict(B=-1), b'B = -1'), (dict(thr=(1 << 24) + 1), b'last_thr'),
                     (dict(thr=5, M=0, mm=0), b'last_thr'), (dict(), b'null pointer')):
        assert windows(**kw) == EINVAL, kw
        assert word in L.b4c_last_error() and b'cloze_batch_windows' in L.b4c_last_error(), (kw, L.b4c_last_error())
    assert windows(B=0) == 0
    pos, n = np.zeros(64, np.int32), np.zeros(1, np.int32)
    for args in ((0, 0, 0, 1022, 0.4, 10, 0), (0, -1, 0, 3, 0.4, 10, 0), (0, 2 ** 54, 0, 3, 0.4, 10, 0), (0, 0, -1, 3, 0.4, 10, 0),
                 (0, 0, 0, 3, 1.5, 10, 0), (0, 0, 0, 3, 0.4, 65, 0), (0, 0, 0, 3, 0.4, 10, (1 << 24) + 1)):
        assert L.b4c_cloze_choose_window(*args, pos.ctypes.data, n.ctypes.data) == EINVAL, args
        assert b'cloze_choose_window' in L.b4c_last_error()
    assert L.b4c_cloze_choose_window(0, 0, 0, 3, 0.4, 10, 0, None, n.ctypes.data) == EINVAL
    for kw in (dict(drop=0), dict(E=0), dict(E=1025), dict(ld=3), dict(B=-1), dict()):
        a = dict(B=2, drop=1, E=4, ld=4)
        a.update(kw)
        assert L.b4c_cloze_history(None, None, None, a['B'], a['drop'], a['E'], None, a['ld'], None) == EINVAL, kw
        assert b'cloze_history' in L.b4c_last_error()
    assert L.b4c_cloze_history(None, None, None, 0, 1, 4, None, 4, None) == 0


def test_the_bindings_check_their_arguments_before_device_work():
    from bert4clickpath_amd import ops
    from bert4clickpath_amd._lib import B4CError
    items, offsets = torch.zeros(6, dtype=torch.int32), torch.tensor([0, 2, 6])
    ws, wa, wl, rows = (torch.zeros(2, dtype=torch.int32) for _ in range(4))

    def call(items=items, offsets=offsets, ws=ws, wa=wa, wl=wl, rows=rows, W=4, mode=ops.CLOZE_TRAIN, seed=0, **kw):
        return ops.cloze_batch_windows(items, offsets, ws, wa, wl, rows, W, mode, seed, **kw)

    for kw, word in ((dict(items=items.long()), 'items'), (dict(offsets=offsets.int()), 'offsets'), (dict(ws=ws.long()), 'win_seq'),
                     (dict(wa=wa[:1]), 'win_start'), (dict(wl=wl.float()), 'win_len'), (dict(rows=rows.long()), 'row_win'),
                     (dict(W=0), 'W = 0'), (dict(W=1022), 'W = 1022'), (dict(mode=2), 'mode 2'), (dict(M=9), 'M = 9'),
                     (dict(M=65), 'M = 65'), (dict(last_thr=-1), 'last_thr = -1'), (dict(last_thr=(1 << 24) + 1), 'last_thr'),
                     (dict(last_thr=3, max_masked=0), 'last_thr = 3'), (dict(masked_percentage=2.0), 'masked_percentage'),
                     (dict(seed=-1), 'seed'), (dict(), 'CPU tensor'), (dict(rows=None), 'CPU tensor')):
        with pytest.raises(B4CError, match=word):
            call(**kw)
    seq = torch.zeros(3, dtype=torch.int32)
    for args, word in (((items.long(), offsets, seq, 4), 'items'), ((items, offsets.int(), seq, 4), 'offsets'),
                       ((items, offsets, seq.long(), 4), 'seq_idx'), ((items, offsets, seq, 0), 'E = 0'),
                       ((items, offsets, seq, 1025), 'E = 1025'), ((items, offsets, seq, 4, 0), 'drop = 0'),
                       ((items, offsets, seq, 4), 'CPU tensor')):
        with pytest.raises(B4CError, match=word):
            ops.cloze_history(*args)
    with pytest.raises(B4CError, match='last_thr'):
        ops.cloze_choose_window_host(0, 0, 0, 3, 0.4, 10, (1 << 24) + 1)
    with pytest.raises(B4CError, match='L = 1022'):
        ops.cloze_choose_window_host(0, 0, 0, 1022)
    with pytest.raises(B4CError, match='rate'):
        ops.cloze_last_thr(1.01)
