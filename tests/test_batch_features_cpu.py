"""Side features of device-built batches, the parts that need no GPU (NO REFERENCE ORACLE: an extension -- the restatement is
tests/batch_features_ref.py): the entry points' declarations and their binding, the argument checks that refuse a launch, the rule on the host
(b4c_batch_features_row) against the restatement, DeviceCloze's validation of features= and next_item_loss' missing-feature error."""
import numpy as np
import pytest

import abi_pin
import batch_features_ref as ref

A = 1 << 20                                                       # a well-aligned, never dereferenced "pointer"
NAMES = ('b4c_batch_features', 'b4c_batch_features_row')


def test_header_declares_the_entry_points_and_they_are_bound():
    from bert4clickpath_amd import _lib, ops
    c = _lib.ctypes
    lib = _lib.lib()
    declared = _lib.signatures()
    ptr, i32, i64 = c.c_void_p, c.c_int, c.c_int64
    lists = {
        # (items, offsets, win_seq, win_start, win_len, row_win, B, W, layout, holdout, max_len, V, items_in, ld_items, n_feat, src, kind,
        #  on_mask, out, ld_out, stream)
        'b4c_batch_features': [ptr] * 6 + [i32] * 6 + [ptr, i32, i32, ptr, ptr, ptr, ptr, i32, ptr],
        # (seq, n_g, seq_off, a, L, W, layout, holdout, max_len, V, src, kind, on_mask, items_in, out, geom_out)
        'b4c_batch_features_row': [ptr, i32, i64] + [i32] * 7 + [ptr, i32, i32, ptr, ptr, ptr],
    }
    assert set(NAMES) <= set(declared) and sorted(n for n in declared if n.startswith('b4c_batch_features')) == sorted(NAMES)
    for name in NAMES:
        assert declared[name] == (c.c_int, lists[name]), name
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == lists[name] and getattr(lib, name).restype is c.c_int
    assert (ops.FEAT_EVENT, ops.FEAT_ITEM, ops.FEAT_MASKED, ops.FEAT_KEPT) == (0, 1, 0, 1)
    assert (ops.FEAT_CLOZE, ops.FEAT_NEXT_TRAIN, ops.FEAT_NEXT_EVAL) == (0, 1, 2)
    assert ops.FEAT_KINDS == ref.KINDS and ops.FEAT_ON_MASK == ref.ON_MASK
    assert _lib.ABI_VERSION == abi_pin.ABI_VERSION and lib.b4c_abi_version() == abi_pin.ABI_VERSION and _lib.MAX_FEATURES == 4


def _launch(L, items=A, offsets=A, win_seq=A, win_start=A, win_len=A, row_win=A, B=4, W=8, layout=0, holdout=1, max_len=8, V=500, items_in=A,
            ld_items=8, n_feat=2, src=(A, A), kind=(0, 1), on_mask=(0, 1), out=(A, A), ld_out=8, arrays=()):
    import ctypes as c
    ptrs = lambda v: None if v is None else (c.c_void_p * len(v))(*v)
    ints = lambda v: None if v is None else (c.c_int * len(v))(*v)
    src, out = (None if 'src' in arrays else src), (None if 'out' in arrays else out)
    kind, on_mask = (None if 'kind' in arrays else kind), (None if 'on_mask' in arrays else on_mask)
    return L.b4c_batch_features(items, offsets, win_seq, win_start, win_len, row_win, B, W, layout, holdout, max_len, V, items_in, ld_items,
                                n_feat, ptrs(src), ints(kind), ints(on_mask), ptrs(out), ld_out, None)


FOUR = dict(src=(A,) * 5, kind=(0,) * 5, on_mask=(0,) * 5, out=(A,) * 5)
BAD = [dict(items=None), dict(offsets=None), dict(items_in=None), dict(arrays=('src',)), dict(arrays=('kind',)), dict(arrays=('on_mask',)),
       dict(arrays=('out',)), dict(src=(A, None)), dict(out=(None, A)),
       dict(n_feat=0), dict(n_feat=5, **FOUR), dict(n_feat=-1),
       dict(W=0), dict(W=1022, ld_items=1022, ld_out=1022), dict(ld_items=7), dict(ld_out=7),
       dict(layout=3), dict(layout=-1), dict(kind=(0, 2)), dict(kind=(-1, 0)), dict(on_mask=(2, 0)), dict(on_mask=(0, -1)),
       dict(win_seq=None), dict(win_start=None), dict(win_len=None), dict(layout=1, win_seq=None), dict(layout=1, win_len=None),
       dict(layout=1, holdout=0), dict(layout=2, holdout=0), dict(layout=2, max_len=0), dict(B=-1), dict(V=0)]


def test_bad_arguments_are_refused_without_a_launch():
    """(every call here would fault on its made-up pointers if it were launched, and there is no device to launch on)"""
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    for kw in BAD:
        assert _launch(L, **kw) == _lib._C['B4C_EINVAL'], kw
        assert b'batch_features' in L.b4c_last_error(), (kw, L.b4c_last_error())
    # nothing to do is not an error (and launches nothing)
    assert _launch(L, B=0) == 0
    assert _launch(L, B=0, items=None, items_in=None, arrays=('src', 'out', 'kind', 'on_mask')) == 0
    # the Cloze layout reads neither holdout nor max_len, NEXT_EVAL no table: not refused for them (B = 0: nothing is launched)
    assert _launch(L, B=0, holdout=0, max_len=0) == 0 and _launch(L, B=0, layout=2, win_seq=None, win_start=None, win_len=None) == 0


def test_host_wrappers_validate_before_the_device_is_needed():
    import torch
    from bert4clickpath_amd import ops
    it, off = torch.zeros(5, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    w = torch.zeros(1, dtype=torch.int32)
    rows = torch.zeros(1, 4, dtype=torch.int64)
    ev, tab = torch.zeros(5, dtype=torch.int32), torch.zeros(9, dtype=torch.int32)
    ok = [(ev, 'event', 'keep'), (tab, 'item', 'mask')]
    with pytest.raises(ops.B4CError, match='int32'):
        ops.batch_features(it.long(), off, w, w, w, w, 4, 0, rows, ok)
    with pytest.raises(ops.B4CError, match='1 .. 4'):
        ops.batch_features(it, off, w, w, w, w, 4, 0, rows, ok * 3)
    with pytest.raises(ops.B4CError, match='1 .. 4'):
        ops.batch_features(it, off, w, w, w, w, 4, 0, rows, [])
    with pytest.raises(ops.B4CError, match="'event' or 'item'"):
        ops.batch_features(it, off, w, w, w, w, 4, 0, rows, [(ev, 'token', 'keep')])
    with pytest.raises(ops.B4CError, match="'mask' or 'keep'"):
        ops.batch_features(it, off, w, w, w, w, 4, 0, rows, [(ev, 'event', 'drop')])
    with pytest.raises(ops.B4CError, match='9 values for 5 tokens'):
        ops.batch_features(it, off, w, w, w, w, 4, 0, rows, [(tab, 'event', 'keep')])
    with pytest.raises(ops.B4CError, match='another has 9'):
        ops.batch_features(it, off, w, w, w, w, 4, 0, rows, [(tab, 'item', 'keep'), (ev, 'item', 'keep')])
    with pytest.raises(ops.B4CError, match='layout 3'):
        ops.batch_features(it, off, w, w, w, w, 4, 3, rows, ok)
    with pytest.raises(ops.B4CError, match='items_in'):
        ops.batch_features(it, off, w, w, w, w, 5, 0, rows, ok)
    with pytest.raises(ops.B4CError, match=r'row_win must be an int32 \[B\] = \[1\]'):
        ops.batch_features(it, off, w, w, w, torch.zeros(2, dtype=torch.int32), 4, 0, rows, ok)
    with pytest.raises(ops.B4CError, match='holdout'):
        ops.batch_features(it, off, w, w, w, w, 4, 1, rows, ok, holdout=0)
    with pytest.raises(ops.B4CError, match='HIP device only'):
        ops.batch_features(it, off, w, w, w, w, 4, 0, rows, ok)


# ---- the rule on the host ---------------------------------------------------------------------------------------------------------
MAX_LEN, W = 5, 7
POLICIES = [(per, on_mask) for per in ('event', 'item') for on_mask in ('mask', 'keep')]


def _windows(lengths, holdout):
    from bert4clickpath_amd.cloze_batches import window_table
    return window_table(lengths, MAX_LEN, MAX_LEN, holdout)


def _check_row(ops, data, g, a, L, layout, holdout, items_in):
    """b4c_batch_features_row of the row against the restatement, for both kinds and both mask policies -> n"""
    items, offsets, V, event, table = data
    seq = items[offsets[g]:offsets[g + 1]]
    first, n = ref.geometry(layout, len(seq), a, L, holdout, MAX_LEN, W)
    for per, on_mask in POLICIES:
        src = event if per == 'event' else table
        want = ref.one_row(items, offsets, g, first, n, W, src, ref.KINDS[per], ref.ON_MASK[on_mask], items_in)
        got, gf, gn = ops.batch_features_row_host(seq, offsets[g], W, layout, src, per, on_mask, items_in, a=a, L=L, holdout=holdout,
                                                  max_len=MAX_LEN)
        assert (gf, gn) == (first if n else gf, n) and np.array_equal(got, want), (g, a, L, layout, per, on_mask)
        if n and on_mask == 'keep':
            assert (got[:n] >= 10).all()
        if n and on_mask == 'mask':
            assert np.array_equal(got[:n] == 1, np.asarray(items_in[:n]) == 1)
    return n


@pytest.mark.parametrize('holdout', [1, 2])
def test_host_row_equals_the_restatement_cloze(holdout):
    """Cloze TRAIN rows (the masked positions from b4c_cloze_choose_window, the item builder's own host rule) and EVAL rows (the
    last position masked) of every window of the case list"""
    from bert4clickpath_amd import ops
    data = ref.case_data()
    items, offsets = data[:2]
    lengths = np.diff(offsets)
    n_masked = n_rows = 0
    for g, a, L in zip(*_windows(lengths, holdout)):
        if g == 7 and a not in (0, 5, 50, 1090, 1094, 1095):     # the long sequence: a few windows are enough
            continue
        row = np.zeros(W, np.int64)
        row[:L] = items[offsets[g] + a:offsets[g] + a + L].astype(np.int64) + 10
        pos = ops.cloze_choose_window_host(77, g, a, L, masked_percentage=0.4, max_masked=3)
        row[pos] = 1
        n_masked += len(pos)
        n_rows += _check_row(ops, data, int(g), int(a), int(L), ref.CLOZE, holdout, row) > 0
    assert n_masked > 10 and n_rows > 10
    for drop in range(1, holdout + 1):                             # EVAL: the window ends at the target, which is masked
        for g in range(len(lengths)):
            end = max(int(lengths[g]) - drop + 1, 0)
            start = max(end - MAX_LEN, 0)
            row = np.zeros(W, np.int64)
            row[:end - start] = items[offsets[g] + start:offsets[g] + end].astype(np.int64) + 10
            if end > start:
                row[end - start - 1] = 1
            assert _check_row(ops, data, g, start, end - start, ref.CLOZE, holdout, row) == end - start


@pytest.mark.parametrize('holdout', [1, 2])
def test_host_row_equals_the_restatement_next_item(holdout):
    """next-item TRAIN rows of every window (a = 0 and the prepended input of a > 0) and EVAL rows of every sequence, the item rows
    from b4c_next_item_row; holdout is the EVAL rows' drop"""
    from bert4clickpath_amd import ops
    data = ref.case_data()
    items, offsets, V = data[:3]
    seen = set()
    for g, a, L in zip(*_windows(np.diff(offsets), holdout)):
        if g == 7 and a not in (0, 5, 50, 1090, 1094, 1095):
            continue
        seq = items[offsets[g]:offsets[g + 1]]
        row = ops.next_item_row_host(seq, offsets[g], W, ops.NEXT_TRAIN, V, a, L, holdout, MAX_LEN)
        n = _check_row(ops, data, int(g), int(a), int(L), ref.NEXT_TRAIN, holdout, row['inputs'])
        assert n == row['n_in']
        seen.add((int(a > 0), min(n, 2)))
    assert {(0, 0), (0, 1), (0, 2), (1, 2)} <= seen
    ns = set()
    for g in range(len(offsets) - 1):
        seq = items[offsets[g]:offsets[g + 1]]
        row = ops.next_item_row_host(seq, offsets[g], W, ops.NEXT_EVAL, V, holdout=holdout, max_len=MAX_LEN)
        n = _check_row(ops, data, g, 0, 0, ref.NEXT_EVAL, holdout, row['inputs'])
        assert n == row['n_in']
        ns.add(n)
    assert {0, 1, MAX_LEN} <= ns


def test_host_row_refusals():
    from bert4clickpath_amd import ops
    items, offsets, V, event, table = ref.case_data()
    seq = items[offsets[3]:offsets[4]]
    row = np.zeros(W, np.int64)
    with pytest.raises(ops.B4CError, match='leaves its sequence'):
        ops.batch_features_row_host(seq, offsets[3], W, ops.FEAT_CLOZE, event, 'event', 'mask', row, a=1, L=5)
    with pytest.raises(ops.B4CError, match=r'outside \[0, V = 4\)'):
        ops.batch_features_row_host(seq, offsets[3], W, ops.FEAT_CLOZE, table[:4], 'item', 'mask', row, a=0, L=3)
    with pytest.raises(ops.B4CError, match='W = 0'):
        ops.batch_features_row_host(seq, offsets[3], 0, ops.FEAT_CLOZE, event, 'event', 'mask', row)


# ---- DeviceCloze, host side --------------------------------------------------------------------------------------------------------
def test_device_cloze_validates_its_features():
    from bert4clickpath_amd.cloze_batches import DeviceCloze, Feature
    items, offsets, V, event, table = ref.case_data()
    good = {'action': Feature(event, ref.EVENT_SIZE, per='event', on_mask='keep'), 'category': Feature(table, ref.ITEM_SIZE, per='item')}
    dc = DeviceCloze(items, offsets, V=V, device=None, features=good)
    assert list(dc.features) == ['action', 'category'] and dc.features['action'][0].dtype == np.int32
    assert np.array_equal(dc.features['category'][0], table) and dc.features['category'][1].on_mask == 'mask'
    assert DeviceCloze(items, offsets, V=V, device=None).features == {}
    with pytest.raises(ValueError, match='host side only'):
        dc.batch([1, 2], 'train')
    bad = [({'a': Feature(event, 7), 'b': Feature(event, 7), 'c': Feature(event, 7), 'd': Feature(event, 7)}, 'at most 3'),
           ({'action': Feature(event[:-1], 7)}, "'action' is per 'event'"),
           ({'category': Feature(table[:-1], 23, per='item')}, "'category' is per 'item'"),
           ({'category': Feature(event, 23, per='item')}, "'category' is per 'item'"),
           ({'action': Feature(event, 6)}, r"'action': values outside \[0, size = 6\)"),
           ({'action': Feature(event.astype(np.int64) - 1, 7)}, r"'action': values outside"),
           ({'action': Feature(event.astype(np.float32), 7)}, "'action': values of dtype float32"),
           ({'action': Feature(event, 0)}, "'action': values outside"),
           ({'action': event}, 'Feature objects')]
    for features, match in bad:
        with pytest.raises(ValueError, match=match):
            DeviceCloze(items, offsets, V=V, device=None, features=features)
    with pytest.raises(ValueError, match="per = 'user'"):
        Feature(event, 7, per='user')
    with pytest.raises(ValueError, match="on_mask = 'drop'"):
        Feature(event, 7, on_mask='drop')
    b = {'items': 'I', 'features': {'action': 'A', 'category': 'C'}}
    assert DeviceCloze.inputs(b, 'asin') == {'asin': 'I', 'action': 'A', 'category': 'C'} and DeviceCloze.inputs({'items': 'I'}, 'x') == {'x': 'I'}


def _cpu_model(config):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, ClozeMaskedItemPrediction
    vocabs = {'items': ['i%d' % i for i in range(20)], 'cats': ['c%d' % i for i in range(5)]}
    return ClickstreamTransformer(config, vocabs, {'items': 8, 'cats': 8}, ClozeMaskedItemPrediction([], 20), value_to_head='[MASK]',
                                  num_encoder_layers=1, num_attention_heads=1, dropout_rate=0.0, attention='causal')


def test_next_item_loss_names_the_feature_the_batch_lacks():
    """raised before any device work: a CPU model and a batch of placeholders are enough"""
    from bert4clickpath_amd import B4CError
    model = _cpu_model({'items': ['asin'], 'cats': ['category']})
    with pytest.raises(B4CError, match="the feature 'category', which the batch does not carry \\(it has none\\)"):
        model.next_item_loss({'items': None})
    with pytest.raises(B4CError, match=r"'category'.*it has \['action'\]"):
        model.next_item_loss({'items': None, 'features': {'action': None}})
    assert model._next_item_inputs({'items': 'I', 'features': {'category': 'C', 'action': 'A'}}) == {'asin': 'I', 'category': 'C'}
    chained = _cpu_model({'items': ['asin', 'asin2'], 'cats': ['category']})
    with pytest.raises(B4CError, match='exactly one input'):
        chained.next_item_loss({'items': None, 'features': {'category': None}})
