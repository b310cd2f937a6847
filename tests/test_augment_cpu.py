"""The contrastive-views section of include/b4c.h, its binding and the host rule of the views, without a GPU: the header parses
to the declared table, include/ holds the one header, a duplicate name is refused, the library exports the names;
every argument b4c_augment_views refuses is refused with NULL pointers; b4c_augment_row equals the restatement tests/augment_ref.py
(written from the header's text) on every window of the case data; the structural properties of the ops hold on the restatement;
DeviceCloze's host token count equals the restatement's.  Everything is integer-exact: no tolerance."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import abi_pin
import augment_ref as ar
import next_item_ref as nref

V_, I, I64, F, U32, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint32, ctypes.c_uint64
VIEWS = [V_] * 6 + [I] * 6 + [U32, F, F, F, U64, V_, V_, V_, I, V_, I, V_, I, V_, V_, V_, V_, V_]
ROW = [V_, V_, I64, I64] + [I] * 7 + [U32, F, F, F, U64, V_, V_, V_, I, V_, V_, V_]


@pytest.fixture(scope='module')
def L():
    from bert4clickpath_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def ops():
    from bert4clickpath_amd import ops as o
    return o


@pytest.fixture(scope='module')
def data():
    items, offsets, V = nref.case_data()
    per = {h: (ar.case_table(offsets, h), ar.target_index(items, offsets, h, V)) for h in (1, 2)}
    return items, offsets, V, per


# ---- header and binding -----------------------------------------------------------------------------------------------------------
NAMES = {'b4c_augment_views', 'b4c_augment_row'}


def test_header_parses_to_the_declared_table(L):
    sig = L.signatures()
    assert sig['b4c_augment_views'] == (I, VIEWS) and sig['b4c_augment_row'] == (I, ROW)
    const = L.header_constants(L._header_text(L.HEADER_PATH))
    assert {k: v for k, v in const.items() if k.startswith('B4C_AUG_')} == {
        'B4C_AUG_CROP': 1, 'B4C_AUG_MASK': 2, 'B4C_AUG_REORDER': 4, 'B4C_AUG_SAME_TARGET': 8, 'B4C_AUG_MAX_VIEWS': 4}
    assert (L.AUG_CROP, L.AUG_MASK, L.AUG_REORDER, L.AUG_SAME_TARGET, L.AUG_MAX_VIEWS) == (1, 2, 4, 8, 4)


def test_one_header_declares_the_family(L):
    sig = L.signatures()
    assert len(sig) == abi_pin.ENTRY_POINTS and L.ABI_VERSION == abi_pin.ABI_VERSION
    assert os.listdir(os.path.dirname(L.HEADER_PATH)) == ['b4c.h']
    assert NAMES <= set(sig)


def test_a_duplicate_name_is_refused(L):
    with pytest.raises(L.B4CError, match=r'declares b4c_augment_views twice'):
        L.parse_header(L._header_text(L.HEADER_PATH) + '\nint b4c_augment_views(const void *z, int ld_z);\n')


def test_the_library_exports_the_names(L):
    nm = shutil.which('nm')
    if nm:
        out = subprocess.run([nm, '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    else:
        lib = ctypes.CDLL(L.LIB_PATH)
        exported = {n for n in NAMES if hasattr(lib, n)}
    assert NAMES <= exported, sorted(NAMES - exported)


def test_a_library_without_a_declared_name_is_refused(L, monkeypatch, tmp_path):
    """lib() raises its usual error for a name the .so lacks: here a header that declares one more name than the library has"""
    more = tmp_path / 'b4c_more.h'
    with open(L.HEADER_PATH) as f:
        more.write_text(f.read() + '\nint b4c_augment_not_there(int n);\n')
    monkeypatch.setattr(L, 'HEADER_PATH', str(more))
    monkeypatch.setattr(L, '_lib', None)
    with pytest.raises(L.B4CError, match=r'does not export b4c_augment_not_there; rebuild it'):
        L.lib()


# ---- argument refusals: before any pointer is looked at ----------------------------------------------------------------------------
GOOD = dict(B=4, W=8, layout=1, holdout=1, max_len=5, n_views=2, ops_mask=7, crop=0.6, mask=0.3, reorder=0.6)
NAN, INF = float('nan'), float('inf')
BAD = [('ops_mask', dict(ops_mask=0)), ('ops_mask', dict(ops_mask=16)), ('ops_mask', dict(ops_mask=0x80000001)),
       ('crop_ratio', dict(crop=0.0)), ('crop_ratio', dict(crop=1.5)), ('crop_ratio', dict(crop=-0.1)), ('crop_ratio', dict(crop=NAN)),
       ('crop_ratio', dict(crop=INF)),
       ('mask_ratio', dict(mask=-0.1)), ('mask_ratio', dict(mask=1.01)), ('mask_ratio', dict(mask=NAN)), ('mask_ratio', dict(mask=INF)),
       ('reorder_ratio', dict(reorder=-0.1)), ('reorder_ratio', dict(reorder=1.01)), ('reorder_ratio', dict(reorder=NAN)),
       ('reorder_ratio', dict(reorder=-INF)),
       ('n_views', dict(n_views=0)), ('n_views', dict(n_views=5)), ('W', dict(W=0)), ('W', dict(W=1022)), ('B', dict(B=-1)),
       ('layout', dict(layout=2)), ('layout', dict(layout=3)), ('holdout', dict(holdout=-1)),
       ('SAME_TARGET', dict(ops_mask=8, layout=0)), ('SAME_TARGET', dict(ops_mask=15, layout=0)),
       ('index', dict(ops_mask=8)), ('index', dict(ops_mask=9))]


def _call(lib, a, ld=None):
    return lib.b4c_augment_views(None, None, None, None, None, None, a['B'], a['W'], a['layout'], a['holdout'], a['max_len'], a['n_views'],
                                 a['ops_mask'], a['crop'], a['mask'], a['reorder'], 5, None, None, None, 0, None, a['W'] if ld is None else ld,
                                 None, a['W'], None, None, None, None, None)


@pytest.mark.parametrize('name,change', BAD, ids=['%s-%s' % (n, '-'.join(str(v) for v in c.values())) for n, c in BAD])
def test_bad_arguments_are_refused_before_any_pointer_is_looked_at(L, name, change):
    lib = L.lib()
    rc = _call(lib, dict(GOOD, **change))
    msg = lib.b4c_last_error().decode()
    assert rc == L._C['B4C_EINVAL'], (rc, msg)
    assert msg.startswith('augment_views:') and name in msg, msg


def test_a_short_pitch_is_refused(L):
    assert _call(L.lib(), GOOD, ld=7) == L._C['B4C_EINVAL'] and 'ld_items' in L.lib().b4c_last_error().decode()


def test_no_rows_is_ok(L):
    assert _call(L.lib(), dict(GOOD, B=0)) == 0
    assert _call(L.lib(), dict(GOOD, B=0, ops_mask=8)) == 0


def test_null_pointers_with_good_scalars_are_refused(L):
    lib = L.lib()
    assert _call(lib, GOOD) == L._C['B4C_EINVAL'] and 'null pointer' in lib.b4c_last_error().decode()


# ---- b4c_augment_row equals the restatement ------------------------------------------------------------------------------------
def _cases(layout):
    return [c for c in ar.CONFIGS if layout == ar.NEXT_TRAIN or 'same_target' not in c[0]]


def _rows_of(data, holdout, layout, config, seed, v, W=8, windows=None):
    items, offsets, V, per = data
    table, index = per[holdout]
    names, kw = config
    for w in (range(len(table[0])) if windows is None else windows):
        g, a, Lw = (-1, 0, 0) if w < 0 else (int(t[w]) for t in table)
        yield w, (g, a, Lw), ar.one_view(items, offsets, g, a, Lw, layout, W, v, ar.ops_mask(names), seed, holdout=holdout, max_len=ar.MAX_LEN,
                                         index=index, V=V, **kw)


@pytest.mark.parametrize('holdout', [1, 2])
@pytest.mark.parametrize('layout', [ar.CLOZE, ar.NEXT_TRAIN], ids=['cloze', 'next'])
@pytest.mark.parametrize('config', ar.CONFIGS, ids=ar.config_id)
def test_host_row_equals_the_restatement(ops, data, holdout, layout, config):
    """every window at max_len = stride = 5 (and the L = 0 window), three seeds, views 0 and 1"""
    if config not in _cases(layout):
        with pytest.raises(ops.B4CError, match='same_target'):
            ops.augment_row_host(data[0], data[1], 4, 8, layout, config[0], 1)
        return
    items, offsets, V, per = data
    names, kw = config
    for seed in ar.SEEDS:
        for v in (0, 1):
            for w, (g, a, Lw), want in _rows_of(data, holdout, layout, config, seed, v):
                got = ops.augment_row_host(items, offsets, g, 8, layout, names, seed, view=v, a=a, L=Lw, holdout=holdout, max_len=ar.MAX_LEN,
                                           target_index=per[holdout][1], V=V, **kw)
                where = (seed, v, w)
                assert np.array_equal(got['items'], want['items']) and np.array_equal(got['src_tok'], want['src_tok']), where
                assert (got['n_items'], got['op'], got['target'], got['self']) == (want['n_out'], want['op'], want['target'], want['self']), where


def test_host_row_of_an_empty_row(ops, data):
    got = ops.augment_row_host(data[0], data[1], -1, 4, ar.NEXT_TRAIN, ('crop', 'mask'), 3)
    assert not got['items'].any() and (got['src_tok'] == -1).all() and (got['n_items'], got['op'], got['target'], got['self']) == (0, 0, -1, 0)


# ---- structural properties, on the restatement ---------------------------------------------------------------------------------
def _source(data, holdout, layout, gaL, W=8):
    items, offsets = data[0].astype(np.int64), data[1]
    g, a, Lw = gaL
    if g < 0:
        return np.zeros(0, np.int64)
    first, n = ar.row_rule(layout, int(offsets[g + 1] - offsets[g]), a, Lw, holdout, W)
    return items[offsets[g] + first:offsets[g] + first + n] + ar.RESERVED


@pytest.mark.parametrize('holdout', [1, 2])
@pytest.mark.parametrize('layout', [ar.CLOZE, ar.NEXT_TRAIN], ids=['cloze', 'next'])
def test_structure_of_crop_mask_reorder(data, holdout, layout):
    seen = {op: 0 for op in (ar.CROP, ar.MASK, ar.REORDER)}
    for config in _cases(layout):
        names, kw = config
        if 'same_target' in names:
            continue
        ratio = {'crop_ratio': 0.6, 'mask_ratio': 0.3, 'reorder_ratio': 0.6, **kw}
        for w, gaL, r in _rows_of(data, holdout, layout, config, ar.SEEDS[0], 1):
            src = _source(data, holdout, layout, gaL)
            n, out = len(src), r['items']
            assert (out[r['n_out']:] == 0).all() and (r['src_tok'][r['n_out']:] == -1).all()
            if n == 0:
                assert (r['n_out'], r['op'], r['target']) == (0, 0, -1)
                continue
            assert r['op'] in [ar.OPS[o] for o in names]
            seen[r['op']] += 1
            keep = out[:r['n_out']] != ar.MASK_ID
            assert np.array_equal(data[0][r['src_tok'][:r['n_out']]][keep] + ar.RESERVED, out[:r['n_out']][keep])
            if r['op'] == ar.CROP:
                Lc = max(1, ar.share(n, ratio['crop_ratio']))
                assert r['n_out'] == Lc
                assert any(np.array_equal(src[c:c + Lc], out[:Lc]) for c in range(n - Lc + 1))          # a contiguous slice
                assert (np.diff(r['src_tok'][:Lc]) == 1).all()
                if ratio['crop_ratio'] == 1.0:
                    assert np.array_equal(out[:n], src)
            elif r['op'] == ar.MASK:
                m = min(n, ar.share(n, ratio['mask_ratio']))
                assert r['n_out'] == n and int((out[:n] != src).sum()) == m and (out[:n][out[:n] != src] == ar.MASK_ID).all()
                if ratio['mask_ratio'] == 0.0:
                    assert np.array_equal(out[:n], src)
            else:
                Lr = min(n, ar.share(n, ratio['reorder_ratio']))
                tok = r['src_tok'][:n]
                i = int(tok.min())
                moved = np.flatnonzero(tok != i + np.arange(n))
                assert r['n_out'] == n and sorted(tok.tolist()) == list(range(i, i + n))                # a permutation of the row
                assert len(moved) == 0 or int(moved.max() - moved.min()) < Lr                            # ... of one span of Lr, the identity outside
                if ratio['reorder_ratio'] == 0.0:
                    assert np.array_equal(out[:n], src)
    assert all(c > 20 for c in seen.values()), seen


def test_a_row_depends_on_seed_view_and_window_alone(data):
    """not on its place in the batch, nor on the other rows, B or n_views"""
    items, offsets, V, per = data
    table, index = per[1]
    rows = ar.case_rows(table)
    kw = dict(holdout=1, max_len=ar.MAX_LEN, index=index, V=V)
    a = ar.batch(items, offsets, table, rows, ar.NEXT_TRAIN, 8, 2, 15, 9, **kw)
    perm = np.random.default_rng(0).permutation(len(rows))
    b = ar.batch(items, offsets, table, rows[perm], ar.NEXT_TRAIN, 8, 4, 15, 9, **kw)
    for k in ('items', 'src_tok', 'n_out', 'op', 'target'):
        assert np.array_equal(a[k][:, perm], b[k][:2]), k
    c = ar.batch(items, offsets, table, rows, ar.NEXT_TRAIN, 8, 2, 15, 10, **kw)
    assert not np.array_equal(a['items'], c['items']) and not np.array_equal(a['items'][0], a['items'][1])


# ---- the case list is not vacuous ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('holdout', [1, 2])
@pytest.mark.parametrize('layout', [ar.CLOZE, ar.NEXT_TRAIN], ids=['cloze', 'next'])
def test_every_op_occurs_among_the_case_rows_of_the_mix(data, holdout, layout):
    items, offsets, V, per = data
    table = per[holdout][0]
    for seed in ar.SEEDS:
        got = ar.batch(items, offsets, table, ar.case_rows(table), layout, 8, 2, 7, seed, holdout=holdout, max_len=ar.MAX_LEN)
        for op in (ar.CROP, ar.MASK, ar.REORDER):
            assert int((got['op'] == op).sum()) >= 2, (seed, op, got['op'])


@pytest.mark.parametrize('holdout', [1, 2])
def test_same_target_finds_a_partner_and_falls_back(data, holdout):
    """sequence 6's targets are repeated 5s and 6s: a partner at another position.  Rows whose target item is no other row's target
    fall back to themselves: every self row's list holds its own token alone, and there are some."""
    items, offsets, V, per = data
    table, index = per[holdout]
    partner = selfs = 0
    for seed in ar.SEEDS:
        for v in (0, 1):
            for w, (g, a, Lw), r in _rows_of(data, holdout, ar.NEXT_TRAIN, (('same_target',), {}), seed, v):
                if not r['n_out']:
                    continue
                assert r['op'] == ar.SAME_TARGET
                tok = r['src_tok'][:r['n_out']]
                assert r['target'] == int(items[tok[-1] + 1])                                        # the view ends in front of the same item
                first, n = ar.row_rule(ar.NEXT_TRAIN, int(offsets[g + 1] - offsets[g]), a, Lw, holdout, 8)
                own = int(offsets[g]) + first + n
                y = r['target']
                if r['self']:
                    assert index[1][index[0][y]:index[0][y + 1]].tolist() == [own] and tok[-1] + 1 == own
                    selfs += 1
                else:
                    assert tok[-1] + 1 != own and r['n_out'] == min(r['partner_q'], ar.MAX_LEN)
                    partner += g == 6
    assert partner >= 1 and selfs >= 1, (partner, selfs)


def test_same_target_self_row_of_sequence_3(ops, data):
    """sequence 3 = [4, 4, 8]: its one training row is [4] in front of the target 4.  Among the first seven sequences of the case
    data no other target is a 4, so the row is its own view (in the whole data set the 1100 random items of sequence 7 hold two
    more 4s, and the row finds them: asserted too)"""
    items, offsets, V, per = data
    small = (items[:offsets[7]], offsets[:8])
    index = ar.target_index(small[0], small[1], 1, V)
    table = ar.case_table(small[1], 1)
    (w,) = np.flatnonzero(table[0][:-1] == 3)
    g, a, Lw = (int(t[w]) for t in table)
    for seed in ar.SEEDS:
        r = ar.one_view(small[0], small[1], g, a, Lw, ar.NEXT_TRAIN, 8, 0, ar.SAME_TARGET, seed, holdout=1, max_len=ar.MAX_LEN, index=index, V=V)
        assert (r['self'], r['n_out'], r['target'], r['op']) == (1, 1, 4, ar.SAME_TARGET) and r['items'][0] == 4 + ar.RESERVED
        got = ops.augment_row_host(small[0], small[1], g, 8, ar.NEXT_TRAIN, 'same_target', seed, a=a, L=Lw, holdout=1, max_len=ar.MAX_LEN,
                                   target_index=index, V=V)
        assert got['self'] == 1 and np.array_equal(got['items'], r['items'])
        whole = ar.one_view(items, offsets, g, a, Lw, ar.NEXT_TRAIN, 8, 0, ar.SAME_TARGET, seed, holdout=1, max_len=ar.MAX_LEN,
                            index=per[1][1], V=V)
        assert whole['self'] == 0 and whole['partner_q'] in (877, 1079) and whole['n_out'] == ar.MAX_LEN


# ---- DeviceCloze's host count ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('holdout', [1, 2])
@pytest.mark.parametrize('objective,layout', [('cloze', ar.CLOZE), ('next_item', ar.NEXT_TRAIN)])
def test_host_token_count_equals_the_restatement(data, holdout, objective, layout):
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    items, offsets, V, per = data
    dc = DeviceCloze(items, offsets, V=V, device=None, max_len=ar.MAX_LEN, stride=ar.MAX_LEN, holdout=holdout)
    index = per[holdout][1]
    assert all(np.array_equal(x, y) for x, y in zip(dc.target_index()[:3], index))
    win = np.concatenate([np.arange(dc.n_windows), [-1, 0, 0]])
    for names, kw in _cases(layout):
        for W in (8, 3):
            got = dc.view_lengths(win, 2024, names, 2, objective, W, **kw)
            want = ar.batch(items, offsets, dc.windows, win, layout, W, 2, ar.ops_mask(names), 2024, holdout=holdout, max_len=ar.MAX_LEN,
                            index=index, V=V, **kw)
            assert np.array_equal(got, want['n_out']), (names, kw, W)
            assert [int(r.sum()) + 3 * len(win) for r in got] == [int(r.sum()) + 3 * len(win) for r in want['n_out']]
