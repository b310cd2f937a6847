"""Side features of device-built batches (include/b4c.h; NO REFERENCE ORACLE: an extension -- the restatement is
tests/batch_features_ref.py): the kernel bit for bit on item rows that the real builders wrote, purity, every builder of
DeviceCloze(features=...), and two-feature models fed from such batches against the same losses on host-built inputs.
Everything about the batches is integer-exact: no tolerance.  Gradients of two routes through the same kernels differ only by the
order of float atomics: the two-route gates of tests/test_gpu_candidate_loss.py (fp32: 2 x 2e-4 of a gradient's largest entry,
2 x 1e-5 where it is identically zero)."""
import numpy as np
import pytest
import torch

import batch_features_ref as ref
import next_item_ref as nref

pytestmark = pytest.mark.gpu

SENT = -777
MAX_LEN = 5
POLICIES = [(ref.EVENT, ref.MASKED), (ref.ITEM, ref.MASKED), (ref.EVENT, ref.KEPT), (ref.ITEM, ref.KEPT)]


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops as o
    return o


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


@pytest.fixture(scope='module')
def data(ops):
    items, offsets, V, event, table = ref.case_data()
    return {'items': items, 'offsets': offsets, 'V': V, 'event': event, 'table': table, 'items_d': _dev(items, np.int32),
            'offsets_d': _dev(offsets, np.int64), 'event_d': _dev(event, np.int32), 'table_d': _dev(table, np.int32)}


def _table(offsets, holdout):
    """window_table's windows at max_len = stride = 5, and one window of no items (L = 0) of sequence 1 at the end"""
    from bert4clickpath_amd.cloze_batches import window_table
    w = window_table(np.diff(offsets), MAX_LEN, MAX_LEN, holdout)
    return tuple(np.concatenate([x, np.array([v], np.int32)]) for x, v in zip(w, (1, 0, 0)))


def _eval_table(offsets, drop):
    """DeviceCloze's evaluation rows as windows: sequence g's row ends at its target n_g - drop, the target included"""
    end = np.maximum(np.diff(offsets) - drop + 1, 0)
    start = np.maximum(end - MAX_LEN, 0)
    return np.arange(len(end), dtype=np.int32), start.astype(np.int32), (end - start).astype(np.int32)


def _case_rows(table):
    """<= 16 rows: every short sequence's windows, the repeated-item sequence, three windows of the 1100-item sequence (its first,
    one inside, its last), the 12-item sequence's first and last (a > 0), an empty row (negative index), the L = 0 window"""
    seq, start, _ = table
    pick = [int(w) for w in np.flatnonzero(np.isin(seq[:-1], [2, 3, 5, 6, 10]))]
    long_w = np.flatnonzero(seq[:-1] == 7)
    four = np.flatnonzero(seq[:-1] == 4)
    pick += [int(long_w[np.argmin(start[long_w])]), int(long_w[len(long_w) // 2]), int(long_w[0]), int(four[0]), int(four[-1]), -1,
             len(seq) - 1]
    assert len(pick) <= 16
    return np.array(pick, np.int64)


def _sources(data, policies):
    host = [(data['event'] if k == ref.EVENT else data['table'], k, m) for k, m in policies]
    dev = [data['event_d'] if k == ref.EVENT else data['table_d'] for k, m in policies]
    return host, dev


def _launch(data, layout, row_idx, table, W, items_in, policies, holdout=1, max_len=MAX_LEN, pad=2):
    """b4c_batch_features into sentinel-filled buffers with two spare rows and `pad` spare columns (ld_out = W + pad; odd W + 2:
    every other row starts off a 16-byte boundary) -> [numpy [B, W]]; the spare cells are checked here"""
    import ctypes as c
    from bert4clickpath_amd import _lib
    B, n = items_in.shape[0], len(policies)
    tab = [_dev(t, np.int32) for t in table] if table is not None else [None] * 3
    row_d = None if row_idx is None else _dev(row_idx, np.int32)
    _, srcs = _sources(data, policies)
    outs = [torch.full((B + 2, W + pad), SENT, dtype=torch.int64, device='cuda') for _ in policies]
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.lib().b4c_batch_features(
        p(data['items_d']), p(data['offsets_d']), p(tab[0]), p(tab[1]), p(tab[2]), p(row_d), B, W, layout, holdout, max_len, data['V'],
        p(items_in), items_in.stride(0), n, (c.c_void_p * n)(*[s.data_ptr() for s in srcs]), (c.c_int * n)(*[k for k, _ in policies]),
        (c.c_int * n)(*[m for _, m in policies]), (c.c_void_p * n)(*[o.data_ptr() for o in outs]), W + pad, torch.cuda.current_stream().cuda_stream),
        'batch_features')
    torch.cuda.synchronize()
    got = []
    for o in outs:
        o = o.cpu().numpy()
        assert (o[B:] == SENT).all() and (o[:, W:] == SENT).all()
        got.append(o[:B, :W])
    return got


def _item_rows(ops, data, case, rows, table, W, holdout):
    """the item rows of the case from the real builder -> (layout, table the feature kernel reads, items_in device [B, W])"""
    it, off = data['items_d'], data['offsets_d']
    row_d = _dev(rows, np.int32)
    if case in ('cloze_train', 'cloze_eval'):
        tab = [_dev(t, np.int32) for t in table]
        mode = ops.CLOZE_TRAIN if case == 'cloze_train' else ops.CLOZE_EVAL
        out, _, nm = ops.cloze_batch_windows(it, off, tab[0], tab[1], tab[2], row_d, W, mode, 1234, masked_percentage=0.4, max_masked=3)
        return ref.CLOZE, table, out, int(nm.sum().item())
    mode = nref.TRAIN if case == 'next_train' else nref.EVAL
    want = nref.batch(data['items'], data['offsets'], mode, rows, data['V'], table, holdout, MAX_LEN, W=None if W >= MAX_LEN else 1021)
    if W < MAX_LEN:                                                # rows cut at W: the target counts follow the cut
        per = [min(int(c), W) if mode == nref.TRAIN else int(c) for c in np.diff(want['row_off'])]
        want = {'row_off': np.concatenate([[0], np.cumsum(per)]).astype(np.int32), 'n_targets': int(np.sum(per))}
    tab = [_dev(t, np.int32) for t in table] if mode == nref.TRAIN else [None] * 3
    out = ops.next_item_batch(it, off, tab[0], tab[1], tab[2], row_d, _dev(want['row_off'], np.int32), W, mode, want['n_targets'], data['V'],
                              holdout=holdout, max_len=MAX_LEN)[0]
    return (ref.NEXT_TRAIN if mode == nref.TRAIN else ref.NEXT_EVAL), (table if mode == nref.TRAIN else None), out, 0


# ---- the kernel against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('holdout', [1, 2])
@pytest.mark.parametrize('W', [1, 5, 7])
@pytest.mark.parametrize('case', ['cloze_train', 'cloze_eval', 'next_train', 'next_eval'])
def test_kernel_equals_the_restatement(ops, data, case, W, holdout):
    """Every layout on the case list's rows -- L = 0, 1, 2, windows at a > 0 (the next-item lead input), the 1100-item sequence's
    windows, a negative row --, the item rows from the real builders; four features (both kinds x both mask policies) in one launch
    and each of them alone; W = 1, and odd W on a pitch of W + 2 (rows off the 16-byte boundary, a one-column tail); holdout is the
    EVAL rows' drop."""
    items, offsets = data['items'], data['offsets']
    if case == 'cloze_eval':
        table = _eval_table(offsets, holdout)
        rows = np.array(list(range(len(offsets) - 1)) + [-1], np.int64)
    elif case == 'next_eval':
        table, rows = None, np.array(list(range(len(offsets) - 1)) + [-1], np.int64)
    else:
        table = _table(offsets, holdout)
        rows = _case_rows(table)
        picked = [(int(table[1][w]), int(table[2][w])) for w in rows if w >= 0]
        assert {0, 1, 2, MAX_LEN} <= set(L for _, L in picked) and any(a > 0 for a, _ in picked) and (rows < 0).any()
        assert sum(int(table[0][w]) == 7 for w in rows if w >= 0) == 3
    assert len(rows) <= 16
    layout, ftable, items_in, n_masked = _item_rows(ops, data, case, rows, table, W, holdout)
    host = items_in.cpu().numpy()
    assert (n_masked > 0) == (case == 'cloze_eval' or (case == 'cloze_train' and W >= 5)) and ((host == 1).sum() == n_masked)
    src_host, _ = _sources(data, POLICIES)
    want = ref.batch(items, offsets, layout, rows, W, host, src_host, ftable, holdout, MAX_LEN)
    got = _launch(data, layout, rows, ftable, W, items_in, POLICIES, holdout)
    for f, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (case, W, holdout, POLICIES[f])
    assert (want[0] != 0).sum() == (host != 0).sum() > 0
    if n_masked:                                                   # the policies differ exactly at the [MASK] positions
        assert (want[0][host == 1] == 1).all() and (want[1][host == 1] == 1).all()
        assert (want[2][host == 1] >= 10).all() and (want[3][host == 1] >= 10).all()
        assert np.array_equal(want[0][host != 1], want[2][host != 1]) and np.array_equal(want[1][host != 1], want[3][host != 1])
    for f, policy in enumerate(POLICIES):                          # one feature per launch, on a pitch of W (no spare column)
        alone = _launch(data, layout, rows, ftable, W, items_in, [policy], holdout, pad=0)
        assert np.array_equal(alone[0], want[f]), (case, W, holdout, policy)


@pytest.mark.parametrize('case', ['cloze_train', 'next_train'])
def test_row_win_null_names_the_windows_in_order(ops, data, case):
    """row_win NULL: row b is window b of a table of B windows"""
    items, offsets = data['items'], data['offsets']
    table = _table(offsets, 1)
    rows = _case_rows(table)
    rows = rows[rows >= 0]
    small = tuple(t[rows] for t in table)
    ident = np.arange(len(rows), dtype=np.int64)
    layout, _, items_in, _ = _item_rows(ops, data, case, ident, small, 7, 1)
    src_host, _ = _sources(data, POLICIES)
    want = ref.batch(items, offsets, layout, None, 7, items_in.cpu().numpy(), src_host, small, 1, MAX_LEN)
    got = _launch(data, layout, None, small, 7, items_in, POLICIES, 1)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and (want[1] != 0).sum() > 20


def test_a_feature_that_copies_the_items_is_the_item_row_of_every_builder(ops, data):
    """The builders and the feature kernel share one row geometry (csrc/batch_rows.h): with the single source (items, 'event',
    'mask') ops.batch_features returns exactly the item row the layout's builder has just written -- 0 in the pads, 1 at a [MASK],
    item + 10 elsewhere -- for Cloze TRAIN windows, next-item TRAIN windows and next-item EVAL sequences.  The case rows of
    tests/test_gpu_next_item.py (_case_rows is the same list here), W = 8: wider than any window, B <= 16."""
    W, it, off = 8, data['items_d'], data['offsets_d']
    table = _table(data['offsets'], 1)
    tab = [_dev(t, np.int32) for t in table]
    for case in ('cloze_train', 'next_train', 'next_eval'):
        rows = _case_rows(table) if case != 'next_eval' else np.array(list(range(len(data['offsets']) - 1)) + [-1], np.int64)
        assert len(rows) <= 16
        layout, ftable, items_in, n_masked = _item_rows(ops, data, case, rows, table, W, 1)
        win = tab if ftable is not None else [None] * 3
        out, = ops.batch_features(it, off, win[0], win[1], win[2], _dev(rows, np.int32), W, layout, items_in, [(it, 'event', 'mask')],
                                  holdout=1, max_len=MAX_LEN)
        assert torch.equal(out, items_in), case
        assert int((items_in >= 10).sum()) > 10 and (n_masked > 0) == (case == 'cloze_train') and int((items_in == 1).sum()) == n_masked


# ---- DeviceCloze -----------------------------------------------------------------------------------------------------------------
FEATURES = [('action', 'event', 'keep'), ('category', 'item', 'mask'), ('dwell', 'event', 'mask')]


def _dc(data, with_features=True, **kw):
    from bert4clickpath_amd.cloze_batches import DeviceCloze, Feature
    feats = None
    if with_features:
        feats = {name: Feature(data['event'] if per == 'event' else data['table'], ref.EVENT_SIZE if per == 'event' else ref.ITEM_SIZE,
                               per=per, on_mask=on_mask) for name, per, on_mask in FEATURES}
    return DeviceCloze(data['items'], data['offsets'], V=data['V'], features=feats, **kw)


def _check_features(data, b, layout, rows, W, table, holdout):
    """the batch's 'features' against the restatement on the batch's own item rows"""
    host = [(data['event'] if per == 'event' else data['table'], ref.KINDS[per], ref.ON_MASK[on_mask]) for _, per, on_mask in FEATURES]
    want = ref.batch(data['items'], data['offsets'], layout, rows, W, b['items'].cpu().numpy(), host, table, holdout, MAX_LEN)
    assert list(b['features']) == [name for name, _, _ in FEATURES]
    for (name, _, _), w in zip(FEATURES, want):
        t = b['features'][name]
        assert t.dtype == torch.int64 and t.is_cuda and tuple(t.shape) == tuple(b['items'].shape) == (len(rows), W)
        assert np.array_equal(t.cpu().numpy(), w), name
    return int((want[0] != 0).sum())


def test_a_row_does_not_depend_on_its_batch(ops, data):
    dc = _dc(data, max_len=MAX_LEN)
    rows = _case_rows((dc.windows.seq, dc.windows.start, dc.windows.len))[:-2]         # (the L = 0 window is not in dc's table)
    rows = np.concatenate([rows, rows])[:16]
    where = {}
    for build in (lambda r: dc.window_batch(r, seed=4, width=7), lambda r: dc.next_item_window_batch(r, seed=4, width=7)):
        big = build(rows)
        assert len(rows) == 16
        for b, w in enumerate(rows.tolist()):
            one = build([w])
            for name in big['features']:
                assert torch.equal(one['features'][name][0], big['features'][name][b]), (name, b, w)
            where.setdefault(w, set()).add(b)
    assert max(len(v) for v in where.values()) == 2               # the same window at two places of one batch


KEYS_CLOZE = {'items', 'labels_padded', 'n_masked', 'seq_idx', 'win_idx', 'n_real_tokens'}
KEYS_NEXT = {'items', 'flat_idx', 'labels', 'candidates', 'row_offsets', 'short', 'seq_idx', 'win_idx', 'n_targets', 'n_real_tokens'}


def _same_without_features(b, b0, keys):
    """the batch of a DeviceCloze without features=: exactly today's keys, the same tensors"""
    assert set(b0) == keys and set(b) == keys | {'features'}
    for k in keys:
        if isinstance(b0[k], torch.Tensor):
            assert torch.equal(b0[k], b[k]), k
        else:
            assert b0[k] == b[k], k


def test_every_builder_carries_the_features(ops, data):
    """batch, window_batch, train_batches, eval_batches, next_item_window_batch, next_item_batches, next_item_eval_batches: 'features'
    equals the restatement on the batch's own item rows; without features= the dicts are today's"""
    offsets = data['offsets']
    dc, dc0 = _dc(data, max_len=MAX_LEN, holdout=2), _dc(data, False, max_len=MAX_LEN, holdout=2)
    win = (dc.windows.seq, dc.windows.start, dc.windows.len)
    n = 0
    # Cloze
    seqs = [3, 10, 5, 0, 2]                                        # one training window each, or none
    b, b0 = dc.batch(seqs, 'train', seed=9, width=7), dc0.batch(seqs, 'train', seed=9, width=7)
    _same_without_features(b, b0, KEYS_CLOZE)
    n += _check_features(data, b, ref.CLOZE, b['win_idx'].cpu().numpy(), 7, win, 2)
    for split, drop in (('valid', 2), ('test', 1)):
        seqs = [7, 0, 1, 4, 6]
        b, b0 = dc.batch(seqs, 'eval', width=7, split=split), dc0.batch(seqs, 'eval', width=7, split=split)
        _same_without_features(b, b0, KEYS_CLOZE)
        n += _check_features(data, b, ref.CLOZE, np.array(seqs), 7, _eval_table(offsets, drop), 2)
        for b, b0 in zip(dc.eval_batches(6, width=5, split=split), dc0.eval_batches(6, width=5, split=split)):
            _same_without_features(b, b0, KEYS_CLOZE)
            n += _check_features(data, b, ref.CLOZE, b['seq_idx'].cpu().numpy(), 5, _eval_table(offsets, drop), 2)
    rows = _case_rows(win)[:-2]
    rows = rows[rows >= 0]
    b, b0 = dc.window_batch(rows, seed=5, width=6), dc0.window_batch(rows, seed=5, width=6)
    _same_without_features(b, b0, KEYS_CLOZE)
    assert int(b['n_masked'].sum().item()) > 5
    n += _check_features(data, b, ref.CLOZE, rows, 6, win, 2)
    for b, b0 in zip(dc.train_batches(8, 21, 2, width=5), dc0.train_batches(8, 21, 2, width=5)):
        _same_without_features(b, b0, KEYS_CLOZE)
        n += _check_features(data, b, ref.CLOZE, b['win_idx'].cpu().numpy(), 5, win, 2)
    # next item
    rows = np.concatenate([rows, [-1]])
    b, b0 = dc.next_item_window_batch(rows, seed=5, width=6, num_negatives=2), dc0.next_item_window_batch(rows, seed=5, width=6, num_negatives=2)
    _same_without_features(b, b0, KEYS_NEXT)
    n += _check_features(data, b, ref.NEXT_TRAIN, rows, 6, win, 2)
    for b, b0 in zip(dc.next_item_batches(8, 21, 2, width=5), dc0.next_item_batches(8, 21, 2, width=5)):
        _same_without_features(b, b0, KEYS_NEXT)
        n += _check_features(data, b, ref.NEXT_TRAIN, b['win_idx'].cpu().numpy(), 5, win, 2)
    for split, drop in (('valid', 2), ('test', 1)):
        for b, b0 in zip(dc.next_item_eval_batches(6, width=7, split=split), dc0.next_item_eval_batches(6, width=7, split=split)):
            _same_without_features(b, b0, KEYS_NEXT | {'target_seq_idx'})
            n += _check_features(data, b, ref.NEXT_EVAL, b['seq_idx'].cpu().numpy(), 7, None, drop)
    assert n > 200
    assert dc.inputs(b, 'asin').keys() == {'asin', 'action', 'category', 'dwell'} and dc.inputs(b, 'asin')['asin'] is b['items']
    assert dc0.inputs(b0, 'asin').keys() == {'asin'}


# ---- the model ------------------------------------------------------------------------------------------------------------------
V_TINY, CATS, ACTIONS = 60, 6, 4


@pytest.fixture(scope='module')
def tiny(ops):
    """14 click paths of 2 .. 19 events over 60 items, an action per event and a category per item"""
    rng = np.random.default_rng(8)
    lengths = rng.integers(2, 20, 14)
    d = {'items': rng.integers(0, V_TINY, int(lengths.sum())).astype(np.int32),
         'offsets': np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), 'V': V_TINY,
         'event': rng.integers(0, ACTIONS, int(lengths.sum())).astype(np.int32), 'table': rng.integers(0, CATS, V_TINY).astype(np.int32)}
    return d


def _tiny_dc(tiny, **kw):
    from bert4clickpath_amd.cloze_batches import DeviceCloze, Feature
    return DeviceCloze(tiny['items'], tiny['offsets'], V=V_TINY, max_len=12, features={
        'action': Feature(tiny['event'], ACTIONS, per='event', on_mask='keep'), 'category': Feature(tiny['table'], CATS, per='item')}, **kw)


def _model(combine, attention, seed=0):
    """items + categories, d = 24 + 8 (concat) or 32 and 32 (sum), 2 layers, a tied head; the batches' 'action' is not a model input"""
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, ClozeMaskedItemPrediction
    torch.manual_seed(seed)
    dims = {'items': 24, 'cats': 8} if combine == 'concat' else {'items': 32, 'cats': 32}
    m = ClickstreamTransformer({'items': ['asin'], 'cats': ['category']},
                               {'items': ['i%d' % i for i in range(V_TINY)], 'cats': ['c%d' % i for i in range(CATS)]}, dims,
                               ClozeMaskedItemPrediction([], V_TINY), value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2,
                               dropout_rate=0.0, feature_combine=combine, attention=attention).to('cuda')
    with torch.no_grad():
        m.head.output_bias.normal_(0, 0.3)
    return m


def _host_inputs(tiny, b, layout, rows, W, table, holdout):
    """{'asin', 'category'} built by the restatement from the batch's item rows, uploaded"""
    host = b['items'].cpu().numpy()
    cat = ref.batch(tiny['items'], tiny['offsets'], layout, rows, W, host, [(tiny['table'], ref.ITEM, ref.MASKED)], table, holdout, 12)[0]
    return {'asin': torch.from_numpy(host).cuda(), 'category': torch.from_numpy(cat).cuda()}


def _grads(model, loss):
    model.zero_grad(set_to_none=True)
    loss.backward()
    return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}


def _gate(g_got, g_ref):
    assert set(g_got) == set(g_ref)
    for n, gr in g_ref.items():
        if float(gr.abs().max()) < 1e-9:
            assert float(g_got[n].abs().max()) < 2 * 1e-5, n
        else:
            assert float((g_got[n] - gr).abs().max()) <= 2 * 2e-4 * float(gr.abs().max()), n


@pytest.mark.parametrize('combine', ['concat', 'sum'])
def test_cloze_loss_on_a_device_batch_equals_host_built_inputs(ops, tiny, combine):
    """cloze_loss(data.inputs(batch, 'asin'), ...) in the sync-free form against the same call on inputs the restatement built: the
    same ids through the same kernels, so the same loss; the category is [MASK] exactly where the item is"""
    dc = _tiny_dc(tiny)
    win = (dc.windows.seq, dc.windows.start, dc.windows.len)
    rows = np.arange(min(12, dc.n_windows))
    b = dc.window_batch(rows, seed=3, width=14)
    assert int(b['n_masked'].sum().item()) > 10
    assert torch.equal(b['features']['category'] == 1, b['items'] == 1) and not bool((b['features']['action'] == 1).any())
    model = _model(combine, 'bidirectional', seed=1)
    kw = dict(max_masked_per_row=dc.max_masked, n_real_tokens=b['n_real_tokens'])
    got = model.cloze_loss(dc.inputs(b, 'asin'), b['labels_padded'], **kw)
    g_got = _grads(model, got)
    host = model.cloze_loss(_host_inputs(tiny, b, ref.CLOZE, rows, 14, win, 1), b['labels_padded'], **kw)
    g_ref = _grads(model, host)
    print('cloze_loss %s: device batch %.9g, host-built %.9g' % (combine, float(got.detach()), float(host.detach())))
    assert float(got.detach()) == float(host.detach()) and np.isfinite(float(got.detach()))
    _gate(g_got, g_ref)
    assert float(g_got['transformer.embedding_layers.cats.weight'].abs().max()) > 0


@pytest.mark.parametrize('combine', ['concat', 'sum'])
@pytest.mark.parametrize('loss', ['full', 'bce'])
def test_next_item_loss_of_a_two_feature_model(ops, tiny, loss, combine):
    """next_item_loss(device batch) of a model with a second embedded feature against cloze_loss / candidate_loss on host-built inputs
    with the batch's flat_idx: the loss is equal, gradients inside the two-route gates.  (Without the side features this call
    raises: a one-feature model was all next_item_loss took.)"""
    dc = _tiny_dc(tiny)
    win = (dc.windows.seq, dc.windows.start, dc.windows.len)
    rows = np.arange(min(12, dc.n_windows))
    N = 0 if loss == 'full' else 5
    b = dc.next_item_window_batch(rows, seed=13, width=14, num_negatives=N)
    assert b['n_targets'] > 40 and not bool((b['features']['category'] == 1).any())
    model = _model(combine, 'causal', seed=2)
    got = model.next_item_loss(b, loss=loss)
    g_got = _grads(model, got)
    inputs = _host_inputs(tiny, b, ref.NEXT_TRAIN, rows, 14, win, 1)
    if loss == 'full':
        host = model.cloze_loss(inputs, b['labels'], flat_idx=b['flat_idx'], n_real_tokens=b['n_real_tokens'])
    else:
        host = model.candidate_loss(inputs, b['labels'], candidates=b['candidates'], loss=loss, flat_idx=b['flat_idx'],
                                    n_real_tokens=b['n_real_tokens'])
    g_ref = _grads(model, host)
    print('next_item_loss %s %s: device batch %.9g, host-built %.9g' % (loss, combine, float(got.detach()), float(host.detach())))
    assert float(got.detach()) == float(host.detach()) and np.isfinite(float(got.detach()))
    _gate(g_got, g_ref)
    assert float(g_got['transformer.embedding_layers.cats.weight'].abs().max()) > 0
    with pytest.raises(ops.B4CError, match="the feature 'category'"):
        model.next_item_loss({k: v for k, v in b.items() if k != 'features'}, loss=loss)
