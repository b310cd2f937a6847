"""Contrastive views built on the device (include/b4c.h; NO REFERENCE ORACLE: an extension -- the restatement is
tests/augment_ref.py, written from the header's text): every output of the kernel bit for bit on the case list of
test_augment_cpu.py, the smallest shapes where it can still go wrong, purity, DeviceCloze.views' host count and features, and
model.contrastive_loss with a device view on the padding-free layout.  Everything about the views is integer-exact: no tolerance
(numerical parity of the packed against the dense layout is the existing tests' business)."""
import numpy as np
import pytest
import torch

import augment_ref as ar
import next_item_ref as nref

pytestmark = pytest.mark.gpu

SENT = -777


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops as o
    return o


@pytest.fixture(scope='module')
def data(ops):
    items, offsets, V = nref.case_data()
    per = {h: (ar.case_table(offsets, h), ar.target_index(items, offsets, h, V)) for h in (1, 2)}
    return items, offsets, V, per, torch.from_numpy(items).cuda(), torch.from_numpy(offsets).cuda()


def _launch(data, layout, row_idx, table, W, n_views, mask, seed, holdout=1, max_len=ar.MAX_LEN, index=None, want_tok=True, want_target=True,
            **ratios):
    """b4c_augment_views into sentinel-filled buffers with two spare rows / columns -> numpy outputs cut to the written extent (the
    spare cells are checked here)"""
    from bert4clickpath_amd import _lib
    items_d, offsets_d, V = data[4], data[5], data[2]
    B = len(row_idx)
    R = n_views * B
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    tab = [dev(t, np.int32) for t in table]
    row_d = dev(row_idx, np.int32)
    idx = [None] * 3 if index is None else [dev(t, dt) for t, dt in zip(index, (np.int64, np.int64, np.int32))]
    out = torch.full((R + 2, W + 2), SENT, dtype=torch.int64, device='cuda')
    tok = torch.full((R + 2, W + 3), SENT, dtype=torch.int64, device='cuda')
    n_out, op, target = (torch.full((R + 2,), SENT, dtype=torch.int32, device='cuda') for _ in range(3))
    selfc = torch.full((3,), SENT, dtype=torch.int32, device='cuda')
    p = lambda t: None if t is None else t.data_ptr()
    r = {'crop_ratio': 0.6, 'mask_ratio': 0.3, 'reorder_ratio': 0.6, **ratios}
    _lib.check(_lib.lib().b4c_augment_views(p(items_d), p(offsets_d), p(tab[0]), p(tab[1]), p(tab[2]), p(row_d), B, W, layout, holdout, max_len,
                                            n_views, mask, r['crop_ratio'], r['mask_ratio'], r['reorder_ratio'], seed, p(idx[0]), p(idx[1]),
                                            p(idx[2]), V if index is not None else 0, p(out), W + 2, p(tok) if want_tok else None, W + 3,
                                            p(n_out), p(op), p(target) if want_target else None, p(selfc),
                                            torch.cuda.current_stream().cuda_stream), 'augment_views')
    torch.cuda.synchronize()
    out, tok, n_out, op, target, selfc = (t.cpu().numpy() for t in (out, tok, n_out, op, target, selfc))
    assert (out[R:] == SENT).all() and (out[:, W:] == SENT).all() and (n_out[R:] == SENT).all() and (op[R:] == SENT).all()
    assert (selfc[1:] == SENT).all() and selfc[0] >= 0
    assert ((tok[R:] == SENT).all() and (tok[:, W:] == SENT).all()) if want_tok else (tok == SENT).all()
    assert (target[R:] == SENT).all() if want_target else (target == SENT).all()
    return {'items': out[:R, :W].reshape(n_views, B, W), 'src_tok': tok[:R, :W].reshape(n_views, B, W) if want_tok else None,
            'n_out': n_out[:R].reshape(n_views, B), 'op': op[:R].reshape(n_views, B),
            'target': target[:R].reshape(n_views, B) if want_target else None, 'self_count': int(selfc[0])}


KEYS = ('items', 'src_tok', 'n_out', 'op', 'target')


def _same(got, want):
    for k in KEYS:
        assert got[k] is None or np.array_equal(got[k], want[k]), k
    assert got['self_count'] == want['self_count']


def _want(data, layout, rows, table, W, n_views, mask, seed, holdout=1, max_len=ar.MAX_LEN, index=None, **ratios):
    return ar.batch(data[0], data[1], table, rows, layout, W, n_views, mask, seed, holdout=holdout, max_len=max_len, index=index, V=data[2],
                    **ratios)


# ---- the kernel against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('holdout', [1, 2])
@pytest.mark.parametrize('layout', [ar.CLOZE, ar.NEXT_TRAIN], ids=['cloze', 'next'])
@pytest.mark.parametrize('config', ar.CONFIGS, ids=ar.config_id)
def test_views_equal_the_restatement(data, holdout, layout, config):
    """the case list of test_augment_cpu.py in one launch per seed: an empty row (index -1), the L = 0 window, W = 8 wider than
    every row, two views; NULL src_tok / target_out on the last seed"""
    names, ratios = config
    if 'same_target' in names and layout == ar.CLOZE:
        return                                                    # (refused: test_augment_cpu.py)
    table, index = data[3][holdout]
    index = index if 'same_target' in names else None
    rows = ar.case_rows(table)
    mask = ar.ops_mask(names)
    for k, seed in enumerate(ar.SEEDS):
        want = _want(data, layout, rows, table, 8, 2, mask, seed, holdout, index=index, **ratios)
        full = k < len(ar.SEEDS) - 1
        _same(_launch(data, layout, rows, table, 8, 2, mask, seed, holdout, index=index, want_tok=full, want_target=full, **ratios), want)
        assert (want['n_out'][:, -2:] == 0).all() and (want['op'][:, -2:] == 0).all()          # the empty row and the L = 0 window


def test_every_op_of_a_row_of_one_item(data):
    """n = 1: crop Lc = 1; mask m = 0 and 1; reorder spans of 0 and 1; the same-target row of one input"""
    table, index = data[3][1]
    for layout, seqs in ((ar.CLOZE, [1, 2]), (ar.NEXT_TRAIN, [2, 3])):
        rows = np.flatnonzero(np.isin(table[0][:-1], seqs))
        configs = [(('crop',), {'crop_ratio': 0.3}), (('mask',), {'mask_ratio': 0.3}), (('mask',), {'mask_ratio': 1.0}),
                   (('reorder',), {'reorder_ratio': 0.6}), (('reorder',), {'reorder_ratio': 1.0})]
        configs += [(('same_target',), {})] if layout == ar.NEXT_TRAIN else []
        for names, ratios in configs:
            idx = index if 'same_target' in names else None
            want = _want(data, layout, rows, table, 4, 2, ar.ops_mask(names), 5, index=idx, **ratios)
            assert 'same_target' in names or ((want['n_out'] == 1) & (want['op'] != 0)).any(), (layout, names)      # (a partner's row is longer)
            _same(_launch(data, layout, rows, table, 4, 2, ar.ops_mask(names), 5, index=idx, **ratios), want)


@pytest.mark.parametrize('layout', [ar.CLOZE, ar.NEXT_TRAIN], ids=['cloze', 'next'])
def test_a_row_of_300_items(data, layout):
    """W = 300: every thread loops more than once, MASK counts over 300 keys and REORDER's span (ratio 1) runs past 256 threads;
    the same-target partners lie in the 1100-item sequence"""
    table = (np.array([7, 7], np.int32), np.array([100, 640], np.int32), np.array([300, 300], np.int32))
    index = data[3][1][1]
    rows = np.array([0, 1, 0], np.int64)
    configs = [(('crop',), {}), (('mask',), {}), (('reorder',), {'reorder_ratio': 1.0}), (('reorder',), {}), (('crop', 'mask', 'reorder'), {})]
    configs += [(('same_target',), {})] if layout == ar.NEXT_TRAIN else []
    for names, ratios in configs:
        idx = index if 'same_target' in names else None
        want = _want(data, layout, rows, table, 300, 2, ar.ops_mask(names), 31, max_len=0, index=idx, **ratios)
        assert want['n_out'].max() == 300 or names in (('crop',), ('same_target',))
        _same(_launch(data, layout, rows, table, 300, 2, ar.ops_mask(names), 31, max_len=0, index=idx, **ratios), want)
        if 'same_target' in names:
            assert any(r['partner_q'] is not None for r in want['rows'].values())


def test_same_target_partner_is_clipped_to_the_most_recent_W(data):
    """sequence 3's target, a 4, occurs again at positions 877 and 1079 of the 1100-item sequence: with no max_len cap the view is the
    W = 8 items in front of one of them; with max_len = 5 the 5 in front"""
    table, index = data[3][1]
    rows = np.flatnonzero(table[0][:-1] == 3)
    for max_len, n in ((0, 8), (ar.MAX_LEN, 5)):
        want = _want(data, ar.NEXT_TRAIN, rows, table, 8, 4, ar.SAME_TARGET, 18, max_len=max_len, index=index)
        assert (want['n_out'] == n).all() and all(r['partner_q'] in (877, 1079) for r in want['rows'].values()) and want['self_count'] == 0
        assert len({r['partner_q'] for r in want['rows'].values()}) == 2
        _same(_launch(data, ar.NEXT_TRAIN, rows, table, 8, 4, ar.SAME_TARGET, 18, max_len=max_len, index=index), want)


def test_the_views_of_one_launch_are_those_of_smaller_launches(data):
    """the grid's second dimension only selects v: a launch of k = 1 .. 4 views gives the first k views of the launch of four"""
    table, index = data[3][2]
    rows = ar.case_rows(table)
    four = _launch(data, ar.NEXT_TRAIN, rows, table, 8, 4, 15, 123, holdout=2, index=index)
    _same(four, _want(data, ar.NEXT_TRAIN, rows, table, 8, 4, 15, 123, holdout=2, index=index))
    assert len({four['items'][v].tobytes() for v in range(4)}) == 4
    for k in (1, 2, 3):
        got = _launch(data, ar.NEXT_TRAIN, rows, table, 8, k, 15, 123, holdout=2, index=index)
        for key in KEYS:
            assert np.array_equal(got[key], four[key][:k]), (k, key)


def test_purity(data):
    """the same rows in a permuted batch order give the permuted outputs; two launches give the same bits"""
    table, index = data[3][1]
    rows = ar.case_rows(table)
    a = _launch(data, ar.NEXT_TRAIN, rows, table, 8, 2, 15, 9, index=index)
    again = _launch(data, ar.NEXT_TRAIN, rows, table, 8, 2, 15, 9, index=index)
    perm = np.random.default_rng(0).permutation(len(rows))
    b = _launch(data, ar.NEXT_TRAIN, np.concatenate([rows[perm], rows[:3]]), table, 8, 2, 15, 9, index=index)
    for key in KEYS:
        assert np.array_equal(a[key], again[key]), key
        assert np.array_equal(a[key][:, perm], b[key][:, :len(rows)]) and np.array_equal(a[key][:, :3], b[key][:, len(rows):]), key


# ---- DeviceCloze.views ---------------------------------------------------------------------------------------------------------------
def _device_cloze(data, features):
    from bert4clickpath_amd.cloze_batches import DeviceCloze, Feature
    items, offsets, V = data[:3]
    rng = np.random.default_rng(8)
    vals = {'ev_mask': (rng.integers(0, 7, len(items)), 7, 'event', 'mask'), 'ev_keep': (rng.integers(0, 5, len(items)), 5, 'event', 'keep'),
            'it_mask': (rng.integers(0, 9, V), 9, 'item', 'mask'), 'it_keep': (rng.integers(0, 3, V), 3, 'item', 'keep')}
    feats = {n: Feature(vals[n][0], vals[n][1], per=vals[n][2], on_mask=vals[n][3]) for n in features}
    return DeviceCloze(items, offsets, V=V, max_len=ar.MAX_LEN, stride=ar.MAX_LEN, holdout=2, features=feats), vals


@pytest.mark.parametrize('objective,features', [('cloze', ('ev_mask', 'it_keep', 'it_mask')), ('next_item', ('ev_keep', 'it_mask', 'ev_mask'))])
def test_device_cloze_views(data, objective, features):
    """views() of a Cloze and of a next-item batch: the kernel's outputs under the batch's width, the host count n_real_tokens equal
    to the device's (read back here only), every feature a numpy gather through src_tok"""
    dc, vals = _device_cloze(data, features)
    items = data[0]
    win = ar.case_rows(tuple(np.append(t, 0) for t in dc.windows))[:-2]
    if objective == 'next_item':
        win = np.concatenate([win, [-1]])                        # (an empty row; window_batch takes none)
    batch = dc.window_batch(win, seed=4) if objective == 'cloze' else dc.next_item_window_batch(win, seed=4)
    B, W = batch['items'].shape
    layout = ar.CLOZE if objective == 'cloze' else ar.NEXT_TRAIN
    kinds = (('crop', 'mask', 'reorder'), {'mask_ratio': 0.5}), (('same_target',), {})
    for names, ratios in (kinds if objective == 'next_item' else kinds[:1]):
        views = dc.views(batch, 77, ops=names, n_views=3, **ratios)
        index = ar.target_index(items, data[1], 2, data[2]) if 'same_target' in names else None
        want = _want(data, layout, win, dc.windows, W, 3, ar.ops_mask(names), 77, holdout=2, index=index, **ratios)
        assert len(views) == 3
        for v, view in enumerate(views):
            got = {k: view[k].cpu().numpy() for k in ('items', 'src_tok', 'op', 'target')}
            assert got['items'].shape == (B, W) and view['items'].dtype == torch.int64 and view['n_items'].dtype == torch.int32
            for k in got:
                assert np.array_equal(got[k], want[k][v]), (k, v)
            assert np.array_equal(view['n_items'].cpu().numpy(), want['n_out'][v])
            assert isinstance(view['n_real_tokens'], int) and view['n_real_tokens'] == int((view['items'] != 0).sum()) + 3 * B
            assert int(view['self_count'][0]) == want['self_count']
            tok, ids = got['src_tok'], got['items']
            assert set(view['features']) == set(features)
            for name in features:
                values, _, per, on_mask = vals[name]
                src = values[np.maximum(tok, 0)] if per == 'event' else values[items[np.maximum(tok, 0)]]
                exp = np.where(tok >= 0, src + 10, 0)
                if on_mask == 'mask':
                    exp[ids == 1] = 1
                assert np.array_equal(view['features'][name].cpu().numpy(), exp), (name, v)
        if 'mask' in names:
            assert any(bool((view['items'] == 1).any()) for view in views)
    with pytest.raises(ValueError, match='evaluation batch'):
        dc.views(next(iter(dc.eval_batches(4, limit=4))), 1)


# ---- the model: a device view on the padding-free layout ------------------------------------------------------------------------------
V, B, S = 300, 6, 24


def _model_and_batch(dtype):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    torch.manual_seed(0)
    d = 64
    model = ClickstreamTransformer({'items': ['asin']}, {'items': ['item%d' % i for i in range(V)]}, {'items': d}, SoftMaxHead([64, d], V),
                                   value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, dropout_rate=0.0,
                                   compute_dtype=dtype, attention='causal').to('cuda')
    rng = np.random.default_rng(2)
    lengths = rng.integers(6, 30, size=40)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    items = rng.integers(0, V, size=int(offsets[-1])).astype(np.int32)
    dc = DeviceCloze(items, offsets, V=V, max_len=S - 3, holdout=2)
    batch = next(iter(dc.next_item_batches(B, 21, 1, width=S - 3)))
    return model, dc, batch


def _spy_pack(model, monkeypatch):
    """note the layout every _masked_rows call of the model is asked for"""
    seen = []
    orig = model._masked_rows

    def rows(inputs, training, flat_idx, pack=False, n_real_tokens=None, **kw):
        seen.append((bool(pack), n_real_tokens))
        return orig(inputs, training, flat_idx, pack=pack, n_real_tokens=n_real_tokens, **kw)
    monkeypatch.setattr(model, '_masked_rows', rows)
    return seen


def test_contrastive_loss_takes_a_device_view_padding_free(ops, monkeypatch):
    model, dc, batch = _model_and_batch(torch.bfloat16)
    inputs = model._next_item_inputs(batch)
    view = dc.views(batch, 5, n_views=1)[0]
    assert view['n_real_tokens'] < batch['n_real_tokens']          # (crops are shorter)
    seen = _spy_pack(model, monkeypatch)
    loss = model.contrastive_loss(inputs, {'asin': view['items']}, temperature=0.5, similarity='cos', n_real_tokens=batch['n_real_tokens'],
                                  n_real_tokens_b=view['n_real_tokens'])
    assert seen == [(True, batch['n_real_tokens']), (True, view['n_real_tokens'])]
    model.zero_grad(set_to_none=True)
    loss.backward()
    assert np.isfinite(float(loss.detach())) and float(loss.detach()) > 0
    body = [n for n, _ in model.named_parameters() if not n.startswith('head.')]
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert body and set(body) <= set(grads), sorted(set(body) - set(grads))          # (the head is not part of this loss)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and any(float(g.abs().max()) > 0 for g in grads.values())
    # with the main loss every parameter has a gradient
    same = dc.views(batch, 5, ops='same_target', n_views=1)[0]
    total = model.next_item_loss(batch) + 0.1 * model.contrastive_loss(inputs, {'asin': same['items']}, same_target=same['target'],
                                                                       n_real_tokens=batch['n_real_tokens'],
                                                                       n_real_tokens_b=same['n_real_tokens'])
    model.zero_grad(set_to_none=True)
    total.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters()) and np.isfinite(float(total.detach()))


def test_without_the_count_the_second_view_is_dense_as_before(ops, monkeypatch):
    model, dc, batch = _model_and_batch(torch.bfloat16)
    inputs = model._next_item_inputs(batch)
    view = dc.views(batch, 5, n_views=1)[0]
    seen = _spy_pack(model, monkeypatch)
    a = model.contrastive_loss(inputs, {'asin': view['items']}, temperature=0.5, n_real_tokens=batch['n_real_tokens'])
    b = model.contrastive_loss(inputs, {'asin': view['items']}, temperature=0.5, n_real_tokens=batch['n_real_tokens'], n_real_tokens_b=None)
    assert seen == [(True, batch['n_real_tokens']), (False, None)] * 2
    assert torch.equal(a.detach(), b.detach()) and np.isfinite(float(a.detach()))
