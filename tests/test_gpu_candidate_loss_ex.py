"""The extended sampled-negative losses on the device (include/b4c.h: BPR, the weighted BCE of gBCE, the logQ
correction; NO REFERENCE ORACLE: an extension -- the float64 restatement and the derived bounds are tests/candidate_loss_ex_ref.py):
b4c_candidate_loss_fwd_ex and the unchanged b4c_candidate_loss_bwd on the grid of candidate_loss_ref.CASES, element by element; the
bit-identity of the first entry point with the shared kernel; the model's candidate_loss('bpr' | 'gbce', logq=, item_cdf=) against
float64 from the head's input rows on; next_item_loss with the new keywords; the row-lazy optimizer under 'bpr'.

Gate of the element-wise comparisons: the derived bound of candidate_loss_ex_ref.bounds times max(2, 2 x MEASURED_RATIO_EX), where
MEASURED_RATIO_EX = 0.056 is the worst distance of the restatement's float32 mode from float64 in units of that bound on these very
inputs and settings (measured on the CPU: tests/test_candidate_loss_ex_cpu.py::test_measured_ratio_ex_is_current) -- so the gate
is 2 x the bound.  An element whose bound is 0 (ignored rows, absent entries, rows no list names, a row without a present
negative under BPR, the one-entry softmax) must be exact."""
import functools

import numpy as np
import pytest
import torch

import candidate_loss_ex_ref as cx
import candidate_loss_ref as cl

pytestmark = pytest.mark.gpu

GATE = max(2.0, 2.0 * cx.MEASURED_RATIO_EX)
SENTINEL = -12345.0


@pytest.fixture(scope='module')
def ops():
    from bert4clickpath_amd import ops as o
    return o


def _check(name, got, ref, bound):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64) * GATE
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    assert np.isfinite(got).all(), '%s: non-finite values' % name
    err = np.abs(got - ref)
    bad = err > bound
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print('%s: worst |err| / gate = %.3f' % (name, ratio))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError('%s: %d of %d elements outside their gate (worst |err| / gate = %.3g); first at %s: got %.9g, ref %.9g, gate '
                             '%.3g' % (name, int(bad.sum()), bad.size, ratio, i, got[i], ref[i], bound[i]))


@functools.lru_cache(maxsize=None)
def _inputs(case, bf16):
    R, C, K, V, scale = case
    h, table, b, cand = cl.inputs(R, C, K, V, scale, bf16)
    rng = np.random.default_rng(7)
    G0 = (rng.standard_normal(table.shape).astype(np.float32), rng.standard_normal(V).astype(np.float32))
    valid = int(((cand[:, 0] >= 0) & (cand[:, 0] < V)).sum())
    gscale = float(np.float32(0.7 / max(valid, 1)))                # an upstream gradient of 0.7 folded in
    return h, table, b, cand, cx.corr_for(C, V), G0, gscale


@functools.lru_cache(maxsize=None)
def _reference(case, bf16, off, setting):
    """inputs, G0, float64 restatement and bounds of one grid point (computed once, never written to)"""
    V = case[3]
    kind, beta, with_corr, target = setting
    h, table, b, cand, corr, G0, gscale = _inputs(case, bf16)
    W = cl.operand_rows(table, off, V, bf16)
    g0 = (G0[0][off:off + V], G0[1])
    ref = cx.restate(h, W, b, cand, kind, beta=beta, corr=corr if with_corr else None, correct_target=target, gscale=gscale, G0=g0)
    return ref, cx.bounds(h, W, b, ref, kind, G0=g0, bf16=bf16)


def _launch(h, table, b, cand, off, bf16, G0, gscale, V, kind, beta=1.0, corr=None, flags=0, legacy=False, backward=True):
    """the forward (b4c_candidate_loss_fwd_ex, or b4c_candidate_loss_fwd with legacy=True) and b4c_candidate_loss_bwd through the
    binding with every pitch larger than its width -> host arrays (padding included)"""
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    dev = 'cuda'
    R, K = h.shape
    C = cand.shape[1]
    rows = table.shape[0]
    dt = torch.bfloat16 if bf16 else torch.float32
    st = torch.cuda.current_stream().cuda_stream
    hd = torch.full((R, K + 8), 3.0, dtype=dt, device=dev)
    hd[:, :K] = torch.from_numpy(h).to(dt)
    td = torch.full((rows, K + 4), 5.0, dtype=torch.float32, device=dev)
    td[:, :K] = torch.from_numpy(table)
    bd = torch.from_numpy(b).to(dev)
    cd = torch.zeros(R, C + 3, dtype=torch.int32, device=dev)
    cd[:, :C] = torch.from_numpy(cand)
    qd = None if corr is None else torch.from_numpy(corr).to(dev)
    item = torch.full((R,), SENTINEL, device=dev)
    g = torch.full((R, C + 5), SENTINEL, device=dev)
    sc = torch.full((R, C + 2), SENTINEL, device=dev)
    code = {'bce': _lib.CANDX_BCE, 'softmax': _lib.CANDX_SOFTMAX, 'bpr': _lib.CANDX_BPR}[kind]
    dtc = _lib.BF16 if bf16 else _lib.F32
    if legacy:
        assert beta == 1.0 and corr is None and flags == 0
        _lib.check(L.b4c_candidate_loss_fwd(hd.data_ptr(), K + 8, td.data_ptr(), K + 4, rows, off, bd.data_ptr(), cd.data_ptr(), C + 3, R, C,
                                            V, K, dtc, code, item.data_ptr(), g.data_ptr(), C + 5, sc.data_ptr(), C + 2, st), 'fwd')
    else:
        _lib.check(L.b4c_candidate_loss_fwd_ex(hd.data_ptr(), K + 8, td.data_ptr(), K + 4, rows, off, bd.data_ptr(), cd.data_ptr(), C + 3, R,
                                               C, V, K, dtc, code, beta, None if qd is None else qd.data_ptr(), flags, item.data_ptr(),
                                               g.data_ptr(), C + 5, sc.data_ptr(), C + 2, st), 'fwd_ex')
    out = dict(item=item, g=g, scores=sc)
    if backward:
        dh = torch.full((R, K + 8), 7.0, dtype=dt, device=dev)
        dtab = torch.full((rows, K + 4), SENTINEL, device=dev)
        dtab[:, :K] = torch.from_numpy(G0[0])
        dbias = torch.from_numpy(G0[1]).to(dev)
        gs = torch.tensor([gscale], dtype=torch.float32, device=dev)
        _lib.check(L.b4c_candidate_loss_bwd(hd.data_ptr(), K + 8, td.data_ptr(), K + 4, rows, off, cd.data_ptr(), C + 3, g.data_ptr(), C + 5,
                                            gs.data_ptr(), R, C, V, K, dtc, dh.data_ptr(), K + 8, dtab.data_ptr(), K + 4, dbias.data_ptr(),
                                            st), 'bwd')
        out.update(dh=dh, dtable=dtab, dbias=dbias)
    torch.cuda.synchronize()
    return {k: v.float().cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('off', cl.ROW_OFFS)
@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('setting', cx.SETTINGS, ids=cx.setting_id)
@pytest.mark.parametrize('case', cl.CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_kernels_against_float64(case, setting, bf16, off):
    from bert4clickpath_amd import _lib
    R, C, K, V, scale = case
    kind, beta, with_corr, target = setting
    h, table, b, cand, corr, G0, gscale = _inputs(case, bf16)
    ref, bd = _reference(case, bf16, off, setting)
    out = _launch(h, table, b, cand, off, bf16, G0, gscale, V, kind, beta, corr if with_corr else None,
                  _lib.CANDX_CORR_TARGET if target else 0)
    absent = (cand < 0) | (cand >= V)
    ignored = absent[:, 0]
    live = ~absent & ~ignored[:, None]
    # exact: the padding is untouched, ignored rows and absent entries are zeros, unnamed sink rows keep G0
    assert (out['g'][:, C:] == SENTINEL).all() and (out['scores'][:, C:] == SENTINEL).all()
    assert (out['dh'][:, K:] == 7.0).all() and (out['dtable'][:, K:] == SENTINEL).all()
    assert not out['g'][:, :C][~live].any() and not out['item'][ignored].any() and not out['dh'][:, :K][ignored].any()
    assert np.isnan(out['scores'][:, :C][~live]).all()
    named = np.zeros(table.shape[0], bool)
    named[cand[live] + off] = True
    assert np.array_equal(out['dtable'][:, :K][~named], G0[0][~named])
    assert np.array_equal(out['dbias'][~named[off:off + V]], G0[1][~named[off:off + V]])
    if kind == 'bpr':                                            # sigma of a difference; the target's is minus their sum
        assert (np.abs(out['g'][:, 1:C]) <= 1).all() and (out['g'][:, 0] <= 0).all() and (np.abs(out['g'][:, 0]) <= C - 1).all()
        none = ~ignored & ~live[:, 1:].any(1)                      # a valid target and no present negative: exactly nothing
        assert not out['item'][none].any() and not out['g'][:, :C][none].any() and not out['dh'][:, :K][none].any()
    else:
        assert (np.abs(out['g'][:, :C]) <= max(1.0, beta)).all()
    if scale > 1:                                                # the |s| = 100 case: a finite loss (and the bounds above)
        assert float(np.abs(ref['s']).max()) > 100 and np.isfinite(out['item']).all()
    if C == 1 and kind != 'bce':
        assert not out['item'].any() and np.array_equal(out['dtable'][:, :K], G0[0]) and np.array_equal(out['dbias'], G0[1])
    # within the gate: everything else (an element with bound 0 must be exact).  scores: the UNCORRECTED s
    tag = '%s %s %s off %d' % (case, cx.setting_id(setting), 'bf16' if bf16 else 'fp32', off)
    _check(tag + ' scores', np.where(live, out['scores'][:, :C], 0), ref['s'], bd['s'])
    _check(tag + ' item', out['item'], ref['item'], bd['item'])
    _check(tag + ' g', out['g'][:, :C], ref['g'], bd['g'])
    _check(tag + ' dh', out['dh'][:, :K], ref['dh'], bd['dh'])
    _check(tag + ' dtable', out['dtable'][off:off + V, :K], ref['dW'], bd['dW'])
    _check(tag + ' dbias', out['dbias'], ref['db'], bd['db'])


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('kind', cl.KINDS)
@pytest.mark.parametrize('case', cl.CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_first_entry_point_and_the_extended_one_agree_bit_for_bit(case, kind, bf16):
    """b4c_candidate_loss_fwd and b4c_candidate_loss_fwd_ex(beta = 1, corr = NULL, flags = 0): item_loss, g and scores, padding
    included (NaN where both hold NaN)"""
    V = case[3]
    h, table, b, cand, _, G0, gscale = _inputs(case, bf16)
    a = _launch(h, table, b, cand, 10, bf16, G0, gscale, V, kind, legacy=True, backward=False)
    c = _launch(h, table, b, cand, 10, bf16, G0, gscale, V, kind, backward=False)
    for name in ('item', 'g', 'scores'):
        assert np.array_equal(a[name].view(np.int32), c[name].view(np.int32)), name
    assert (a['g'][:, cand.shape[1]:] == SENTINEL).all() and np.isfinite(a['item']).all()


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _model(V, d, dtype, head, dims=(), seed=0, heads=2, **kw):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, ClozeMaskedItemPrediction, SampledSoftmaxHead
    torch.manual_seed(seed)
    hd = ClozeMaskedItemPrediction(list(dims), V) if head == 'tied' else SampledSoftmaxHead(list(dims), V, num_sampled=64)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': d}, hd, value_to_head='[MASK]',
                               num_encoder_layers=2, num_attention_heads=heads, dropout_rate=0.0, compute_dtype=dtype, **kw)
    if head == 'tied':
        hd.tie(m.transformer.embedding_layers['items'].weight)
    m = m.to('cuda')
    with torch.no_grad():
        m.head.output_bias.normal_(0, 0.3)
    return m


def _batch(B, S, V, seed, min_len=6):
    from bert4clickpath_amd import input_pipeline
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=seed, min_len=min_len)
    ids = torch.from_numpy(b['ids'])
    return b, ids, {'asin': ids[:, 2:S - 1].contiguous().cuda()}, torch.from_numpy(b['labels_padded']).cuda()


def _spy(model):
    """note the rows, the lists and the keywords head.candidate_loss is called with, and keep the rows' gradient"""
    seen = {}
    orig = model.head.candidate_loss

    def spy(x2d, cand, kind, unit_grad=False, **kw):
        if x2d.requires_grad:
            x2d.retain_grad()
        seen.update(rows=x2d, cand=cand, kind=kind, kw=kw)
        return orig(x2d, cand, kind, unit_grad, **kw)
    model.head.candidate_loss = spy
    return seen


def _head_operands(model, bf16):
    hd = model.head
    V = hd.output_vocab_size
    _, table, bias = hd._proj()
    off = hd._packs[-1].tied_offset
    return cl.operand_rows(table.detach().cpu().numpy(), off, V, bf16), bias.detach().cpu().numpy(), table, off


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('head', ['tied', 'sampled'])
@pytest.mark.parametrize('loss', ['bpr', 'gbce'])
def test_model_losses_against_float64(ops, loss, head, dtype):
    """candidate_loss(loss='bpr' | 'gbce', num_negatives=5, logq=, item_cdf=) through the model: the head is handed the kind, the
    beta of gSASRec's formula and the correction; the negatives are drawn by the cdf (never an item without mass); and from the rows
    that reach the head on -- loss, d rows, d bias, d table -- the device agrees with the float64 restatement inside the kernels'
    gate (the heads here have no trunk, so the rows are the kernels' h)."""
    from bert4clickpath_amd import cloze
    V, d, B, S, N = 200, 16, 6, 20, 5
    bf16 = dtype == torch.bfloat16
    model = _model(V, d, dtype, head, heads=1)                  # (d = 16: one head of the kernels' smallest depth)
    b, ids, feats, labels = _batch(B, S, V, 11)
    cnt = cx.item_counts(V, seed=1)
    logq = cloze.log_expected_count(torch.from_numpy(cnt), num_negatives=N, device='cuda')
    assert np.array_equal(logq.cpu().numpy(), cx.log_expected_count(cnt, N))
    cdf = torch.from_numpy(np.cumsum(cnt)).cuda()
    seen = _spy(model)
    out = model.candidate_loss(feats, labels, num_negatives=N, loss=loss, logq=logq, item_cdf=cdf, seed=5)
    out.backward()
    rows, cand = seen['rows'], seen['cand'].cpu().numpy()
    want = b['labels'].astype(np.int32)
    R = want.shape[0]
    assert cand.shape == (R, N + 1) and rows.shape[0] == R and np.array_equal(cand[:, 0], want)
    neg = cand[:, 1:]
    assert ((neg >= 0) & (neg < V)).all() and (neg != cand[:, :1]).all() and (cnt[neg] > 0).all()
    beta = 1.0
    if loss == 'gbce':
        alpha = N / (V - 1.0)
        beta = alpha * (0.75 * (1 - 1 / alpha) + 1 / alpha)
        assert seen['kind'] == 'bce' and abs(seen['kw']['beta'] - beta) < 1e-15 and 0.25 < beta < 0.3
    else:
        assert seen['kind'] == 'bpr' and 'beta' not in seen['kw']
    assert seen['kw']['corr'] is logq and seen['kw']['correct_target'] is False
    W, bias, table, off = _head_operands(model, bf16)
    h = rows.detach().float().cpu().numpy()
    kind = 'bce' if loss == 'gbce' else loss
    ref = cx.restate(h, W, bias, cand, kind, beta=float(np.float32(beta)), corr=logq.cpu().numpy())
    bd = cx.bounds(h, W, bias, ref, kind, bf16=bf16)
    tag = 'model %s %s %s' % (loss, head, 'bf16' if bf16 else 'fp32')
    _check(tag + ' loss', float(out.detach()), ref['loss'], bd['loss'])
    _check(tag + ' d rows', rows.grad.float().cpu().numpy(), ref['dh'], bd['dh'])
    _check(tag + ' d bias', model.head.output_bias.grad.cpu().numpy(), ref['db'], bd['db'])
    if head == 'sampled':                                      # (the tied table's gradient also holds the embedding layer's)
        _check(tag + ' d table', table.grad.cpu().numpy(), ref['dW'], bd['dW'])
    else:
        assert float(table.grad[off:off + V].abs().max()) > 0
    # the correction is in the loss: without it the value differs; the target's too: it differs again
    with torch.no_grad():
        kw = dict(candidates=torch.from_numpy(cand).cuda(), loss=loss)
        plain = float(model.candidate_loss(feats, labels, **kw))
        both = float(model.candidate_loss(feats, labels, logq=logq, correct_target=True, **kw))
        again = float(model.candidate_loss(feats, labels, logq=logq, **kw))
    assert again == float(out.detach()) and len({plain, both, again}) == 3
    ref2 = cx.restate(h, W, bias, cand, kind, beta=float(np.float32(beta)), corr=logq.cpu().numpy(), correct_target=True)
    _check(tag + ' loss, target corrected', both, ref2['loss'], cx.bounds(h, W, bias, ref2, kind, bf16=bf16)['loss'])


def test_gbce_at_t_0_is_bce_bit_for_bit(ops):
    V, d, B, S = 200, 16, 6, 20
    model = _model(V, d, torch.float32, 'tied', heads=1)
    b, ids, feats, labels = _batch(B, S, V, 3)
    seen = _spy(model)
    with torch.no_grad():
        a = model.candidate_loss(feats, labels, num_negatives=5, loss='bce', seed=2)
        assert seen['kw'] == {}
        c = model.candidate_loss(feats, labels, num_negatives=5, loss='gbce', gbce_t=0.0, seed=2)
        assert seen['kind'] == 'bce' and np.float32(seen['kw'].get('beta', 1.0)) == 1    # (alpha * (1 / alpha): 1 in fp32)
        e = model.candidate_loss(feats, labels, num_negatives=5, loss='gbce', seed=2)
    assert a.view(torch.int32).item() == c.view(torch.int32).item() and float(e) < float(a)
    with pytest.raises(ops.B4CError, match="'gbce' needs at least one negative"):
        model.candidate_loss(feats, labels, candidates=torch.from_numpy(b['labels'].astype(np.int32))[:, None].cuda(), loss='gbce')
    with pytest.raises(ops.B4CError, match='logq has 199 entries'):
        model.candidate_loss(feats, labels, num_negatives=5, loss='bpr', logq=torch.zeros(199, device='cuda'))


# ---- next-item batches --------------------------------------------------------------------------------------------------------------
def test_next_item_loss_hands_the_keywords_on(ops):
    """next_item_loss(batch, loss='bpr' | 'gbce', logq=) is candidate_loss called with the batch's own fields: the same bits"""
    import next_item_ref as nref
    from bert4clickpath_amd import cloze
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    items, offsets, V = nref.case_data()
    dc = DeviceCloze(items, offsets, V=V, max_len=20, holdout=1)
    model = _model(V, 64, torch.float32, 'tied', attention='causal', seed=2)
    cnt = dc.item_counts()
    N = 7
    logq = cloze.log_expected_count(cnt, num_negatives=N, device='cuda')
    cdf = torch.from_numpy(np.cumsum(cnt)).cuda()
    seq = dc.windows.seq          # 12 windows of up to 20 items: the long sequence's, the repeated-item sequence's, short ones
    rows = np.concatenate([np.flatnonzero(seq == 7)[:6], np.flatnonzero(np.isin(seq, [3, 4, 6, 8, 9, 10]))])[:12]
    bt = dc.next_item_window_batch(rows, seed=13, width=24, num_negatives=N, item_cdf=cdf)
    assert bt['n_targets'] > 20
    feats = {'asin': bt['items']}
    for kw in (dict(loss='bpr', logq=logq), dict(loss='gbce', gbce_t=0.5, logq=logq, correct_target=True), dict(loss='bpr')):
        got = model.next_item_loss(bt, **kw)
        model.zero_grad(set_to_none=True)
        got.backward()
        g_got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        host = model.candidate_loss(feats, bt['labels'], candidates=bt['candidates'], flat_idx=bt['flat_idx'],
                                    n_real_tokens=bt['n_real_tokens'], **kw)
        assert np.isfinite(float(got.detach())) and got.detach().view(torch.int32).item() == host.detach().view(torch.int32).item(), kw
        assert len(g_got) > 4 and all(bool(torch.isfinite(g).all()) for g in g_got.values())
    assert len({float(model.next_item_loss(bt, loss='bpr', logq=q, training=False).detach()) for q in (None, logq)}) == 2


# ---- the row-lazy optimizer -------------------------------------------------------------------------------------------------------
def _disjoint_lists(R, C, V, seed):
    """a permutation of the items dealt out: no item in two entries"""
    assert V >= R * C
    return np.random.default_rng(seed).permutation(V)[:R * C].reshape(R, C).astype(np.int32)


def _train_sampled(lazy, loss, **kw):
    """three steps of candidate_loss(loss) on SampledSoftmaxHead with pairwise disjoint lists (distinct labels included), the lists of
    step 2 disjoint from those of steps 1 and 3, which are the same: at step 3 every listed row is one step stale"""
    import bench
    from bert4clickpath_amd import optim
    V, d, B, S, C = 4000, 128, 8, 32, 6
    model = _model(V, d, torch.bfloat16, 'sampled', dims=(64, 128), seed=4)
    rows = [p for n, p in model.named_parameters() if 'embedding_layers' in n or n == 'head.output_embedding'] if lazy else []
    opt = optim.Adam(model.parameters(), order=bench.backward_order(model), lazy_rows=rows, learning_rate=1e-2)
    b, ids, feats, labels = _batch(B, S, V, 6)
    R = int((labels != -1.0).sum())
    lists = [_disjoint_lists(R, C, V // 2, 1), _disjoint_lists(R, C, V // 2, 2) + V // 2]
    lists.append(lists[0])
    losses, touched = [], []
    for c in lists:
        cand = torch.from_numpy(c).cuda()
        lab = labels.clone()
        lab[lab != -1.0] = cand[:, 0].float()                    # the labels are the lists' first column: all distinct
        opt.zero_grad()
        out = model.candidate_loss(feats, lab, candidates=cand, loss=loss, **kw)
        out.backward()
        touched.append((model.head.touched_rows().cpu().numpy(), np.unique(c)))
        opt.step()
        losses.append(float(out.detach()))
    opt.sync_rows()
    torch.cuda.synchronize()
    return losses, touched, opt.arena.flat.clone(), opt.m.clone(), opt.v.clone()


def test_row_lazy_adam_equals_dense_bit_for_bit_under_bpr(ops):
    logq = torch.from_numpy(cx.log_expected_count(cx.item_counts(4000, seed=2), 5)).cuda()
    dense = _train_sampled(False, 'bpr', logq=logq)
    lazy = _train_sampled(True, 'bpr', logq=logq)
    assert dense[0] == lazy[0], (dense[0], lazy[0])
    for what, x, y in zip(('parameters', 'first moments', 'second moments'), dense[2:], lazy[2:]):
        assert torch.equal(x, y), '%s differ in %d of %d elements' % (what, int((x != y).sum()), x.numel())
    for got, want in dense[1] + lazy[1]:
        assert np.array_equal(got, want)                         # touched_rows(): the unique listed ids
    assert len(set(lazy[0])) == 3 and all(np.isfinite(v) for v in lazy[0])
