"""Sampled-negative training losses over per-row candidate lists on the device (NO REFERENCE ORACLE: an extension -- the float64
restatement and the derived bounds are tests/candidate_loss_ref.py): the two kernels on a grid of shapes, element by element; the
reproducibility of disjoint lists; the list-wise softmax over the whole vocabulary against cloze_loss; the model's candidate_loss
against float64 from the head's input rows on; the NaN loss of contradicted inputs; the row-lazy optimizer; drawn lists, with
one exclusion list per sequence in the sync-free form too.

Gate of the element-wise comparisons: the derived bound of candidate_loss_ref.bounds times max(2, 2 x MEASURED_RATIO), where
MEASURED_RATIO = 0.063 is the worst distance of the restatement's float32 mode from float64 in units of that bound on these very
inputs (measured on the CPU: tests/test_candidate_loss_cpu.py::test_measured_ratio_is_current) -- so the gate is 2 x the bound.  An
element whose bound is 0 (ignored rows, absent entries, rows no list names, the one-entry softmax) must be exact."""
import functools

import numpy as np
import pytest
import torch

import candidate_loss_ref as cl

pytestmark = pytest.mark.gpu

GATE = max(2.0, 2.0 * cl.MEASURED_RATIO)
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
def _reference(case, bf16, off, kind):
    """inputs, G0, float64 restatement and bounds of one grid case (computed once, never written to)"""
    R, C, K, V, scale = case
    h, table, b, cand = cl.inputs(R, C, K, V, scale, bf16)
    W = cl.operand_rows(table, off, V, bf16)
    rng = np.random.default_rng(7)
    G0 = (rng.standard_normal(table.shape).astype(np.float32), rng.standard_normal(V).astype(np.float32))
    valid = int(((cand[:, 0] >= 0) & (cand[:, 0] < V)).sum())
    gscale = float(np.float32(0.7 / max(valid, 1)))                # an upstream gradient of 0.7 folded in
    ref = cl.restate(h, W, b, cand, kind, gscale=gscale, G0=(G0[0][off:off + V], G0[1]))
    bd = cl.bounds(h, W, b, ref, kind, G0=(G0[0][off:off + V], G0[1]), bf16=bf16)
    return h, table, b, cand, G0, gscale, ref, bd


def _launch(h, table, b, cand, off, kind, bf16, G0, gscale, V):
    """both entry points through the binding with every pitch larger than its width -> host arrays (padding included)"""
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
    item = torch.full((R,), SENTINEL, device=dev)
    g = torch.full((R, C + 5), SENTINEL, device=dev)
    sc = torch.full((R, C + 2), SENTINEL, device=dev)
    code = _lib.CAND_BCE if kind == 'bce' else _lib.CAND_SOFTMAX
    dtc = _lib.BF16 if bf16 else _lib.F32
    _lib.check(L.b4c_candidate_loss_fwd(hd.data_ptr(), K + 8, td.data_ptr(), K + 4, rows, off, bd.data_ptr(), cd.data_ptr(), C + 3, R, C, V,
                                        K, dtc, code, item.data_ptr(), g.data_ptr(), C + 5, sc.data_ptr(), C + 2, st), 'fwd')
    dh = torch.full((R, K + 8), 7.0, dtype=dt, device=dev)
    dtab = torch.full((rows, K + 4), SENTINEL, device=dev)
    dtab[:, :K] = torch.from_numpy(G0[0])
    dbias = torch.from_numpy(G0[1]).to(dev)
    gs = torch.tensor([gscale], dtype=torch.float32, device=dev)
    _lib.check(L.b4c_candidate_loss_bwd(hd.data_ptr(), K + 8, td.data_ptr(), K + 4, rows, off, cd.data_ptr(), C + 3, g.data_ptr(), C + 5,
                                        gs.data_ptr(), R, C, V, K, dtc, dh.data_ptr(), K + 8, dtab.data_ptr(), K + 4, dbias.data_ptr(), st),
               'bwd')
    torch.cuda.synchronize()
    return {k: v.float().cpu().numpy() for k, v in dict(item=item, g=g, scores=sc, dh=dh, dtable=dtab, dbias=dbias).items()}


@pytest.mark.parametrize('off', cl.ROW_OFFS)
@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('kind', cl.KINDS)
@pytest.mark.parametrize('case', cl.CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_kernels_against_float64(case, kind, bf16, off):
    R, C, K, V, scale = case
    h, table, b, cand, G0, gscale, ref, bd = _reference(case, bf16, off, kind)
    out = _launch(h, table, b, cand, off, kind, bf16, G0, gscale, V)
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
    if scale > 1:
        assert float(np.abs(ref['s']).max()) > 100               # the |s| = 100 case: finite loss, coefficients in [-1, 1]
        assert (np.abs(out['g'][:, :C]) <= 1).all()
    if C == 1 and kind == 'softmax':
        assert not out['item'].any() and np.array_equal(out['dtable'][:, :K], G0[0]) and np.array_equal(out['dbias'], G0[1])
    # within the gate: everything else (an element with bound 0 must be exact)
    tag = '%s %s %s off %d' % (case, kind, 'bf16' if bf16 else 'fp32', off)
    _check(tag + ' scores', np.where(live, out['scores'][:, :C], 0), ref['s'], bd['s'])
    _check(tag + ' item', out['item'], ref['item'], bd['item'])
    _check(tag + ' g', out['g'][:, :C], ref['g'], bd['g'])
    _check(tag + ' dh', out['dh'][:, :K], ref['dh'], bd['dh'])
    _check(tag + ' dtable', out['dtable'][off:off + V, :K], ref['dW'], bd['dW'])
    _check(tag + ' dbias', out['dbias'], ref['db'], bd['db'])


def _disjoint_lists(R, C, V, seed):
    """a permutation of the items dealt out: no item in two entries"""
    assert V >= R * C
    return np.random.default_rng(seed).permutation(V)[:R * C].reshape(R, C).astype(np.int32)


@pytest.mark.parametrize('kind', cl.KINDS)
def test_disjoint_lists_are_reproducible(kind):
    R, C, K, V = 64, 20, 128, 1500
    h, table, b, _ = cl.inputs(R, C, K, V, 0.3, True)
    cand = _disjoint_lists(R, C, V, 3)
    rng = np.random.default_rng(1)
    G0 = (rng.standard_normal(table.shape).astype(np.float32), rng.standard_normal(V).astype(np.float32))
    a = _launch(h, table, b, cand, 10, kind, True, G0, 1.0 / R, V)
    c = _launch(h, table, b, cand, 10, kind, True, G0, 1.0 / R, V)
    assert np.array_equal(a['dtable'], c['dtable']) and np.array_equal(a['dbias'], c['dbias']) and np.array_equal(a['dh'], c['dh'])
    assert not np.array_equal(a['dtable'][:, :K], G0[0])
    # every element received one add: G0 + the one product, rounded once
    W = cl.operand_rows(table, 10, V, True)
    ref = cl.restate(h, W, b, cand, kind, gscale=float(np.float32(1.0 / R)), G0=(G0[0][10:10 + V], G0[1]))
    bd = cl.bounds(h, W, b, ref, kind, G0=(G0[0][10:10 + V], G0[1]), bf16=True)
    _check('disjoint dtable', a['dtable'][10:10 + V, :K], ref['dW'], bd['dW'])
    _check('disjoint dbias', a['dbias'], ref['db'], bd['db'])


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _model(V, d, dtype, head, dims=(), seed=0, **kw):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, ClozeMaskedItemPrediction, SampledSoftmaxHead
    torch.manual_seed(seed)
    hd = ClozeMaskedItemPrediction(list(dims), V) if head == 'tied' else SampledSoftmaxHead(list(dims), V, num_sampled=64)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': d}, hd, value_to_head='[MASK]',
                               num_encoder_layers=2, num_attention_heads=2, dropout_rate=0.0, compute_dtype=dtype, **kw)
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
    """note the rows and the lists head.candidate_loss is called with, and keep the rows' gradient"""
    seen = {}
    orig = model.head.candidate_loss

    def spy(x2d, cand, kind, unit_grad=False):
        if x2d.requires_grad:
            x2d.retain_grad()
        seen['rows'], seen['cand'] = x2d, cand
        return orig(x2d, cand, kind, unit_grad)
    model.head.candidate_loss = spy
    return seen


def _head_operands(model, bf16):
    hd = model.head
    V = hd.output_vocab_size
    _, table, bias = hd._proj()
    off = hd._packs[-1].tied_offset
    return cl.operand_rows(table.detach().cpu().numpy(), off, V, bf16), bias.detach().cpu().numpy(), table, off


@pytest.mark.parametrize('form,head,dtype,N', [('sync_free', 'tied', torch.float32, 1), ('packed', 'sampled', torch.bfloat16, 20),
                                               ('causal', 'sampled', torch.float32, 20), ('causal', 'tied', torch.bfloat16, 1)])
def test_model_bce_against_float64(ops, form, head, dtype, N):
    """candidate_loss(loss='bce', num_negatives=N) through the model: the rows and lists that reach the head are what the form
    promises (the labels of cloze_loss in column 0, N distinct negatives that are not the label), and from those rows on -- loss,
    d rows, d bias, d table -- the device agrees with the float64 restatement inside the kernels' gate (the heads here have no
    trunk, so the rows are the kernels' h).  The encoder's backward from d rows is the path cloze_loss takes."""
    V, d, B, S = 500, 128, 12, 40
    bf16 = dtype == torch.bfloat16
    model = _model(V, d, dtype, head, attention='causal' if form == 'causal' else 'bidirectional')
    b, ids, feats, labels = _batch(B, S, V, 11)
    seen = _spy(model)
    want = torch.from_numpy(b['labels']).to(torch.int32)
    if form == 'causal':
        full = ids.clone()                                     # the unmasked batch; every item position predicts the next item
        full.view(-1)[torch.from_numpy(b['flat_idx']).long()] = torch.from_numpy(b['labels']).long() + 10
        feats = {'asin': full[:, 2:S - 1].contiguous().cuda()}
        item = full >= 10
        src = item[:, :-1] & item[:, 1:]
        flat = (torch.arange(B * S).view(B, S)[:, :-1])[src]
        want = (full[:, 1:][src] - 10).to(torch.int32)
        loss = model.candidate_loss(feats, want.cuda(), num_negatives=N, seed=5, flat_idx=flat.to(torch.int32).cuda())
    elif form == 'packed':
        loss = model.candidate_loss(feats, labels, num_negatives=N, seed=5, max_masked_per_row=10, packed=True,
                                    n_real_tokens=int((ids != 0).sum()))
        assert model._packed is not None
    else:
        loss = model.candidate_loss(feats, labels, num_negatives=N, seed=5, max_masked_per_row=10)
    loss.backward()
    rows, cand = seen['rows'], seen['cand'].cpu().numpy()
    R = want.shape[0]
    assert cand.shape == (rows.shape[0], N + 1) and rows.shape[0] == (R if form == 'causal' else B * 10)
    assert np.array_equal(cand[:R, 0], want.numpy()) and (cand[R:] == -1).all()
    neg = cand[:R, 1:]
    assert ((neg >= 0) & (neg < V)).all() and (neg != cand[:R, :1]).all()
    assert all(len(set(r.tolist())) == N for r in neg)
    W, bias, table, off = _head_operands(model, bf16)
    h = rows.detach().float().cpu().numpy()
    ref = cl.restate(h, W, bias, cand, 'bce')
    bd = cl.bounds(h, W, bias, ref, 'bce', bf16=bf16)
    tag = 'model %s %s N=%d' % (form, head, N)
    _check(tag + ' loss', float(loss.detach()), ref['loss'], bd['loss'])
    _check(tag + ' d rows', rows.grad.float().cpu().numpy(), ref['dh'], bd['dh'])
    _check(tag + ' d bias', model.head.output_bias.grad.cpu().numpy(), ref['db'], bd['db'])
    if head == 'sampled':                                      # (the tied table's gradient also holds the embedding layer's)
        _check(tag + ' d table', table.grad.cpu().numpy(), ref['dW'], bd['dW'])
    else:
        assert float(table.grad[off:off + V].abs().max()) > 0


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_softmax_over_every_item_equals_cloze_loss(ops, dtype):
    """A tied model, V = 200: candidate_loss(loss='softmax', candidates=[y, every other item]) is cloze_loss(variant='plain'), in the
    loss and in every parameter's gradient.  cloze_loss is the measured-against side; the tolerance is the sum of the two routes'
    gates against float64, which for model gradients are the suite's own: fp32 -- loss 1e-4 absolute, a gradient 2e-4 of its largest
    entry (1e-5 absolute where it is identically zero) (tests/test_gpu_causal_model.py); bf16 -- loss 2e-3 relative, a gradient
    bf16_gates.BF16_GRAD_BOUND in relative L2."""
    from bf16_gates import BF16_GRAD_BOUND, grad_errors
    V, d, B, S = 200, 64, 8, 24
    model = _model(V, d, dtype, 'tied', dims=(64,), seed=3)
    b, ids, feats, labels = _batch(B, S, V, 5, min_len=5)
    y = b['labels'].astype(np.int64)
    cand = torch.from_numpy(np.stack([np.concatenate([[t], np.setdiff1d(np.arange(V), [t])]) for t in y]).astype(np.int32))

    def grads(loss):
        model.zero_grad(set_to_none=True)
        loss.backward()
        return float(loss.detach()), {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}
    l_ref, g_ref = grads(model.cloze_loss(feats, labels, training=True, variant='plain'))
    l_got, g_got = grads(model.candidate_loss(feats, labels, candidates=cand, loss='softmax'))
    print('softmax over every item: %.6f, cloze_loss %.6f' % (l_got, l_ref))
    assert set(g_got) == set(g_ref)
    if dtype == torch.float32:
        assert abs(l_got - l_ref) <= 2 * 1e-4
    else:
        assert abs(l_got - l_ref) <= 2 * 2e-3 * abs(l_ref)
    if dtype == torch.bfloat16:                                # (p.grad holds the candidate route's gradients: the latest backward)
        errs = grad_errors(model.named_parameters(), g_ref)      # leaves out the key bias: rounding noise on both sides
        assert len(errs) >= len(g_ref) - 2 and max(errs.values()) <= 2 * BF16_GRAD_BOUND, errs
        return
    for n, gr in g_ref.items():
        gg = g_got[n]
        if float(gr.abs().max()) < 1e-9:
            assert float(gg.abs().max()) < 2 * 1e-5, n
        else:
            assert float((gg - gr).abs().max()) <= 2 * 2e-4 * float(gr.abs().max()), n


def test_contradicted_inputs_give_a_nan_loss(ops):
    V, d, B, S = 500, 128, 8, 40
    model = _model(V, d, torch.bfloat16, 'tied')
    b, ids, feats, labels = _batch(B, S, V, 2)
    n_real = int((ids != 0).sum())
    with torch.no_grad():
        good = model.candidate_loss(feats, labels, num_negatives=5, seed=1, max_masked_per_row=10, packed=True, n_real_tokens=n_real)
        bad = model.candidate_loss(feats, labels, num_negatives=5, seed=1, max_masked_per_row=10, packed=True, n_real_tokens=n_real + 3)
        assert torch.isfinite(good) and torch.isnan(bad)
        lab = torch.from_numpy(b['labels']).to(torch.int32)
        R = lab.shape[0]
        cand = torch.randint(0, V, (R, 4), dtype=torch.int32)
        cand[:, 0] = lab
        assert torch.isfinite(model.candidate_loss(feats, labels, candidates=cand, loss='softmax'))
        cand[R // 2, 0] = (lab[R // 2] + 1) % V                  # column 0 is not the label
        assert torch.isnan(model.candidate_loss(feats, labels, candidates=cand, loss='softmax'))
    with pytest.raises(ops.B4CError, match='exactly one'):
        model.candidate_loss(feats, labels)
    with pytest.raises(ops.B4CError, match='exactly one'):
        model.candidate_loss(feats, labels, candidates=cand, num_negatives=3)


def test_drawn_lists_respect_the_exclusions_and_the_seed(ops):
    from bert4clickpath_amd import cloze
    V, d, B, S, N = 300, 64, 8, 32, 50
    model = _model(V, d, torch.float32, 'tied')
    b, ids, feats, labels = _batch(B, S, V, 4)
    seen = _spy(model)
    ex = cloze.seen_items(feats['asin'])                         # (B, E): the user's own items
    with torch.no_grad():
        l1 = model.candidate_loss(feats, labels, num_negatives=N, exclude=ex, seed=9, row_base=1000)
        c1 = seen['cand'].clone()
        l2 = model.candidate_loss(feats, labels, num_negatives=N, exclude=ex, seed=9, row_base=1000)
        assert torch.equal(c1, seen['cand']) and l1.view(torch.int32).item() == l2.view(torch.int32).item()
        model.candidate_loss(feats, labels, num_negatives=N, exclude=ex, seed=9, row_base=2000)
        assert not torch.equal(c1, seen['cand'])
    # no negative of a row is an item of its sequence
    counts = (labels != -1.0).sum(1).cpu().numpy()
    seq = np.repeat(np.arange(B), counts)
    exn, cn = ex.cpu().numpy(), c1.cpu().numpy()
    assert cn.shape == (len(seq), N + 1)
    for r, s in enumerate(seq):
        assert not set(cn[r, 1:].tolist()) & set(exn[s][exn[s] >= 0].tolist()), r


def test_sync_free_form_takes_one_exclusion_list_per_sequence(ops):
    """max_masked_per_row runs the head on B x M rows, more than there are [MASK] positions: the rows past the last one have no
    sequence.  They are ignored rows (label -1) and must not index past the (B, E) lists."""
    from bert4clickpath_amd import cloze
    V, d, B, S, N = 300, 64, 8, 32, 20
    model = _model(V, d, torch.float32, 'tied')
    b, ids, feats, labels = _batch(B, S, V, 4)
    seen = _spy(model)
    ex = cloze.seen_items(feats['asin'])
    loss = model.candidate_loss(feats, labels, num_negatives=N, exclude=ex, seed=9, max_masked_per_row=10)
    loss.backward()
    assert torch.isfinite(loss) and seen['rows'].shape[0] == B * 10
    counts = (labels != -1.0).sum(1).cpu().numpy()
    seq = np.repeat(np.arange(B), counts)
    R = len(seq)
    assert R < B * 10
    exn, cn = ex.cpu().numpy(), seen['cand'].cpu().numpy()
    assert np.array_equal(cn[:R, 0], b['labels']) and (cn[R:] == -1).all()
    for r, s in enumerate(seq):
        assert not set(cn[r, 1:].tolist()) & set(exn[s][exn[s] >= 0].tolist()), r
    with torch.no_grad():                                      # the same rows without the cap: the same loss
        ref = model.candidate_loss(feats, labels, num_negatives=N, exclude=ex, seed=9)
    assert abs(float(ref) - float(loss.detach())) <= 1e-5 * abs(float(ref))


# ---- the row-lazy optimizer -------------------------------------------------------------------------------------------------------
def _train_sampled(lazy, log=None):
    """three steps of candidate_loss('bce') on SampledSoftmaxHead with pairwise disjoint lists (distinct labels included), the lists
    of step 2 disjoint from those of steps 1 and 3, which are the same: at step 3 every listed row is one step stale"""
    import bench
    from bert4clickpath_amd import ops as o, optim
    V, d, B, S, C = 4000, 128, 8, 32, 6
    model = _model(V, d, torch.bfloat16, 'sampled', dims=(64, 128), seed=4)
    rows = [p for n, p in model.named_parameters() if 'embedding_layers' in n or n == 'head.output_embedding'] if lazy else []
    opt = optim.Adam(model.parameters(), order=bench.backward_order(model), lazy_rows=rows, learning_rate=1e-2)
    b, ids, feats, labels = _batch(B, S, V, 6)
    R = int((labels != -1.0).sum())
    lists = [_disjoint_lists(R, C, V // 2, 1), _disjoint_lists(R, C, V // 2, 2) + V // 2]
    lists.append(lists[0])
    if log is not None:
        lz = model.head.output_embedding._b4c_lazy
        orig_cu, orig_fwd = lz.catch_up, o.candidate_loss_fwd
        lz.catch_up = lambda ids_, note=True: (log.append(('catch_up', ids_.clone(), note)), orig_cu(ids_, note))[1]
        o.candidate_loss_fwd = lambda *a, **k: (log.append(('fwd',)), orig_fwd(*a, **k))[1]
    losses, touched = [], []
    try:
        for c in lists:
            cand = torch.from_numpy(c).cuda()
            lab = labels.clone()
            lab[lab != -1.0] = cand[:, 0].float()                # the labels are the lists' first column: all distinct
            opt.zero_grad()
            loss = model.candidate_loss(feats, lab, candidates=cand, loss='bce')
            loss.backward()
            touched.append((model.head.touched_rows().cpu().numpy(), np.unique(c)))
            opt.step()
            losses.append(float(loss.detach()))
    finally:
        if log is not None:
            o.candidate_loss_fwd = orig_fwd
    opt.sync_rows()
    torch.cuda.synchronize()
    return losses, touched, opt.arena.flat.clone(), opt.m.clone(), opt.v.clone()


def test_row_lazy_adam_equals_dense_bit_for_bit(ops):
    dense = _train_sampled(False)
    log = []
    lazy = _train_sampled(True, log)
    assert dense[0] == lazy[0], (dense[0], lazy[0])
    for what, x, y in zip(('parameters', 'first moments', 'second moments'), dense[2:], lazy[2:]):
        assert torch.equal(x, y), '%s differ in %d of %d elements' % (what, int((x != y).sum()), x.numel())
    for got, want in dense[1] + lazy[1]:
        assert np.array_equal(got, want)                         # touched_rows(): the unique listed ids
    # the listed rows are caught up (and noted: the pass is differentiated) before the forward kernel reads them
    kinds = [e[0] for e in log]
    assert kinds == ['catch_up', 'fwd'] * 3
    for (_, ids_, note), (_, want) in zip(log[0::2], lazy[1]):
        assert note and np.array_equal(np.unique(ids_.cpu().numpy()), want)
    assert len(set(lazy[0])) == 3                                # the third step repeats the first lists on moved weights
