"""The BERT4Rec paper's model behind the public keywords, at toy size: learned positions, GELU feed-forward, the normalised
input stage (embedding_layernorm=True, embedding_scale=1.0) and the tied head with its transform
(ClozeMaskedItemPrediction([], V, transform='gelu_tanh')).  NO REFERENCE ORACLE: extensions -- the float64 restatement is
tests/paper_model_ref.py.  40 items, d = 64, 2 heads, 2 layers, feed-forward width 256, B = 6, S = 12 with ragged lengths."""
import os
import tempfile

import numpy as np
import pytest
import torch

import paper_model_ref as pm

pytestmark = pytest.mark.gpu

V, D, H, L, FF, B, S, MAXP = 40, 64, 2, 2, 256, 6, 12, 16
PAPER = dict(ffn_activation='gelu_tanh', position_encoding='learned', max_positions=MAXP, embedding_layernorm=True,
             embedding_scale=1.0)
REF = dict(ffn='gelu_tanh', transform='gelu_tanh', embedding_scale=1.0)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops as o
    return o


def _build(dtype, dropout=0.0, seed=7, head_dims=(), transform='gelu_tanh', d=D, **over):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, ClozeMaskedItemPrediction
    torch.manual_seed(seed)
    kw = dict(PAPER, **over)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': d},
                               ClozeMaskedItemPrediction(list(head_dims), V, transform=transform), value_to_head='[MASK]',
                               num_encoder_layers=L, num_attention_heads=H, encoder_ff_dim=FF, dropout_rate=dropout,
                               compute_dtype=dtype, **kw)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias') or n.endswith('beta'):
                p.normal_(0, 0.05)
            elif n.endswith('embedding_norm.gamma') or n.endswith('transform_norm.gamma'):
                p.add_(torch.randn_like(p) * 0.1)           # (a gamma of ones hides a gamma that is not applied)
    return m.cuda()


def _batch(seed=7, min_len=3):
    from bert4clickpath_amd import input_pipeline
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=seed, min_len=min_len)
    ids = torch.from_numpy(b['ids'])
    return b, ids, {'asin': ids[:, 2:S - 1].contiguous().cuda()}, torch.from_numpy(b['labels_padded']).cuda()


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _maxrel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


@pytest.fixture(scope='module')
def ref(ops):
    """the batch, and float64 loss and gradients of the seed-7 model on it: computed once, shared by the parity cases"""
    model = _build(torch.float32)
    b, ids, feats, labels = _batch()
    assert len(set((b['ids'] != 0).sum(1).tolist())) > 1          # ragged
    Pt = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    for k in ('transformer.embedding_norm.gamma', 'transformer.embedding_norm.beta', 'head.transform_norm.gamma',
              'head.transform_norm.beta', 'transformer.position_embedding.weight', 'head.intermediate_layers.0.kernel'):
        assert k in Pt, k
    loss, _ = pm.model_loss(ids, torch.from_numpy(b['labels']).long(), Pt, L, H, V, **REF)
    loss.backward()
    return dict(b=b, ids=ids, feats=feats, labels=labels, loss=float(loss.detach()), grads={k: Pt[k].grad for k in Pt},
                n_real=int((b['ids'] != 0).sum()))


def test_fp32_matches_float64(ops, ref):
    """cloze_loss within 1e-5, every gradient tensor within 2e-4 (max error over max magnitude): the table's holds the gather's
    gradient (through the LayerNorm) and the tied projection's"""
    model = _build(torch.float32)
    loss = model.cloze_loss(ref['feats'], ref['labels'], training=True)
    loss.backward()
    assert abs(float(loss.detach()) - ref['loss']) < 1e-5, (float(loss.detach()), ref['loss'])
    worst = {}
    for name, p in model.named_parameters():
        gr = ref['grads'][name]
        if float(gr.abs().max()) < 1e-9:
            assert float(p.grad.abs().max()) < 1e-6, name
            continue
        worst[name] = _maxrel(p.grad, gr)
    print('fp32 worst', max(worst.items(), key=lambda kv: kv[1]))
    assert max(worst.values()) < 2e-4, sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    assert set(ref['grads']) == set(n for n, _ in model.named_parameters())
    gp = model.transformer.position_embedding.weight.grad
    assert float(gp[:S].abs().max()) > 0 and float(gp[S:].abs().max()) == 0


def test_reference_composition_agrees_with_cloze_loss(ops, ref):
    from bert4clickpath_amd.clickstream_transformer.losses import sparse_categorical_crossentropy
    from bert4clickpath_amd.cloze import ClozeMaskedLoss
    model = _build(torch.float32)
    loss = ClozeMaskedLoss(sparse_categorical_crossentropy)(ref['labels'], model(ref['feats'], training=True))
    loss.backward()
    g_route = _grads(model)
    model.zero_grad()
    fused = model.cloze_loss(ref['feats'], ref['labels'], training=True)
    fused.backward()
    assert abs(float(loss.detach()) - float(fused.detach())) < 1e-5 and abs(float(loss.detach()) - ref['loss']) < 1e-5
    for n, g in _grads(model).items():
        gr = ref['grads'][n]
        if float(gr.abs().max()) < 1e-9:
            continue
        assert _maxrel(g_route[n], gr) < 2e-4 and _maxrel(g, gr) < 2e-4, n


def test_bf16_under_the_gradient_bound(ops, ref):
    """bf16: the loss within 2e-3 relative, every gradient tensor within bf16_gates.BF16_GRAD_BOUND (relative L2) of float64.  No
    ReLU anywhere in this configuration: no on / off pattern has to be shared with the device pass."""
    from bf16_gates import BF16_GRAD_BOUND, grad_errors
    model = _build(torch.bfloat16)
    loss = model.cloze_loss(ref['feats'], ref['labels'], training=True, packed=False)
    loss.backward()
    assert abs(float(loss.detach()) - ref['loss']) < 2e-3 * ref['loss'], (float(loss.detach()), ref['loss'])
    errs = grad_errors(model.named_parameters(), ref['grads'])
    name, worst = max(errs.items(), key=lambda kv: kv[1])
    print('bf16: loss %.6f (float64 %.6f), worst tensor %s %.2f %%; %s' % (
        float(loss.detach()), ref['loss'], name, 100 * worst,
        ', '.join('%s %.2f %%' % (k.split('.', 1)[1], 100 * errs[k]) for k in errs if 'norm' in k or 'embedding' in k)))
    for k in ('transformer.embedding_norm.gamma', 'head.transform_norm.beta', 'transformer.embedding_layers.items.weight',
              'transformer.position_embedding.weight'):
        assert k in errs
    assert worst < BF16_GRAD_BOUND, (name, worst)


def test_packed_dense_and_full_last_layer_agree(ops, ref):
    """bf16: the packed layout, the dense layout and the masked-query last layer switched off -- one loss (the bounds of
    tests/test_gpu_packed.py: 2e-3; tests/test_gpu_mq.py: 3e-3) and gradients (0.06 relative L2; 0.08 of the maximum)"""
    model = _build(torch.bfloat16)

    def run(**kw):
        model.zero_grad()
        loss = model.cloze_loss(ref['feats'], ref['labels'], training=True, max_masked_per_row=10, **kw)
        loss.backward()
        return float(loss), _grads(model), model._packed is not None
    l_dense, g_dense, pk = run(packed=False)
    assert not pk
    l_pack, g_pack, pk = run(n_real_tokens=ref['n_real'])
    assert pk and model._packed.T == ref['n_real'] < B * S
    ops.mq_last_layer = False
    try:
        l_full, g_full, _ = run(n_real_tokens=ref['n_real'])
    finally:
        ops.mq_last_layer = True
    assert abs(l_pack - l_dense) < 2e-3 * abs(l_dense) and abs(l_pack - l_full) < 3e-3 * abs(l_full)
    for n in g_dense:
        if float(g_dense[n].float().norm()) < 1e-9 or n.endswith('mha.wk.bias'):
            continue
        e = float((g_pack[n].double() - g_dense[n].double()).norm() / g_dense[n].double().norm())
        assert e < 0.06, (n, e)
        assert _maxrel(g_pack[n], g_full[n]) < 0.08, n
    # fp32 (dense layout only): the masked-query last layer against the full one
    m32 = _build(torch.float32)
    out = {}
    for mq in (True, False):
        ops.mq_last_layer = mq
        try:
            m32.zero_grad()
            loss = m32.cloze_loss(ref['feats'], ref['labels'], training=True)
            loss.backward()
            out[mq] = (float(loss), _grads(m32))
        finally:
            ops.mq_last_layer = True
    assert abs(out[True][0] - out[False][0]) < 2e-6 * abs(out[False][0])
    for n in out[True][1]:
        assert _maxrel(out[True][1][n], out[False][1][n]) < 2e-4 or float(out[False][1][n].abs().max()) < 1e-7, n


def _train(lazy, seed_model=11, steps=4):
    from bert4clickpath_amd import optim
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    model = _build(torch.bfloat16, dropout=0.1, seed=seed_model)
    table = model.transformer.embedding_layers['items'].weight
    opt = optim.Adam(model.parameters(), learning_rate=1e-3, weight_decay=0.01, exclude_from_weight_decay=optim.no_decay_params(model),
                     lazy_rows=[table] if lazy else ())
    T.set_dropout_seed(99)
    losses = []
    for i in range(steps):
        b, ids, feats, labels = _batch(seed=40 + i)
        opt.zero_grad()
        loss = model.cloze_loss(feats, labels, training=True, max_masked_per_row=10, n_real_tokens=int((b['ids'] != 0).sum()))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    if lazy:
        opt.sync_rows()
    torch.cuda.synchronize()
    # the new vectors are arena parameters like any other
    flat = opt.arena.flat
    for p in (model.transformer.embedding_norm.gamma, model.transformer.embedding_norm.beta, model.head.transform_norm.gamma,
              model.head.transform_norm.beta):
        assert flat.data_ptr() <= p.data_ptr() < flat.data_ptr() + flat.numel() * 4
    return losses, {n: p.detach().clone() for n, p in model.named_parameters()}


def test_training_with_dropout_lazy_equals_dense_and_repeats(ops):
    """four AdamW steps over different batches, dropout 0.1, packed layout: the row-lazy and the dense optimizer end with the same
    bits in every parameter, and so do two runs from one seed"""
    l_dense, p_dense = _train(False)
    l_lazy, p_lazy = _train(True)
    l_again, p_again = _train(False)
    assert np.isfinite(l_dense).all() and l_dense == l_lazy == l_again
    start = _build(torch.bfloat16, dropout=0.1, seed=11)
    for n, p in start.named_parameters():
        assert torch.equal(p_dense[n], p_lazy[n]), n
        assert torch.equal(p_dense[n], p_again[n]), n
        if 'norm' in n or 'position_embedding' in n:
            assert not torch.equal(p_dense[n], p.detach()), n          # (they train)


def _separate_scores(model):
    """output_bias = 0.5 * (a permutation of 0 .. V-1), item rows of the tied table shrunk: the V logits of a row lie at least
    ~0.4 apart, so neither their fp32 nor their bf16 probabilities tie among the leading items (tests/test_gpu_rank.py has the
    documented tie cases; this test is about the transform reaching every ranking route)"""
    with torch.no_grad():
        g = torch.Generator().manual_seed(1)
        model.head.output_bias.copy_((torch.randperm(V, generator=g).float() * 0.5).cuda())
        model.transformer.embedding_layers['items'].weight[10:10 + V].mul_(0.1)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_ranking_routes_see_the_transform(ops, ref, dtype):
    """predict_topk ids and the ids ranked through model(x, scores='lazy') == a stable argsort of the materialised model(x)
    probabilities of the same model (and of the float64 restatement's); score_candidates == the materialised logits at the
    listed items"""
    from bert4clickpath_amd.clickstream_transformer import ClozeScores
    from bert4clickpath_amd.cloze import ClozeMaskedRecall
    K = 5
    model = _build(dtype)
    _separate_scores(model)
    feats, labels = ref['feats'], ref['labels']
    with torch.no_grad():
        probs = model(feats, training=False)                          # (B, M, V), padded per sequence
        idx, hit, _ = model.predict_topk(feats, K, labels)
        lazy = model(feats, training=False, scores='lazy')
        rows = model._masked_rows(feats, False)[0]
        logits = model.head.logits(rows, out_fp32=True)[:, :V].float().cpu()
    valid = (labels[:, :probs.shape[1]] != -1).cpu().numpy()
    assert int(valid.sum()) == int((labels != -1).sum()) == idx.shape[0]
    p = probs.float().cpu().numpy()[valid]                            # [R, V] row-major, as predict_topk's rows
    want = np.argsort(-p, axis=1, kind='stable')[:, :K]
    top = np.take_along_axis(p, want, 1)
    assert bool((top[:, :-1] > top[:, 1:]).all())                     # (no ties among the leading items: the order is defined)
    assert np.array_equal(idx.cpu().numpy(), want)
    P64 = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    lg64 = pm.model_logits(ref['ids'], P64, L, H, V, **REF)
    assert np.array_equal(np.argsort(-lg64.numpy(), axis=1, kind='stable')[:, :K], want)
    if dtype == torch.bfloat16:                                       # the logits-free route: a head.ClozeScores
        assert isinstance(lazy, ClozeScores)
        lidx, _, _ = lazy.topk(K)                                     # one row per (sequence, slot): the padded (B, M) rows
        assert np.array_equal(lidx.cpu().numpy().reshape(valid.shape + (K,))[valid], want)
    else:                                                             # fp32 has no such route: the probabilities come back
        assert not isinstance(lazy, ClozeScores)
        assert np.array_equal(np.argsort(-lazy.float().cpu().numpy()[valid], axis=1, kind='stable')[:, :K], want)
    rec = ClozeMaskedRecall(K)
    rec.update_state(labels, lazy)
    assert abs(float(rec.result()) - float(hit.mean())) < 1e-6
    # score_candidates: the listed items' logits
    g = torch.Generator().manual_seed(3)
    cand = torch.stack([torch.randperm(V, generator=g)[:8] for _ in range(rows.shape[0])]).to(torch.int32)
    cand[0, 3] = -1
    sc = model.score_candidates(feats, cand.cuda()).cpu()
    want_sc = torch.gather(logits, 1, cand.clamp(min=0).long())
    ok = cand >= 0
    # fp32: the project's 1e-4 activation bar; bf16: two evaluations of a bf16 dot product of 64 terms beside an fp32 bias
    tol = 1e-4 if dtype == torch.float32 else 2.0 ** -7 * float((logits - model.head.output_bias.detach().float().cpu()).abs().max()) + 1e-3
    assert bool(torch.isnan(sc[~ok]).all()) and float((sc[ok] - want_sc[ok]).abs().max()) < tol
    assert float((sc[ok] - lg64.float()[:, :V].gather(1, cand.clamp(min=0).long())[ok]).abs().max()) < (1e-4 if dtype == torch.float32 else 0.05)


@pytest.mark.parametrize('transform,dims', [('relu', ()), ('gelu_tanh', ()), ('gelu', (32,)), ('relu', (32,))])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_head_alone(ops, transform, dims, dtype):
    """the head on its own rows against float64: trunk(), the CE loss (fp32 1e-5, bf16 2e-3 relative) and the gradients -- fp32
    2e-4 relative L2; bf16 under bf16_gates.BF16_GRAD_BOUND, float64 taking the device pass's own ReLU on / off patterns where the
    head holds a ReLU (bf16_gates.GateRecorder; the patterns may differ from float64's own only near zero: check_flips).
    transform='relu', and a relu(Dense(32)) in front of the transform's own Dense."""
    from bf16_gates import BF16_GRAD_BOUND, GateRecorder
    from bert4clickpath_amd import _lib
    from bert4clickpath_amd.clickstream_transformer import ClozeMaskedItemPrediction
    from bert4clickpath_amd.clickstream_transformer.transformer import _Embedding
    torch.manual_seed(5)
    R, d = 37, 64
    emb = _Embedding(V + 11, d)
    with torch.no_grad():
        emb.weight.mul_(8.0)
    head = ClozeMaskedItemPrediction(list(dims), V, item_embedding=emb.weight, input_dim=d, transform=transform)
    with torch.no_grad():
        for n, p in head.named_parameters():
            if n.endswith('bias') or n.endswith('beta'):
                p.normal_(0, 0.1)
            elif n.endswith('gamma'):
                p.add_(torch.randn_like(p) * 0.1)
    emb.cuda(), head.cuda()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(R, d, generator=g).bfloat16().float()
    y = torch.randint(0, V, (R,), generator=g)
    xd = x.to(dtype).cuda().requires_grad_(True)
    fp32 = dtype == torch.float32
    n_relu = len(dims) + (1 if transform == 'relu' else 0)
    with GateRecorder(ops) as rec:
        loss = head.cloze_ce(xd, y.to(torch.int32).cuda(), _lib.CE_TF)
    loss.backward()
    assert len(rec.patterns) == n_relu
    relu = rec.relu_for(0, n_relu, None, 0, 0) if (n_relu and not fp32) else pm.tr._relu
    hP = {k: v.detach().cpu().double().requires_grad_(True) for k, v in head.state_dict().items()}
    assert len([k for k in hP if k.endswith('.kernel')]) == len(dims) + 1 and 'transform_norm.gamma' in hP
    tab = emb.weight.detach().cpu().double().requires_grad_(True)
    xr = x.double().requires_grad_(True)
    want = pm.tr.sparse_ce_tf(torch.softmax(pm.tied_head_logits(xr, hP, tab, 10, V, transform, relu=relu), -1), y).mean()
    want.backward()
    if n_relu and not fp32:
        rec.check_flips()
    assert abs(float(loss.detach()) - float(want.detach())) < (1e-5 if fp32 else 2e-3 * float(want.detach()))
    with torch.no_grad():
        h = head.trunk(xd.detach())
        hx = x.double()
        for i in range(len(dims)):
            hx = torch.relu(hx @ hP['intermediate_layers.%d.kernel' % i] + hP['intermediate_layers.%d.bias' % i])
        i = len(dims)
        hw = pm.head_transform(hx, hP['intermediate_layers.%d.kernel' % i], hP['intermediate_layers.%d.bias' % i],
                               hP['transform_norm.gamma'], hP['transform_norm.beta'], transform)
    # bf16: the activation and the result are rounded once each (2^-9 of values up to ~4, the first amplified by rstd * gamma ~ 2),
    # on top of the bf16 operands of the Dense layers: 0.05 absolute is three times that
    assert tuple(h.shape) == (R, d) and float((h.double().cpu() - hw).abs().max()) < (1e-4 if fp32 else 0.05)
    refs = dict({'head.' + k: v.grad for k, v in hP.items()}, table=tab.grad, x=xr.grad)
    got = dict({'head.' + n: p.grad for n, p in head.named_parameters()}, table=emb.weight.grad, x=xd.grad)
    assert set(got) == set(refs)
    errs = {n: float((got[n].double().cpu() - refs[n]).norm() / refs[n].norm()) for n in got}
    print(transform, dims, dtype, 'worst gradient', max(errs.items(), key=lambda kv: kv[1]))
    for n, e in errs.items():
        assert e < (2e-4 if fp32 else BF16_GRAD_BOUND), (n, e)


def test_checkpoint_round_trip(ops):
    from bert4clickpath_amd import checkpoint
    a, b = _build(torch.float32, seed=1), _build(torch.float32, seed=2)
    names = ('transformer.embedding_norm.gamma', 'transformer.embedding_norm.beta', 'head.transform_norm.gamma',
             'head.transform_norm.beta', 'head.intermediate_layers.0.kernel')
    sa, sb = a.state_dict(), b.state_dict()
    for n in names:
        assert not torch.equal(sa[n], sb[n]), n
    with tempfile.TemporaryDirectory() as tmp:
        path = checkpoint.save_checkpoint(os.path.join(tmp, 'ckpt-paper'), a)
        checkpoint.load_checkpoint(path, b)
        # a model without the new ends does not take the file (and the other way round): the names are part of the format
        plain = _build(torch.float32, seed=3, transform=None, embedding_layernorm=False)
        with pytest.raises(KeyError):
            checkpoint.load_checkpoint(path, plain)
    sb = b.state_dict()
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n
    _, _, feats, labels = _batch()
    assert float(a.cloze_loss(feats, labels, training=False)) == float(b.cloze_loss(feats, labels, training=False))
