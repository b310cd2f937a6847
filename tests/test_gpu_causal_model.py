"""The causal (left-to-right) encoder behind the public keyword attention='causal' (NO REFERENCE ORACLE: an extension -- the
float64 restatement is tests/causal_ref.py): the fp32 model with every dropout mask regenerated, under the [MASK] objective and
under the left-to-right objective (every real item position predicts the next item, cloze_loss(flat_idx=...)); the bf16 model at
d_model 128 under the gate bound; prefix consistency of the encodings; the packed layout against the dense one; the route of the
last layer (always the full layer) and predict_topk on it."""
import numpy as np
import pytest
import torch

import causal_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops as o
    return o


def _build(V, d, L, H, head_dims, dtype, seed, dropout=0.0, **kw):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(seed)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': d}, SoftMaxHead(list(head_dims), V),
                               value_to_head='[MASK]', num_encoder_layers=L, num_attention_heads=H, dropout_rate=dropout,
                               compute_dtype=dtype, **kw)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias') or n.endswith('beta'):
                p.normal_(0, 0.05)
    return m.cuda()


def _batch(B, S, V, seed, min_len=3):
    from bert4clickpath_amd import input_pipeline
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=seed, min_len=min_len)
    ids = torch.from_numpy(b['ids'])
    return b, ids, {'asin': ids[:, 2:S - 1].contiguous().cuda()}, torch.from_numpy(b['labels_padded']).cuda()


class _CountMQ:
    """counts the passes that take the masked-query last layer (tests/test_gpu_attn_dropout.py)"""

    def __init__(self, ops):
        self.ops, self.calls = ops, 0

    def __enter__(self):
        self._orig = self.ops.MQAttnBlockFn
        rec = self

        class Noting(self._orig):
            @staticmethod
            def apply(*a, **k):
                rec.calls += 1
                return rec._orig.apply(*a, **k)
        self.ops.MQAttnBlockFn = Noting
        return self

    def __exit__(self, *exc):
        self.ops.MQAttnBlockFn = self._orig


# ---- fp32 model against float64, every mask regenerated ---------------------------------------------------------------------------
@pytest.mark.parametrize('objective', ['mask', 'next_item'])
def test_fp32_model_matches_float64(ops, objective):
    """B = 4, S = 16, d = 64, H = 2, two layers, dropout 0.1, attention dropout 0.2.  Bounds: those of
    tests/test_gpu_attn_dropout.py::test_encoder_fp32_matches_fp64_with_every_mask_regenerated for the bidirectional encoder (1e-4
    absolute on the forward value -- here the loss --, 2e-4 of the largest entry on every gradient, 1e-5 absolute where the
    float64 gradient is identically zero).
    mask: the [MASK] targets in the sync-free form (max_masked_per_row).  next_item: flat_idx = every real item position but the
    last of its sequence, label = the item that follows -- the left-to-right objective on an unmasked batch."""
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    V, d, L, H, B, S, rate, a_rate = 60, 64, 2, 2, 4, 16, 0.1, 0.2
    model = _build(V, d, L, H, [24, 16], torch.float32, 7, dropout=rate, attention_dropout_rate=a_rate, attention='causal')
    b, ids, feats, labels = _batch(B, S, V, 7)
    if objective == 'mask':
        flat = torch.from_numpy(b['flat_idx']).long()
        lab = torch.from_numpy(b['labels']).long()
        T.set_dropout_seed(2025)
        loss = model.cloze_loss(feats, labels, training=True, max_masked_per_row=10)
    else:
        full = ids.clone()                                     # the unmasked batch: the labels go back to their positions
        full.view(-1)[torch.from_numpy(b['flat_idx']).long()] = torch.from_numpy(b['labels']).long() + 10
        ids = full
        feats = {'asin': ids[:, 2:S - 1].contiguous().cuda()}
        item = ids >= 10
        src = item[:, :-1] & item[:, 1:]                       # an item position followed by an item
        flat = (torch.arange(B * S).view(B, S)[:, :-1])[src]
        lab = ids[:, 1:][src] - 10
        assert flat.numel() > B and len(set((ids >= 10).sum(1).tolist())) > 1
        T.set_dropout_seed(2025)
        loss = model.cloze_loss(feats, lab.to(torch.int32).cuda(), training=True, flat_idx=flat.to(torch.int32).cuda())
    loss.backward()
    # the masks, in the order the model drew its seeds: embedding, then per layer residual 1, residual 2, attention
    stream = T._SeedStream(2025)
    n = B * S * d
    keep = {'emb': torch.from_numpy(ops.keep_mask(stream.next(), n, rate)).view(B, S, d)}
    keep_attn = []
    for i in range(L):
        keep['l%d.1' % i] = torch.from_numpy(ops.keep_mask(stream.next(), n, rate)).view(B, S, d)
        keep['l%d.2' % i] = torch.from_numpy(ops.keep_mask(stream.next(), n, rate)).view(B, S, d)
        keep_attn.append(ops.attn_keep_mask(stream.next(), B, H, S, a_rate))
    assert T.dropout_seeds.counter == stream.counter == 1 + 3 * L
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    ref, _ = cr.model_loss(ids, flat, lab, P, L, H, 2, rate=rate, attn_rate=a_rate, keep=keep, keep_attn=keep_attn)
    ref.backward()
    print('causal fp32 model (%s): loss %.6f, float64 %.6f' % (objective, float(loss), float(ref)))
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-4
    worst = 0.0
    for name, p in model.named_parameters():
        gr = P[name].grad
        if float(gr.abs().max()) < 1e-9:          # d / d key-bias is identically zero (softmax shift invariance; the masks keep it so)
            assert float(p.grad.abs().max()) < 1e-5, name
            continue
        e = float((p.grad.cpu().double() - gr).abs().max() / gr.abs().max())
        worst = max(worst, e)
        assert e < 2e-4, (name, e)
    print('causal fp32 model (%s): worst relative gradient error %.3e' % (objective, worst))
    # the bidirectional restatement is a different function of the same masks: the comparison can tell them apart
    import attn_dropout_ref as ad
    x0 = P['transformer.embedding_layers.items.weight'].detach()[ids]
    x0 = cr.tr.dropout(x0 * float(np.sqrt(np.float32(d))) + cr.tr.positional_encoding(S, d, x0.dtype)[None], rate, keep['emb'])
    Pd = {k[len('transformer.encoder.'):]: v.detach() for k, v in P.items() if k.startswith('transformer.encoder.')}
    bi = ad.encoder_forward(x0, (ids == 0), Pd, L, H, rate, a_rate, keep, keep_attn)
    ca = cr.encoder_forward(x0, (ids == 0), Pd, L, H, rate, a_rate, keep, keep_attn)
    assert float((bi - ca).abs().max()) > 1e-2


# ---- bf16 model, d_model 128 --------------------------------------------------------------------------------------------------------
def test_bf16_model_under_the_gate_bound(ops):
    """d = 128, H = 2, 24 x 200 token rows with the gradients in the optimizer's arena: the size at which the fused feed-forward and
    attention-tail kernels run (tests/test_gpu_ffn_act.py's model).  Loss within 2e-3 relative, every gradient tensor within
    bf16_gates.BF16_GRAD_BOUND (relative L2) of float64 evaluated with the device pass's own ReLU patterns; check_flips()."""
    from bf16_gates import BF16_GRAD_BOUND, GateRecorder, grad_errors
    from bert4clickpath_amd import optim
    V, d, L, H, B, S = 1000, 128, 2, 2, 24, 200
    model = _build(V, d, L, H, [64, 128], torch.bfloat16, 11, attention='causal')
    opt = optim.Adam(model.parameters())
    b, ids, feats, labels = _batch(B, S, V, 13, min_len=150)
    opt.zero_grad()
    with GateRecorder(ops) as rec, _CountMQ(ops) as mq:
        loss = model.cloze_loss(feats, labels, training=True, packed=False)
    loss.backward()
    ops.flush_pending_dw(opt.arena.ctx)
    ops.join_side_work(opt.arena.ctx)
    torch.cuda.synchronize()
    assert mq.calls == 0 and not rec.rows_only_last            # the full last layer
    relu = rec.relu_for(L, 2, torch.from_numpy(b['flat_idx']).long(), B, S)
    Pt = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    ref, _ = cr.model_loss(ids, torch.from_numpy(b['flat_idx']).long(), torch.from_numpy(b['labels']).long(), Pt, L, H, 2, relu=relu)
    ref.backward()
    rec.check_flips()
    print('causal bf16 model: loss %.6f, float64 %.6f' % (float(loss), float(ref)))
    assert abs(float(loss.detach()) - float(ref.detach())) < 2e-3 * float(ref.detach())
    errs = grad_errors(model.named_parameters(), {n: Pt[n].grad for n, _ in model.named_parameters()})
    name, worst = max(errs.items(), key=lambda kv: kv[1])
    print('causal bf16 model: worst gradient tensor %s %.2f %% (L2)' % (name, 100 * worst))
    assert worst < BF16_GRAD_BOUND, (name, worst)


# ---- prefix consistency ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('S,p', [(48, 20), (300, 31), (300, 270)])
def test_encodings_of_a_prefix_do_not_change(ops, dtype, S, p):
    """inference, dense layout: two batches that differ only in the item ids at the positions > p (the same real / pad pattern) give
    bit-identical encoder output rows <= p; with attention='bidirectional' they differ"""
    V, d, L, H, B = 200, 64, 2, 2, 3
    g = torch.Generator().manual_seed(S + p)
    ids = torch.randint(10, 10 + V, (B, S), generator=g)
    ids[:, 0], ids[:, 1], ids[:, S - 1] = 3, 4, 4
    ids[1, S - 9:S - 1] = 0                               # pads before the closing [SEP], behind p
    other = ids.clone()
    change = (torch.arange(S)[None, :] > p) & (ids >= 10)
    other[change] = 10 + (ids[change] - 10 + 1 + torch.randint(0, V - 1, (int(change.sum()),), generator=g)) % V
    assert bool((other[change] != ids[change]).all()) and torch.equal(other == 0, ids == 0) and torch.equal(other[:, :p + 1], ids[:, :p + 1])
    out = {}
    for kind in ('causal', 'bidirectional'):
        model = _build(V, d, L, H, [16], dtype, 5, attention=kind)
        with torch.no_grad():
            out[kind] = [model.transformer({'items': t.cuda()}, training=False).float().cpu() for t in (ids, other)]
        assert tuple(out[kind][0].shape) == (B, S, d)
    a, b_ = out['causal']
    assert torch.equal(a[:, :p + 1], b_[:, :p + 1])
    assert not torch.equal(a[:, p + 1:], b_[:, p + 1:])
    a, b_ = out['bidirectional']
    assert not torch.equal(a[:, :p + 1], b_[:, :p + 1])


# ---- packed against dense -----------------------------------------------------------------------------------------------------
def test_packed_equals_dense(ops):
    """bf16: the packed layout counts q and k inside the sequence, the dense one by position, and the pads between them carry no
    weight: one function.  Bounds of tests/test_gpu_packed.py::test_model_packed_equals_dense_and_oracle: loss 2e-3 relative,
    gradients 0.06 relative L2 (two bf16 evaluations of the same math), the first ranked item equal on more than 0.9 of the rows."""
    V, S, B = 300, 48, 12
    model = _build(V, 64, 2, 2, (32, 64), torch.bfloat16, 3, attention='causal')
    b, ids, feats, labels = _batch(B, S, V, 21)
    n_real = int((b['ids'] != 0).sum())
    assert n_real < 0.8 * B * S

    def run(**kw):
        model.zero_grad()
        loss = model.cloze_loss(feats, labels, training=True, max_masked_per_row=10, **kw)
        loss.backward()
        return float(loss), {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    l_dense, g_dense = run(packed=False)
    assert model._packed is None
    l_pack, g_pack = run(n_real_tokens=n_real)
    assert model._packed is not None and model._packed.T == n_real
    print('causal packed against dense: loss %.6f / %.6f' % (l_pack, l_dense))
    assert abs(l_pack - l_dense) < 2e-3 * abs(l_dense)
    for n in g_dense:
        den = float(g_dense[n].float().norm())
        if den < 1e-9 or n.endswith('mha.wk.bias'):
            continue
        e = float((g_pack[n].double() - g_dense[n].double()).norm() / g_dense[n].double().norm())
        assert e < 0.06, (n, e)
    # ranking: the two layouts agree on the first item of (nearly) every row, as the bidirectional model's do
    t_dense, _, _ = model.predict_topk(feats, 10, labels, packed=False)
    t_pack, _, _ = model.predict_topk(feats, 10, labels, n_real_tokens=n_real)
    assert float((t_dense[:, 0] == t_pack[:, 0]).float().mean()) > 0.9
    # the bidirectional model is another function of the same weights
    bi = _build(V, 64, 2, 2, (32, 64), torch.bfloat16, 3)
    assert abs(float(bi.cloze_loss(feats, labels, training=False)) - float(model.cloze_loss(feats, labels, training=False))) > 1e-3


# ---- the route of the last layer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_full_last_layer_and_predict_topk(ops, dtype):
    """rows_supported(...) is False for a causal encoder: cloze_loss and predict_topk evaluate the full last layer and gather its
    rows; predict_topk equals a top-k computed from the model's own full forward"""
    V, d, L, H, B, S, K = 40, 64, 2, 2, 6, 12, 5
    model = _build(V, d, L, H, [32], dtype, 9, attention='causal')
    with torch.no_grad():                                  # (logits that spread: the ranking depends on the encoding)
        model.head.output_layer.kernel.mul_(4.0)
    b, ids, feats, labels = _batch(B, S, V, 7)
    enc = model.transformer.encoder
    assert not enc.rows_supported(dtype) and not enc.rows_supported(dtype, True) and not enc.rows_route(dtype, False)
    with _CountMQ(ops) as mq:
        idx, hit, ndcg = model.predict_topk(feats, K, labels)
        loss = model.cloze_loss(feats, labels, training=True, max_masked_per_row=10)
        probs = model(feats, training=False)
    assert mq.calls == 0 and bool(torch.isfinite(loss))
    with torch.no_grad():
        full = model.transformer({'items': ids.cuda()}, training=False)                  # (B, S, d): the whole last layer
        rows = full.reshape(B * S, d)[torch.from_numpy(b['flat_idx']).long().cuda()]
        logits = model.head.logits(rows, out_fp32=True)[:, :V].float().cpu().numpy()
    order = np.argsort(-logits, axis=1, kind='stable')[:, :K + 1]
    top = np.take_along_axis(logits, order, 1)
    want = order[:, :K]
    # the order of two items is defined where their logits are apart (1e-3: far above the rounding of a 32-term dot product of either
    # dtype's kernels): the rows whose K + 1 leading logits are, decided on the reference ranking alone -- most of them
    clear = (top[:, :-1] - top[:, 1:] > 1e-3).all(1)
    assert clear.mean() > 0.5 and len(set(map(tuple, want[clear]))) > 1          # (and the ranking depends on the row)
    assert np.array_equal(idx.cpu().numpy()[clear], want[clear])
    lab = torch.from_numpy(b['labels']).long().numpy()
    assert np.array_equal((hit.cpu().numpy() > 0)[clear], (want == lab[:, None]).any(1)[clear])
    # the padded (B, M, V) output of model(...) ranks the same way (fp32: bf16 probabilities 1e-3 apart round to one number)
    valid = (labels[:, :probs.shape[1]] != -1).cpu().numpy()
    assert int(valid.sum()) == idx.shape[0]
    assert dtype == torch.bfloat16 or np.array_equal(np.argsort(-probs.detach().float().cpu().numpy()[valid], axis=1, kind='stable')[:, :K][clear], want[clear])
    # a bidirectional model of the same weights takes the masked-query route and ranks differently somewhere
    bi = _build(V, d, L, H, [32], dtype, 9)
    bi.load_state_dict(model.state_dict())
    ops.bump_weights_epoch()
    with _CountMQ(ops) as mq2:
        idx_bi, _, _ = bi.predict_topk(feats, K, labels)
    assert mq2.calls == 1
    assert not np.array_equal(idx_bi.cpu().numpy()[clear], want[clear])
