"""ops.deterministic (on by default): ONE switch for a bit-reproducible training step.  Switched off, three reductions of
the step finish through float atomics (the vocabulary projection's dW / db, the embedding rows of runs that cross the kernel's
64-entry ranges, the LayerNorm dgamma / dbeta), so two runs of the same step differ in last bits; with the switch every one
of them takes a fixed-order form.  Two fresh runs of the same three optimizer steps -- bf16, padding-free layout, dropout, arena optimizer,
the projection's dW as a background sweep: bench.py's step -- must leave bit-identical arenas (parameters, both Adam moments)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V, B, S = 3000, 96, 64


def _run(steps, seed_model, two_features=False):
    from bert4clickpath_amd import input_pipeline, optim
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    torch.manual_seed(seed_model)
    chains, vocabs, dims = {'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': 128}
    if two_features:
        chains['actions'], vocabs['actions'], dims = ['act'], ['a%d' % i for i in range(20)], {'items': 96, 'actions': 32}
    m = ClickstreamTransformer(chains, vocabs, dims, SoftMaxHead([64, 128], V), value_to_head='[MASK]', num_encoder_layers=3,
                               num_attention_heads=2, dropout_rate=0.1, compute_dtype=torch.bfloat16).to('cuda')
    opt = optim.Adam(m.parameters())
    T.set_dropout_seed(777)
    losses = []
    for i in range(steps):
        b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=100 + i, min_len=10, n_extra_features=1 if two_features else 0, extra_vocab=20)
        feats = {'asin': torch.from_numpy(b['ids'])[:, 2:S - 1].contiguous().cuda()}
        if two_features:
            feats['act'] = torch.from_numpy(b['extra'][0])[:, 2:S - 1].contiguous().cuda()
        opt.zero_grad()
        loss = m.cloze_loss(feats, torch.from_numpy(b['labels_padded']).cuda(), training=True, max_masked_per_row=10,
                            n_real_tokens=int((b['ids'] != 0).sum()))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return losses, opt.arena.flat.clone(), opt.m.clone(), opt.v.clone()


@pytest.mark.parametrize('two_features', [False, True])
def test_two_runs_of_three_steps_are_bit_identical(two_features):
    from bert4clickpath_amd import ops
    prev = (ops.deterministic, ops.background_workgroups)
    ops.deterministic, ops.background_workgroups = True, 8
    try:
        a = _run(3, 5, two_features)
        b = _run(3, 5, two_features)
    finally:
        ops.deterministic, ops.background_workgroups = prev
    assert a[0] == b[0], (a[0], b[0])
    for what, x, y in zip(('parameters', 'first moments', 'second moments'), a[1:], b[1:]):
        assert torch.equal(x, y), '%s differ in %d of %d elements' % (what, int((x != y).sum()), x.numel())
    assert np.isfinite(a[0]).all() and a[0][2] < a[0][0] + 0.5


def test_the_fixed_order_forms_equal_the_atomic_ones_to_rounding():
    """the deterministic kernels compute the same sums (other order): one backward pass either way, gradients equal to fp32
    rounding of the reductions"""
    from bert4clickpath_amd import input_pipeline, ops, optim
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    grads = []
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=9, min_len=10)
    items = torch.from_numpy(b['ids'])[:, 2:S - 1].contiguous().cuda()
    labels = torch.from_numpy(b['labels_padded']).cuda()
    prev = (ops.deterministic, ops.background_workgroups)
    try:
        for det in (False, True):
            ops.deterministic, ops.background_workgroups = det, 8
            torch.manual_seed(3)
            m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': 128}, SoftMaxHead([64, 128], V),
                                       value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, dropout_rate=0.0,
                                       compute_dtype=torch.bfloat16).to('cuda')
            opt = optim.Adam(m.parameters())
            opt.zero_grad()
            m.cloze_loss({'asin': items}, labels, training=True, max_masked_per_row=10, n_real_tokens=int((b['ids'] != 0).sum())).backward()
            ops.join_side_work(opt.arena.ctx)
            torch.cuda.synchronize()
            grads.append({n: p.grad.detach().clone() for n, p in m.named_parameters()})
    finally:
        ops.deterministic, ops.background_workgroups = prev
    for n, g in grads[0].items():
        assert float((g - grads[1][n]).abs().max()) <= 2e-5 * float(g.abs().max()) + 1e-9, n
