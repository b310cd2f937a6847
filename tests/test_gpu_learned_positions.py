"""Learned positional embeddings (position_encoding='learned'; NO REFERENCE ORACLE: an extension -- the float64 restatement is
tests/paper_encoder_ref.py): the table's gradient kernel b4c_pos_table_bwd against float64 (dense and ragged layouts, dropout mask
of the forward, rows it must not touch, accumulation, repeatability), and the model behind the public keyword: float64 autograd,
packed against dense, one optimizer step, the table-length bound, a checkpoint round trip."""
import os
import tempfile

import numpy as np
import pytest
import torch

import paper_encoder_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops as o
    return o


@pytest.mark.parametrize('rate', [0.0, 0.3])
def test_kernel_dense_fp32_against_float64(ops, rate):
    B, S, d, seed = 5, 12, 32, 77
    g = torch.Generator().manual_seed(3)
    dout = torch.randn(B * S, d, generator=g)
    cu = torch.arange(B + 1, dtype=torch.int32) * S
    keep = torch.from_numpy(ops.keep_mask(seed, B * S * d, rate).reshape(B * S, d)) if rate > 0 else None
    want = pr.pos_table_grad(dout, cu, S, d, keep, rate)
    got = ops.pos_table_bwd(dout.cuda(), cu.cuda(), B, S, rate, seed, torch.zeros(S, d, device='cuda'))
    # fp32 sums of B terms (and one multiplication by 1 / (1 - rate)) of fp32 inputs
    terms = (dout.abs() * (keep if keep is not None else 1) / (1.0 - rate)).reshape(B, S, d).sum(0).double()
    err = (got.double().cpu() - want).abs()
    assert bool((err <= 2.0 ** -23 * (B + 2) * terms + 1e-30).all()), float(err.max())
    if rate > 0:
        assert float((want - pr.pos_table_grad(dout, cu, S, d)).abs().max()) > 0.1        # (the mask matters)


def _ragged(B, S, d):
    rng = np.random.default_rng(5)
    lens = rng.integers(2, 150, B)
    lens[3], lens[40] = 1, S                   # positions 150 .. S-1 are held by sequence 40 alone
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    g = torch.Generator().manual_seed(9)
    dout = torch.randint(-8, 9, (int(cu[-1]), d), generator=g).float()      # integers: every sum is exact in fp32
    return lens, cu, dout


def test_kernel_ragged_bf16_is_exact_accumulates_and_repeats(ops):
    B, S, d, rows = 70, 200, 128, 210
    lens, cu, dout = _ragged(B, S, d)
    want = pr.pos_table_grad(dout, cu, S, d)
    dd, cud = dout.bfloat16().cuda(), cu.cuda()
    assert ops.L.lib().b4c_pos_table_bwd_workspace_bytes(B, S, d) > S * d * 4       # more than one block of sequences per position
    sentinel = torch.arange(rows * d, dtype=torch.float32).reshape(rows, d) % 13 - 6
    table = sentinel.clone().cuda()
    table[:S] = 0
    ops.pos_table_bwd(dd, cud, B, S, 0.0, 0, table)
    assert torch.equal(table[:S].double().cpu(), want)                              # fp32 accumulation of exact inputs: equality
    assert torch.equal(table[S:].cpu(), sentinel[S:])                               # rows at and past S: not written
    assert torch.equal(want[150:], dout[int(cu[40]) + 150:int(cu[41])].double())    # one sequence alone
    # a shorter S: rows past it keep their contents, longer sequences give their first S rows
    t2 = sentinel.clone().cuda()
    t2[:100] = 0
    ops.pos_table_bwd(dd, cud, B, 100, 0.0, 0, t2)
    assert torch.equal(t2[:100].double().cpu(), want[:100]) and torch.equal(t2[100:].cpu(), sentinel[100:])
    # accumulation into what is there
    t3 = sentinel.clone().cuda()
    ops.pos_table_bwd(dd, cud, B, S, 0.0, 0, t3)
    assert torch.equal(t3[:S].double().cpu(), want + sentinel[:S].double())
    # repeatability, dropout on
    a = ops.pos_table_bwd(dd, cud, B, S, 0.25, 5, torch.zeros(S, d, device='cuda'))
    b = ops.pos_table_bwd(dd, cud, B, S, 0.25, 5, torch.zeros(S, d, device='cuda'))
    assert torch.equal(a, b) and not torch.equal(a, table[:S])
    # the row_of form (packed layout of sequences whose last token sits at S - 1, pads before it)
    row_of = torch.full((B, S), -1, dtype=torch.int32)
    want_gap = torch.zeros(S, d, dtype=torch.float64)
    for i in range(B):
        n, first = int(lens[i]), int(cu[i])
        pos = list(range(n - 1)) + [S - 1]
        row_of[i, pos] = torch.arange(first, first + n, dtype=torch.int32)
        want_gap[pos] += dout[first:first + n].double()
    got = ops.pos_table_bwd(dd, None, B, S, 0.0, 0, torch.zeros(S, d, device='cuda'), row_of=row_of.reshape(-1).cuda())
    assert torch.equal(got.double().cpu(), want_gap)


# ---- the model ------------------------------------------------------------------------------------------------------------
def _build(V, dims, L, H, head_dims, dtype, seed, dropout=0.0, **kw):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(seed)
    chains, vocabs = {'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}
    if 'actions' in dims:
        chains['actions'], vocabs['actions'] = ['act'], ['a%d' % i for i in range(20)]
    m = ClickstreamTransformer(chains, vocabs, dims, SoftMaxHead(list(head_dims), V), value_to_head='[MASK]', num_encoder_layers=L,
                               num_attention_heads=H, dropout_rate=dropout, compute_dtype=dtype, **kw)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias') or n.endswith('beta'):
                p.normal_(0, 0.05)
        if 'position_encoding' in kw:
            m.transformer.position_embedding.weight.mul_(10.0)        # (a table as large as the sinusoid: it matters to the loss)
    return m.cuda()


def _batch(B, S, V, seed, min_len=4, extra=0):
    from bert4clickpath_amd import input_pipeline
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=seed, min_len=min_len, n_extra_features=extra, extra_vocab=20)
    ids = torch.from_numpy(b['ids'])
    feats = {'asin': ids[:, 2:S - 1].contiguous().cuda()}
    if extra:
        feats['act'] = torch.from_numpy(b['extra'][0])[:, 2:S - 1].contiguous().cuda()
    return b, ids, feats, torch.from_numpy(b['labels_padded']).cuda()


@pytest.mark.parametrize('combine', ['concat', 'sum'])
def test_model_fp32_matches_float64(ops, combine):
    """Loss, the gradient of position_embedding.weight and every other gradient against float64 autograd (tolerances of
    tests/test_gpu_model.py's fp32 model).  On a tree without the feature the keyword is swallowed and the parameter does not exist."""
    V, L, H, B, S, MAXP = 50, 2, 2, 3, 12, 16
    dims = {'items': 32, 'actions': 32} if combine == 'sum' else {'items': 32}
    model = _build(V, dims, L, H, [24, 16], torch.float32, 7, feature_combine=combine, position_encoding='learned', max_positions=MAXP)
    b, ids, feats, labels = _batch(B, S, V, 7, extra=1 if combine == 'sum' else 0)
    loss = model.cloze_loss(feats, labels, training=True)
    loss.backward()
    Pt = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    assert 'transformer.position_embedding.weight' in Pt
    extra = {'actions': torch.from_numpy(b['extra'][0])} if combine == 'sum' else None
    ref, _ = pr.model_loss(ids, torch.from_numpy(b['labels']).long(), Pt, L, H, 2, extra_features=extra, combine=combine)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 2e-5
    for name, p in model.named_parameters():
        gr = Pt[name].grad
        if float(gr.abs().max()) < 1e-9:
            assert float(p.grad.abs().max()) < 1e-6, name
            continue
        err = float((p.grad.cpu().double() - gr).abs().max() / gr.abs().max())
        assert err < 2e-4, (name, err)
    gp = model.transformer.position_embedding.weight.grad
    assert float(gp[:S].abs().max()) > 0 and float(gp[S:].abs().max()) == 0


@pytest.mark.parametrize('layout', ['padded', 'packed'])
def test_bf16_both_layouts_under_the_gate_bound(ops, layout):
    """bf16, d_model 128, ragged batch: the loss (2e-3) and every gradient, position_embedding.weight among them, of the padded and of
    the packed layout against float64 under bf16_gates.BF16_GRAD_BOUND (L2 per tensor, the head trunk's and the blocks' ReLU patterns
    shared with the device pass), exact and with the path's bf16 rounding points emulated -- as tests/test_gpu_dff.py holds both
    layouts of the sinusoidal model.  The packed layout takes a row's position from packed_of: the closing [SEP] of every sequence sits
    at S - 1, pads before it."""
    from bf16_gates import BF16_GRAD_BOUND, GateRecorder, grad_errors
    V, L, H, B, S = 300, 2, 2, 12, 48
    model = _build(V, {'items': 128}, L, H, [32, 64], torch.bfloat16, 3, position_encoding='learned', max_positions=64)
    b, ids, feats, labels = _batch(B, S, V, 21, min_len=3)
    n_real = int((b['ids'] != 0).sum())
    assert n_real < 0.8 * B * S
    kw = {'packed': False} if layout == 'padded' else {'n_real_tokens': n_real}
    with GateRecorder(ops) as rec:
        loss = model.cloze_loss(feats, labels, training=True, max_masked_per_row=10, **kw)
    loss.backward()
    assert (model._packed is not None) == (layout == 'packed')
    token_rows = torch.from_numpy(np.flatnonzero(b['ids'].reshape(-1) != 0)).long()
    relu = rec.relu_for(L, 2, torch.from_numpy(b['flat_idx']).long(), B, S, token_rows=token_rows)
    n = 'transformer.position_embedding.weight'
    for what, ekw in (('fp64 + device gates', {}), ('bf16-emulating + device gates', {'emulate_bf16': True})):
        Pt = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
        ref, _ = pr.model_loss(ids, torch.from_numpy(b['labels']).long(), Pt, L, H, 2, relu=relu, **ekw)
        ref.backward()
        assert abs(float(loss.detach()) - float(ref.detach())) < 2e-3 * float(ref.detach()), what
        errs = grad_errors(model.named_parameters(), {k: Pt[k].grad for k, _ in model.named_parameters()})
        name, worst = max(errs.items(), key=lambda kv: kv[1])
        print('%s, %s: position table %.2f %%, worst tensor %s %.2f %%' % (layout, what, 100 * errs[n], name, 100 * worst))
        assert n in errs and worst < BF16_GRAD_BOUND, (what, name, worst)
    rec.check_flips()
    gp = model.transformer.position_embedding.weight.grad
    assert float(gp[S - 1].abs().max()) > 0 and float(gp[S:].abs().max()) == 0


def test_bf16_packed_step_with_dropout_repeats(ops):
    """two identical packed steps, dropout on: the same bits in the loss and in every gradient"""
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    V, L, H, B, S = 300, 2, 2, 12, 48
    model = _build(V, {'items': 128}, L, H, [32, 64], torch.bfloat16, 3, dropout=0.1, position_encoding='learned', max_positions=64)
    b, ids, feats, labels = _batch(B, S, V, 21, min_len=3)
    n_real = int((b['ids'] != 0).sum())
    out = []
    for _ in range(2):
        model.zero_grad()
        T.set_dropout_seed(17)
        loss = model.cloze_loss(feats, labels, training=True, max_masked_per_row=10, n_real_tokens=n_real)
        loss.backward()
        out.append((float(loss.detach()), {k: p.grad.detach().clone() for k, p in model.named_parameters()}))
    assert out[0][0] == out[1][0] and float(out[0][1]['transformer.position_embedding.weight'].abs().max()) > 0
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k


def test_one_adam_step_dense_and_row_lazy(ops):
    from bert4clickpath_amd import optim
    V, L, H, B, S, MAXP = 300, 1, 2, 8, 24, 40
    b, ids, feats, labels = _batch(B, S, V, 4)
    after = {}
    for lazy in (False, True):
        model = _build(V, {'items': 64}, L, H, [32], torch.bfloat16, 2, position_encoding='learned', max_positions=MAXP)
        w = model.transformer.position_embedding.weight
        before = w.detach().clone()
        table = model.transformer.embedding_layers['items'].weight
        opt = optim.Adam(model.parameters(), lazy_rows=[table] if lazy else ())
        opt.zero_grad()
        loss = model.cloze_loss(feats, labels, training=True, packed=False)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        now = model.transformer.position_embedding.weight.detach()
        assert bool((now[:S] != before[:S]).any(dim=1).all())            # every position of the batch moved
        assert torch.equal(now[S:], before[S:])                           # rows the batch did not reach: bit for bit
        after[lazy] = now.clone()
    assert torch.equal(after[True], after[False])


def test_table_length_bound(ops):
    from bert4clickpath_amd._lib import B4CError
    V, S = 60, 20
    b, ids, feats, labels = _batch(4, S, V, 1)
    ok = _build(V, {'items': 32}, 1, 2, [16], torch.float32, 1, position_encoding='learned', max_positions=S)
    assert float(ok.cloze_loss(feats, labels, training=False)) > 0
    short = _build(V, {'items': 32}, 1, 2, [16], torch.float32, 1, position_encoding='learned', max_positions=S - 1)
    launches = []
    real = ops.embed_concat_pe_fwd
    ops.embed_concat_pe_fwd = lambda *a, **k: launches.append(1) or real(*a, **k)
    try:
        with pytest.raises(B4CError):
            short.cloze_loss(feats, labels, training=False)
    finally:
        ops.embed_concat_pe_fwd = real
    assert not launches


def test_checkpoint_round_trip(ops):
    from bert4clickpath_amd import checkpoint
    kw = dict(position_encoding='learned', max_positions=24)
    a = _build(40, {'items': 32}, 1, 2, [16], torch.float32, 1, **kw)
    b = _build(40, {'items': 32}, 1, 2, [16], torch.float32, 2, **kw)
    wa, wb = a.transformer.position_embedding.weight, b.transformer.position_embedding.weight
    assert not torch.equal(wa, wb)
    with tempfile.TemporaryDirectory() as tmp:
        path = checkpoint.save_checkpoint(os.path.join(tmp, 'ckpt-pos'), a)
        checkpoint.load_checkpoint(path, b)
    assert torch.equal(wa, b.transformer.position_embedding.weight)
