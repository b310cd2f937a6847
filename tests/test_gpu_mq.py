"""Masked-query attention (the last encoder layer of the Cloze path computed for the [MASK] rows only) -- kernels against an
fp64 restatement of transformer.py:64-97 for those rows, then the model with the masked-query last layer against the full
layer it replaces and against the oracle."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def _ragged(B, smax, mmax, H, dh, seed, dtype, with_empty=True):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(3, smax + 1, (B,), generator=g)
    lens[0] = smax
    nq = torch.randint(0 if with_empty else 1, mmax + 1, (B,), generator=g)
    nq[1 % B] = mmax
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    moff = torch.zeros(B + 1, dtype=torch.int32)
    moff[1:] = torch.cumsum(nq, 0)
    T, R, d = int(cu[-1]), int(moff[-1]), H * dh
    q = (torch.randn(R, d, generator=g) * 0.8).to(dtype)
    kv = (torch.randn(T, 2 * d, generator=g) * 0.8).to(dtype)
    go = torch.randn(R, d, generator=g).to(dtype)
    return cu, moff, q, kv, go


def _ref(cu, moff, q, kv, go, H, dh, key_pad=None):
    q64 = q.double().clone().requires_grad_(True)
    kv64 = kv.double().clone().requires_grad_(True)
    d = H * dh
    outs, lses = [], []
    for b in range(len(cu) - 1):
        t0, t1, r0, r1 = int(cu[b]), int(cu[b + 1]), int(moff[b]), int(moff[b + 1])
        if r1 == r0:
            continue
        o_b, l_b = [], []
        for h in range(H):
            qq = q64[r0:r1, h * dh:(h + 1) * dh]
            kk = kv64[t0:t1, h * dh:(h + 1) * dh]
            vv = kv64[t0:t1, d + h * dh:d + (h + 1) * dh]
            s = qq @ kk.t() / np.sqrt(dh)
            if key_pad is not None:
                s = s + key_pad[t0:t1].double()[None, :] * -1e9
            l_b.append(torch.logsumexp(s, 1))
            o_b.append(torch.softmax(s, 1) @ vv)
        outs.append(torch.cat(o_b, 1))
        lses.append(torch.stack(l_b, 1))
    o = torch.cat(outs, 0)
    (o * go.double()).sum().backward()
    return o.detach(), torch.cat(lses, 0).detach(), q64.grad, kv64.grad


@pytest.mark.parametrize('dtype,H,dh,smax,mmax,pad', [
    (torch.float32, 2, 64, 50, 10, False), (torch.float32, 4, 32, 200, 20, True), (torch.float32, 2, 64, 300, 5, False),
    (torch.bfloat16, 2, 64, 200, 10, False), (torch.bfloat16, 4, 64, 512, 12, True), (torch.bfloat16, 2, 32, 70, 33, False),
    (torch.bfloat16, 1, 64, 3, 1, False), (torch.bfloat16, 2, 64, 33, 32, False), (torch.bfloat16, 2, 32, 64, 64, True),
    (torch.float32, 1, 32, 3, 1, False), (torch.bfloat16, 3, 64, 129, 7, False)])
def test_attn_mq_kernels_match_fp64(dtype, H, dh, smax, mmax, pad):
    from bert4clickpath_amd import ops
    B = 9
    cu, moff, q, kv, go = _ragged(B, smax, mmax, H, dh, 100 + smax + mmax, dtype)
    key_pad = None
    if pad:
        key_pad = (torch.rand(int(cu[-1]), generator=torch.Generator().manual_seed(1)) < 0.15).to(torch.uint8)
        key_pad[cu[:-1].long()] = 0                      # every sequence keeps a live key
    ro, rl, rdq, rdkv = _ref(cu, moff, q, kv, go, H, dh, key_pad)
    dev = 'cuda'
    kp = key_pad.to(dev) if key_pad is not None else None
    o, lse = ops.attn_mq_fwd(q.to(dev), kv.to(dev), cu.to(dev), moff.to(dev), B, smax, H, dh, kp)
    tol = 2e-5 if dtype == torch.float32 else 1.5e-2
    assert float((o.double().cpu() - ro).abs().max()) < tol * max(1.0, float(ro.abs().max()))
    assert float((lse.double().cpu() - rl).abs().max()) < (1e-4 if dtype == torch.float32 else 2e-2)
    # backward from the fp64 o / lse rounded to the kernel's dtype (what the forward hands over)
    dq, dkv = ops.attn_mq_bwd(q.to(dev), kv.to(dev), cu.to(dev), moff.to(dev), o, go.to(dev), lse, B, smax, H, dh, kp)
    btol = 1e-4 if dtype == torch.float32 else 3e-2
    assert float((dq.double().cpu() - rdq).abs().max()) < btol * max(1.0, float(rdq.abs().max()))
    assert float((dkv.double().cpu() - rdkv).abs().max()) < btol * max(1.0, float(rdkv.abs().max()))
    # sequences without a query row: exact zeros in dk | dv
    for b in range(B):
        if moff[b + 1] == moff[b]:
            assert float(dkv[int(cu[b]):int(cu[b + 1])].abs().max()) == 0.0
    # beside the whole-tensor bounds: every element of o, lse, dq and of dk and dv SEPARATELY against its own derived bound
    import local_bounds as lb
    d = H * dh
    res = lb.attn_mq(q, kv, cu, moff, go, H, dh, 'row_f32' if dtype == torch.float32 else 'mq_mfma', key_pad)
    for n, t in {'o': o, 'lse': lse, 'dq': dq, 'dk': dkv[:, :d], 'dv': dkv[:, d:]}.items():
        lb.check(n, t, *res[n])


def test_attn_mq_fwd_lds_need_grows_within_one_process():
    """One kernel, two launches whose dynamic LDS need grows across the 64 KiB that a launch gets without an opt-in: the fp32
    forward with dh = 64 needs 16 * 64 * 4 + 16 * SP * 4 + 128 * 64 * 4 bytes (mq_fwd_lds; SP = max_len rounded up to 64), that is
    40,960 at max_len = 64 and 69,632 at max_len = 512.  The opt-in (b4c_allow_lds) must be renewed for the second launch: a helper
    that remembers the kernel and not the size lets the runtime reject it, and the entry point returns an error.
    The fp32 backward cannot cross the line: its need (mq_bwd_lds) does not depend on max_len and is 49,280 bytes at dh = 64."""
    from bert4clickpath_amd import ops
    B, H, dh, dev = 2, 1, 64, 'cuda'
    for max_len in (64, 512):
        cu, moff, q, kv, go = _ragged(B, max_len, 3, H, dh, 7 + max_len, torch.float32, with_empty=False)
        ro, rl, _, _ = _ref(cu, moff, q, kv, go, H, dh)
        o, lse = ops.attn_mq_fwd(q.to(dev), kv.to(dev), cu.to(dev), moff.to(dev), B, max_len, H, dh, None)   # raises unless B4C_OK
        assert float((o.double().cpu() - ro).abs().max()) < 2e-5 * max(1.0, float(ro.abs().max())), max_len
        assert float((lse.double().cpu() - rl).abs().max()) < 1e-4, max_len


# ------------------------------------------------------------------------------------------------------------------
# the model: last encoder layer evaluated at the [MASK] rows only (ops.mq_last_layer) against the full layer and the oracle
# ------------------------------------------------------------------------------------------------------------------
from oracle import torch_ref as tr  # noqa: E402


def _model(V, d, L, H, head_dims, dtype, dropout=0.0, seed=3):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(seed)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': d},
                               SoftMaxHead(list(head_dims), V), value_to_head='[MASK]', num_encoder_layers=L,
                               num_attention_heads=H, dropout_rate=dropout, compute_dtype=dtype)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias') or n.endswith('beta'):
                p.normal_(0, 0.05)
    return m.cuda()


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


@pytest.mark.parametrize('L,H,d', [(2, 2, 64), (1, 2, 128), (3, 1, 64)])
def test_masked_query_last_layer_fp32_equals_full_layer_and_oracle(L, H, d):
    from bert4clickpath_amd import input_pipeline, ops
    V, S, B = 90, 40, 7
    model = _model(V, d, L, H, (32, 24), torch.float32)
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=5, min_len=3)
    ids = torch.from_numpy(b['ids'])
    feats = {'asin': ids[:, 2:S - 1].contiguous().cuda()}
    labels = torch.from_numpy(b['labels_padded']).cuda()
    res = {}
    for mq in (True, False):
        ops.mq_last_layer = mq
        try:
            for kw in ({}, {'max_masked_per_row': 10}):
                model.zero_grad()
                loss = model.cloze_loss(feats, labels, training=True, **kw)
                loss.backward()
                res[(mq, bool(kw))] = (float(loss), {n: p.grad.detach().clone() for n, p in model.named_parameters()})
            with torch.no_grad():
                res[(mq, 'topk')] = model.predict_topk(feats, 10, labels)
        finally:
            ops.mq_last_layer = True
    for syncfree in (False, True):
        (la, ga), (lb, gb) = res[(True, syncfree)], res[(False, syncfree)]
        assert abs(la - lb) < 2e-6 * abs(lb)
        for n in ga:
            assert _rel(ga[n], gb[n]) < 2e-4 or float(gb[n].abs().max()) < 1e-7, n
    ta, tb = res[(True, 'topk')], res[(False, 'topk')]
    assert torch.equal(ta[0], tb[0]) and torch.equal(ta[1], tb[1])
    # the fp64 oracle (full layers everywhere, rows gathered afterwards: the reference's dataflow)
    P = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items() if 'pos_encoding' not in k}
    tP = {k[len('transformer.'):]: v for k, v in P.items() if k.startswith('transformer.')}
    hP = {k[len('head.'):]: v for k, v in P.items() if k.startswith('head.')}
    enc = tr.transformer_forward({'items': ids}, tP, L, H)
    rows, _ = tr.gather_masked_rows(enc, ids)
    probs_ref = torch.softmax(tr.softmax_head_logits(rows, hP, 2), -1)
    ref = tr.sparse_ce_tf(probs_ref, torch.from_numpy(b['labels']).long()).mean()
    ref.backward()
    la, ga = res[(True, False)]
    assert abs(la - float(ref)) < 2e-5 * float(ref)
    for n in ga:
        if float(P[n].grad.abs().max()) > 1e-9:
            assert _rel(ga[n], P[n].grad) < 2e-3, n


def test_masked_query_last_layer_bf16_packed_and_dropout():
    from bert4clickpath_amd import input_pipeline, ops, optim
    V, S, B = 300, 48, 12
    model = _model(V, 128, 2, 2, (64, 128), torch.bfloat16)
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=21, min_len=3)
    ids = torch.from_numpy(b['ids'])
    feats = {'asin': ids[:, 2:S - 1].contiguous().cuda()}
    labels = torch.from_numpy(b['labels_padded']).cuda()
    n_real = int((b['ids'] != 0).sum())
    res = {}
    for mq in (True, False):
        ops.mq_last_layer = mq
        try:
            model.zero_grad()
            loss = model.cloze_loss(feats, labels, training=True, max_masked_per_row=10, n_real_tokens=n_real)
            loss.backward()
            res[mq] = (float(loss), {n: p.grad.detach().clone() for n, p in model.named_parameters()})
        finally:
            ops.mq_last_layer = True
    assert abs(res[True][0] - res[False][0]) < 3e-3 * abs(res[False][0])
    for n in res[True][1]:
        if float(res[False][1][n].float().norm()) < 1e-9 or n.endswith('mha.wk.bias'):
            continue
        assert _rel(res[True][1][n], res[False][1][n]) < 0.08, n
    # with dropout and the optimizer's arena (in-place gradients, grouped dW launches): the loss goes down
    m2 = _model(V, 128, 2, 2, (64, 128), torch.bfloat16, dropout=0.1)
    opt = optim.Adam(m2.parameters(), 1e-3, 0.9, 0.999, 1e-9)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = m2.cloze_loss(feats, labels, training=True, max_masked_per_row=10, n_real_tokens=n_real)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert np.isfinite(losses).all() and losses[-1] < 0.8 * losses[0]


def test_masked_query_last_layer_without_any_mask():
    """A batch without a single [MASK] (an empty replica of a data-parallel step): the loss is 0, every gradient is
    defined (zeros), nothing faults -- with the arena's in-place gradients and without."""
    from bert4clickpath_amd import optim
    V, S, B = 90, 24, 5
    for arena in (False, True):
        model = _model(V, 64, 2, 2, (32, 24), torch.bfloat16, dropout=0.1)
        opt = optim.Adam(model.parameters(), 1e-3, 0.9, 0.999, 1e-9) if arena else None
        g = torch.Generator().manual_seed(2)
        items = torch.randint(10, 10 + V, (B, S), generator=g).cuda()         # item ids only: no [MASK] (id 1) anywhere
        labels = torch.full((B, 10), -1.0).cuda()
        if opt:
            opt.zero_grad()
        loss = model.cloze_loss({'asin': items}, labels, training=True, max_masked_per_row=10, n_real_tokens=B * (S + 3))
        loss.backward()
        assert float(loss) == 0.0
        for n, p in model.named_parameters():
            if p.grad is not None:
                assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) == 0.0, n
        if opt:
            opt.step()
        # the form that reads the row count back: R = 0 rows reach the last layer and the head
        model.zero_grad()
        loss = model.cloze_loss({'asin': items}, labels, training=True)
        loss.backward()
        assert float(loss) == 0.0


def test_background_dw_sweep_gives_the_foreground_gradients():
    """ops.overlap_vocab_dw: the vocabulary head's dW sweep runs in pieces on a side stream beside the encoder backward
    (a piece per attention-backward launch, the count learned from the previous pass).  Same kernels' arithmetic: the
    gradients of three consecutive steps must match the foreground order (fp32 atomics order apart), with and without
    attention launches in the pass, and the pass count must be learned."""
    from bert4clickpath_amd import input_pipeline, ops, optim
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    V, B, S = 3000, 48, 40
    batch = input_pipeline.synthetic_cloze_batch(B, S, V, seed=11, min_len=6)
    items = torch.from_numpy(batch['ids'])[:, 2:S - 1].contiguous().cuda()
    labels = torch.from_numpy(batch['labels_padded']).cuda()
    n_real = int((batch['ids'] != 0).sum())
    grads = {}
    prev = (ops.overlap_vocab_dw, ops.background_workgroups)
    try:
        for layers in (3, 1):               # 1 layer + masked-query last layer: no resident attention backward at all
            for mode in (False, True):
                ops.overlap_vocab_dw, ops.background_workgroups = mode, 8
                torch.manual_seed(0)
                head = SoftMaxHead([64, 128], V)
                m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': 128}, head,
                                           value_to_head='[MASK]', num_encoder_layers=layers, num_attention_heads=2, dropout_rate=0.0,
                                           compute_dtype=torch.bfloat16).to('cuda')
                opt = optim.Adam(m.parameters())
                out = []
                for step in range(3):
                    opt.zero_grad()
                    loss = m.cloze_loss({'asin': items}, labels, training=True, max_masked_per_row=10, n_real_tokens=n_real)
                    loss.backward()
                    c = opt.arena.ctx             # the arena's host state: side-stream queue, plan of the next pass
                    ops.join_side_work(c)
                    torch.cuda.synchronize()
                    out.append({n: p.grad.detach().clone() for n, p in m.named_parameters()})
                    if mode:
                        assert not c.queue and not c.counting and not c.pending and not c.pending_dw and c.side_launched is None
                        assert c.kicks_expected == (layers - 1 if ops.mq_last_layer else layers)
                grads[(layers, mode)] = out
            for step in range(3):
                for n, g in grads[(layers, False)][step].items():
                    gb = grads[(layers, True)][step][n]
                    assert float((g - gb).abs().max()) <= 2e-5 * float(g.abs().max()) + 1e-9, (layers, step, n)
    finally:
        ops.overlap_vocab_dw, ops.background_workgroups = prev


def test_background_dw_sweep_on_a_user_stream():
    """the whole step issued under `with torch.cuda.stream(s)`: the end-of-backward join has to make THAT stream wait for the
    side stream (the callback may run on the autograd engine's thread, whose current stream is the default one)"""
    from bert4clickpath_amd import input_pipeline, ops, optim
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    V, B, S = 20000, 64, 40
    batch = input_pipeline.synthetic_cloze_batch(B, S, V, seed=21, min_len=6)
    items = torch.from_numpy(batch['ids'])[:, 2:S - 1].contiguous().cuda()
    labels = torch.from_numpy(batch['labels_padded']).cuda()
    n_real = int((batch['ids'] != 0).sum())
    prev = ops.overlap_vocab_dw
    try:
        out = {}
        for mode in (False, True):
            ops.overlap_vocab_dw = mode
            torch.manual_seed(0)
            m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': 128},
                                       SoftMaxHead([64, 128], V), value_to_head='[MASK]', num_encoder_layers=2,
                                       num_attention_heads=2, dropout_rate=0.0, compute_dtype=torch.bfloat16).to('cuda')
            opt = optim.Adam(m.parameters())
            torch.cuda.synchronize()
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for step in range(2):
                    opt.zero_grad()
                    loss = m.cloze_loss({'asin': items}, labels, training=True, max_masked_per_row=10, n_real_tokens=n_real)
                    loss.backward()
                    snap = m.head.output_layer.kernel.grad.detach().clone()       # on s, right behind backward: no explicit join
            torch.cuda.synchronize()
            out[mode] = snap
        assert float((out[True] - out[False]).abs().max()) <= 2e-5 * float(out[False].abs().max()) + 1e-12
    finally:
        ops.overlap_vocab_dw = prev
