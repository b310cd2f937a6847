"""Attention-probability dropout in the attention kernels (attention_dropout_rate; an extension with no reference oracle: the
checker is the float64 restatement tests/attn_dropout_ref.py with the keep masks regenerated on the host by the rule of
include/b4c.h).

1. exact mask recovery: with q = k = 0 and one-hot V / dO the outputs ARE the masks, no tolerance -- here for S <= dh only (the
   first two key tiles, the resident backward, the row kernels at one shape).  tests/test_gpu_attn_dropout_routes.py carries the
   construction to any length in passes and lists, per kernel body (the key-block backward with one block and with two
   included) and per skip path, the case that reaches it.
2. parity against float64 with the regenerated mask, bounds of tests/test_gpu_packed.py::test_varlen_attention_matches_fp64 for
   bf16 and of tests/test_gpu_kernels.py::test_attention_fwd_bwd for fp32.
3. the new entry points at rate 0 against today's, bit for bit.
4. a float32 Encoder against the float64 restatement, every mask regenerated.
5. the bf16 packed model: determinism, the route of the last layer, checkpoint / resume."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_dropout_ref as ref  # noqa: E402


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops
    return ops


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _layout(lens, packed):
    """-> (B, S_arg, cu device tensor or None, row offsets on the host)"""
    off = np.concatenate([[0], np.cumsum(lens)])
    cu = torch.tensor(off, dtype=torch.int32, device='cuda') if packed else None
    return len(lens), max(lens), cu, off


# ---- 1. exact mask recovery ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,lens,packed,H,dh', [
    (torch.bfloat16, [40, 40], False, 2, 64),          # two key tiles, the second partial; the resident backward
    (torch.bfloat16, [40, 7, 33, 1], True, 2, 64),     # q, k count from cu[b]; the pitch is max_len
    (torch.float32, [22, 22], False, 2, 32),           # the row kernels; S4 = 24
])
def test_outputs_are_the_masks(ops, dtype, lens, packed, H, dh):
    rate, seed = 0.25, 0xA11CE + len(lens)
    B, S_arg, cu, off = _layout(lens, packed)
    d, T = H * dh, int(off[-1])
    assert S_arg <= dh
    qkv = torch.zeros(T, 3 * d, dtype=dtype)
    do = torch.zeros(T, d, dtype=dtype)
    for b, L in enumerate(lens):
        for i in range(L):
            for h in range(H):
                qkv[off[b] + i, 2 * d + h * dh + i] = 1.0            # V row k = one-hot at column k
                do[off[b] + i, h * dh + i] = 1.0                      # dO row q = one-hot at column q
    qkv, do = qkv.cuda(), do.cuda()
    key_pad = torch.zeros(T, dtype=torch.uint8, device='cuda')
    keep = ref.keep_mask(ops, seed, B, H, S_arg, rate)
    o, lse = ops.attn_fwd(qkv, key_pad, B, S_arg, H, dh, cu, rate, seed)
    dqkv = ops.attn_bwd(qkv, key_pad, o, do, lse, B, S_arg, H, dh, cu, None, rate, seed)
    torch.cuda.synchronize()
    o, dqkv = o.float().cpu(), dqkv.float().cpu()
    for b, L in enumerate(lens):
        ob = o[off[b]:off[b] + L].view(L, H, dh).permute(1, 0, 2)                         # [h][q][c]
        want = torch.zeros(H, L, dh, dtype=torch.bool)
        want[:, :, :L] = keep[b, :, :L, :L]
        assert torch.equal(ob != 0, want), ('o', b)
        dv = dqkv[off[b]:off[b] + L, 2 * d:].reshape(L, H, dh).permute(1, 0, 2)           # [h][k][c]: P~[c][k]
        want = torch.zeros(H, L, dh, dtype=torch.bool)
        want[:, :, :L] = keep[b, :, :L, :L].transpose(-1, -2)
        assert torch.equal(dv != 0, want), ('dv', b)
        # lse is that of the undropped softmax: log(L) for uniform probabilities
        assert float((lse[b, :, :L].cpu() - float(np.log(L))).abs().max()) < 1e-4
    assert not dqkv[:, :2 * d].any()                                                      # dQ, dK: exactly zero
    assert 0.6 < float(keep.float().mean()) < 0.9


# ---- 2. parity against float64 ---------------------------------------------------------------------------------------------------
def _parity_case(ops, dtype, lens, packed, H, dh, n_pad, rate, seed):
    g = torch.Generator().manual_seed(sum(lens) + dh)
    B, S_arg, cu, off = _layout(lens, packed)
    d, T = H * dh, int(off[-1])
    qkv = (torch.randn(T, 3 * d, generator=g) * 0.8).to(dtype)
    do = torch.randn(T, d, generator=g).to(dtype)
    pad = torch.zeros(T, dtype=torch.uint8)
    if n_pad:
        for b, L in enumerate(lens):
            pad[off[b] + L - n_pad:off[b] + L] = 1
    return B, S_arg, cu, off, qkv, do, pad


def _reference(ops, lens, off, B, S_arg, H, dh, qkv, do, pad, rate, seed):
    keep = ref.keep_mask(ops, seed, B, H, S_arg, rate) if rate > 0 else None
    q64 = qkv.double().requires_grad_(True)
    outs, lses = [], []
    for b, L in enumerate(lens):
        rows = q64[off[b]:off[b] + L][None]
        kp = pad[off[b]:off[b] + L][None]
        o, l = ref.attention_qkv(rows, H, dh, kp, keep[b:b + 1, :, :L, :L] if keep is not None else None, rate)
        outs.append(o[0])
        lses.append(l[0])
    o_ref = torch.cat(outs)
    o_ref.backward(do.double())
    return o_ref.detach(), lses, q64.grad


PARITY = [
    (torch.bfloat16, [96, 96], False, 2, 32, 30),           # dense, 30 trailing pad keys: the last key tile is padded but for two keys
    (torch.bfloat16, [256, 256], False, 1, 64, 0),          # past the resident limit of 224: the key-block backward
    (torch.bfloat16, [300, 40, 257, 1], True, 2, 64, 0),    # QPW = 2 forward; two key blocks with the fp32 dQ partial
    (torch.float32, [22, 22], False, 2, 32, 0),             # the row kernels
]


@pytest.mark.parametrize('dtype,lens,packed,H,dh,n_pad', PARITY)
def test_matches_fp64_with_the_regenerated_mask(ops, dtype, lens, packed, H, dh, n_pad):
    """bounds: bf16 those of test_varlen_attention_matches_fp64 (o 1.2e-2, dqkv 2.5e-2 relative L2, lse 3e-2), fp32 those of
    test_attention_fwd_bwd (2e-5, 1e-4, 1e-4), unwidened"""
    rate, seed = 0.2, 0xD0D0 + sum(lens)
    B, S_arg, cu, off, qkv, do, pad = _parity_case(ops, dtype, lens, packed, H, dh, n_pad, rate, seed)
    o_ref, lses, g_ref = _reference(ops, lens, off, B, S_arg, H, dh, qkv, do, pad, rate, seed)
    qd, dod, padd = qkv.cuda(), do.cuda(), pad.cuda()
    o, lse = ops.attn_fwd(qd, padd, B, S_arg, H, dh, cu, rate, seed)
    dqkv = ops.attn_bwd(qd, padd, o, dod, lse, B, S_arg, H, dh, cu, None, rate, seed)
    again = ops.attn_bwd(qd, padd, o, dod, lse, B, S_arg, H, dh, cu, None, rate, seed)
    e_o, e_g = rel_err(o, o_ref), rel_err(dqkv, g_ref)
    e_l = max(float((lse[b, :, :L].double().cpu() - lses[b].detach()).abs().max()) for b, L in enumerate(lens))
    print('attention dropout %s lens=%s: rel_err(o) %.3e  rel_err(dqkv) %.3e  |dlse| %.3e' % (dtype, lens, e_o, e_g, e_l))
    tol_o, tol_l, tol_g = (2e-5, 1e-4, 1e-4) if dtype == torch.float32 else (1.2e-2, 3e-2, 2.5e-2)
    assert e_o < tol_o
    assert e_l < tol_l
    assert e_g < tol_g
    assert torch.equal(again, dqkv)
    # the dropped forward differs from the undropped one; lse does not
    o0, lse0 = ops.attn_fwd(qd, padd, B, S_arg, H, dh, cu)
    assert not torch.equal(o0, o)
    for b, L in enumerate(lens):
        assert torch.equal(lse0[b, :, :L], lse[b, :, :L])


# ---- 3. rate 0 is the old path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,lens,packed,H,dh,n_pad', [PARITY[0], PARITY[2]])
def test_rate_zero_entry_points_equal_the_old_ones(ops, dtype, lens, packed, H, dh, n_pad):
    from bert4clickpath_amd import _lib as L
    B, S, cu, off, qkv, do, pad = _parity_case(ops, dtype, lens, packed, H, dh, n_pad, 0.0, 0)
    qd, dod, padd = qkv.cuda(), do.cuda(), pad.cuda()
    d = H * dh
    p, st, dt = ops._p, ops._st(), ops.dt_code(qd.dtype)
    # the old side: raw calls of the entry points without dropout (ops itself goes through b4c_attn_*_ex)
    o0 = torch.empty(qd.shape[0], d, dtype=qd.dtype, device='cuda')
    lse0 = torch.full((B, H, S), float('nan'), dtype=torch.float32, device='cuda')
    dq0 = torch.empty_like(qd)
    o1, lse1, dq1 = torch.empty_like(o0), torch.full_like(lse0, float('nan')), torch.empty_like(dq0)
    delta = torch.empty_like(lse0)
    need = L.lib().b4c_attn_bwd_workspace_bytes(B, S, H, dh, dt)
    assert (need > 0) == (S > 256)
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device='cuda')
    if cu is None:
        L.check(L.lib().b4c_attn_fwd(p(qd), qd.stride(0), p(padd), p(o0), d, p(lse0), B, S, H, dh, dt, st))
        L.check(L.lib().b4c_attn_bwd_ws(p(qd), qd.stride(0), p(padd), p(o0), d, p(dod), d, p(lse0), p(delta), p(dq0), dq0.stride(0),
                                        B, S, H, dh, p(ws), need, dt, st))
    else:
        L.check(L.lib().b4c_attn_fwd_varlen(p(qd), qd.stride(0), p(padd), p(cu), p(o0), d, p(lse0), B, S, H, dh, dt, st))
        L.check(L.lib().b4c_attn_bwd_varlen(p(qd), qd.stride(0), p(padd), p(cu), p(o0), d, p(dod), d, p(lse0), p(delta), p(dq0),
                                            dq0.stride(0), B, S, H, dh, p(ws), need, dt, st))
    seed = 12345                                          # ignored at rate 0
    if cu is None:
        L.check(L.lib().b4c_attn_fwd_drop(p(qd), qd.stride(0), p(padd), p(o1), d, p(lse1), B, S, H, dh, dt, st, 0.0, seed))
        L.check(L.lib().b4c_attn_bwd_drop_ws(p(qd), qd.stride(0), p(padd), p(o1), d, p(dod), d, p(lse1), p(delta), p(dq1),
                                             dq1.stride(0), B, S, H, dh, p(ws), need, dt, st, 0.0, seed))
    else:
        L.check(L.lib().b4c_attn_fwd_varlen_drop(p(qd), qd.stride(0), p(padd), p(cu), p(o1), d, p(lse1), B, S, H, dh, dt, st, 0.0, seed))
        L.check(L.lib().b4c_attn_bwd_varlen_drop(p(qd), qd.stride(0), p(padd), p(cu), p(o1), d, p(dod), d, p(lse1), p(delta), p(dq1),
                                                 dq1.stride(0), B, S, H, dh, p(ws), need, dt, st, 0.0, seed))
    torch.cuda.synchronize()
    assert torch.equal(o1, o0) and torch.equal(dq1, dq0)
    for b, Lb in enumerate(lens):
        assert torch.equal(lse1[b, :, :Lb], lse0[b, :, :Lb])
    # a rate outside [0, 1) is an error, not a launch
    for bad in (1.0, -0.25, float('nan')):
        rc = L.lib().b4c_attn_fwd_drop(p(qd), qd.stride(0), p(padd), p(o1), d, p(lse1), B, S, H, dh, dt, st, bad, seed)
        assert rc != 0 and b'dropout rate' in L.lib().b4c_last_error()


# ---- 4. encoder level, float32 ---------------------------------------------------------------------------------------------------
def test_encoder_fp32_matches_fp64_with_every_mask_regenerated(ops):
    """bounds: the float32 bounds of tests/test_gpu_round2.py (output 1e-4 absolute, gradients 2e-4 of the largest entry), which
    are also those of the float32 model-with-dropout test (tests/test_gpu_model.py::test_gradients_match_oracle_fp32)"""
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    torch.manual_seed(5)
    B, S, d, H, NL, rate, a_rate = 3, 24, 64, 2, 2, 0.1, 0.2
    enc = T.Encoder(num_layers=NL, d_model=d, num_heads=H, dff=100, dropout_rate=rate, attention_dropout_rate=a_rate).cuda()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith('bias') or n.endswith('beta'):
                p.normal_(0, 0.05)
    x = torch.randn(B, S, d, device='cuda', requires_grad=True)
    wgt = torch.randn(B, S, d)
    pad = torch.zeros(B, S, dtype=torch.uint8)
    pad[0, 20:], pad[1, 9:], pad[2, 23:] = 1, 1, 1
    T.set_dropout_seed(2024)
    out = enc(x, training=True, mask=pad.cuda())
    (out * wgt.cuda()).sum().backward()
    # the masks, in the order the encoder drew its seeds: input dropout, then per layer residual 1, residual 2, attention
    stream = T._SeedStream(2024)
    n = B * S * d
    keep_in = torch.from_numpy(ops.keep_mask(stream.next(), n, rate)).view(B, S, d)
    keep_res, keep_attn = {}, []
    for i in range(NL):
        keep_res['l%d.1' % i] = torch.from_numpy(ops.keep_mask(stream.next(), n, rate)).view(B, S, d)
        keep_res['l%d.2' % i] = torch.from_numpy(ops.keep_mask(stream.next(), n, rate)).view(B, S, d)
        keep_attn.append(ref.keep_mask(ops, stream.next(), B, H, S, a_rate))
    assert T.dropout_seeds.counter == stream.counter == 1 + 3 * NL
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in enc.named_parameters()}
    xr = x.detach().cpu().double().requires_grad_(True)
    ro = ref.encoder_forward(ref.dropout(xr, rate, keep_in), pad, P, NL, H, rate, a_rate, keep_res, keep_attn)
    (ro * wgt.double()).sum().backward()
    err = float((out.detach().cpu().double() - ro.detach()).abs().max())
    print('encoder fp32 with attention dropout: max|dout| %.3e' % err)
    assert err < 1e-4
    worst = float((x.grad.cpu().double() - xr.grad).abs().max() / xr.grad.abs().max())
    assert worst < 2e-4, ('x', worst)
    for name, p in enc.named_parameters():
        gr = P[name].grad
        if float(gr.abs().max()) < 1e-9:          # d / d key-bias is identically zero (softmax shift invariance; the mask keeps it so)
            assert float(p.grad.abs().max()) < 1e-5, name
            continue
        e = float((p.grad.cpu().double() - gr).abs().max() / gr.abs().max())
        worst = max(worst, e)
        assert e < 2e-4, (name, e)
    print('encoder fp32 with attention dropout: worst relative gradient error %.3e' % worst)
    # evaluation draws nothing and drops nothing
    c = T.dropout_seeds.counter
    ev = enc(x.detach(), training=False, mask=pad.cuda())
    assert T.dropout_seeds.counter == c and torch.equal(ev, enc(x.detach(), training=False, mask=pad.cuda()))


# ---- 5. model level, bf16, packed ---------------------------------------------------------------------------------------------
V, D, S, B = 500, 128, 32, 8


def _model(a_rate, seed=3):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(seed)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': D}, SoftMaxHead([128, 64], V),
                               value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, dropout_rate=0.1,
                               compute_dtype=torch.bfloat16, attention_dropout_rate=a_rate)
    return m.cuda()


def _batch(seed=21):
    from bert4clickpath_amd import input_pipeline
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=seed, min_len=3)
    ids = torch.from_numpy(b['ids'])
    return {'asin': ids[:, 2:S - 1].contiguous().cuda()}, torch.from_numpy(b['labels_padded']).cuda(), int((b['ids'] != 0).sum())


class _CountMQ:
    """counts the passes that take the masked-query last layer, the way bf16_gates.GateRecorder notes them"""

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


def _step(model, feats, labels, n_real):
    model.zero_grad()
    loss = model.cloze_loss(feats, labels, training=True, max_masked_per_row=10, n_real_tokens=n_real)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def test_model_bf16_packed_step(ops, tmp_path):
    from bert4clickpath_amd import checkpoint, optim
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    feats, labels, n_real = _batch()
    model, model0 = _model(0.2), _model(0.0)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), model0.state_dict().values()))
    with _CountMQ(ops) as mq:
        T.set_dropout_seed(5)
        loss, grads = _step(model, feats, labels, n_real)
        assert model._packed is not None
        assert mq.calls == 0                               # training with attention dropout: the full last layer
        top, _, _ = model.predict_topk(feats, 10, labels)
        assert mq.calls == 1                               # evaluation (rate 0) keeps the masked-query route
    assert bool(torch.isfinite(loss))
    with _CountMQ(ops) as mq0:
        T.set_dropout_seed(5)
        loss0, _ = _step(model0, feats, labels, n_real)
        assert mq0.calls == 1                              # rate 0: the route every existing model takes
    assert float(loss) != float(loss0)
    T.set_dropout_seed(5)
    loss_b, grads_b = _step(model, feats, labels, n_real)
    assert torch.equal(loss, loss_b)
    for n in grads:
        assert torch.equal(grads[n], grads_b[n]), n

    # one optimizer step, checkpoint, step two; a fresh model and optimizer restored from the checkpoint repeat step two
    opt = optim.Adam(model.parameters())
    T.set_dropout_seed(31)
    _step(model, feats, labels, n_real)
    opt.step()
    path = checkpoint.save_checkpoint(os.path.join(str(tmp_path), 'ckpt-attn-drop'), model, opt, epoch=1)
    feats2, labels2, n_real2 = _batch(seed=22)
    loss2, grads2 = _step(model, feats2, labels2, n_real2)
    other = _model(0.2, seed=99)
    opt2 = optim.Adam(other.parameters())
    T.set_dropout_seed(1)
    checkpoint.load_checkpoint(path, other, opt2)
    loss2r, grads2r = _step(other, feats2, labels2, n_real2)
    assert torch.equal(loss2, loss2r)
    for n in grads2:
        assert torch.equal(grads2[n], grads2r[n]), n
