"""Causal (left-to-right) self-attention in the attention kernels, through ops (attn_fwd / attn_bwd / attn_weights with causal=True:
the CAUSAL = true instantiations of csrc/attn_mfma.hip, csrc/attn.hip and csrc/elemwise.hip behind b4c_attn_*_ex).  NO REFERENCE
ORACLE: an extension -- the checker is the float64 restatement tests/causal_ref.py (tests/test_causal_cpu.py checks it against
bidirectional attention over prefixes).

1. float64 parity of o, lse and dqkv on the shape grid of tests/test_gpu_kernels.py::test_attention_fwd_bwd, its pads and its
   bounds unwidened; more (sequence, head) items than workgroups; the packed layout.
2. exact properties, no tolerance: rows <= p do not depend on the rows behind them; rows >= p receive no gradient when dO is zero
   from p on; the weights above the diagonal are 0.
3. leading pads (queries whose visible keys are all padded): everything finite, the real rows within the bounds.
4. dropout x causal: the recovered masks are the host's keep bits AND visible AND NOT pad.
5. flags = 0 of the *_ex entry points: the bits of raw calls of the existing entry points; ops (which always calls *_ex) without
   options likewise; a _varlen entry point handed cu_seqlens = NULL stays an error.

Routes (the launch code of attn_mfma.hip): bf16 with head depth 32 / 64 and S <= 512 runs the matrix-core kernels -- forward QPW = 2
for S > 256; backward resident while its LDS image fits (S <= 224 at depth 64), else blocks of 256 keys with a workspace iff
S > 256 --, every other case the row kernels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_dropout_ref as ad  # noqa: E402
import causal_ref as cr  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
# bounds of tests/test_gpu_kernels.py::test_attention_fwd_bwd
TOL_O = {F32: 2e-5, BF16: 1.2e-2}           # relative L2
TOL_LSE = {F32: 1e-4, BF16: 3e-2}           # absolute
TOL_G = {F32: 1e-4, BF16: 2.5e-2}           # relative L2


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops
    return ops


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _pads(B, S):
    """those of test_attention_fwd_bwd: the tail of sequence 0, keys 5 .. S-2 of sequence 1; key 0 is real"""
    pad = torch.zeros(B, S, dtype=torch.uint8)
    pad[0, S - 4:] = 1
    if B > 1:
        pad[1, 5:S - 1] = 1
    return pad


def _lse_err(lse, lses, lens):
    return max(float((lse[b, :, :L].double().cpu() - lses[b]).abs().max()) for b, L in enumerate(lens))


# ---- 1. parity against float64 -------------------------------------------------------------------------------------------------
SHAPES = [(3, 13, 2, 32), (3, 32, 1, 64), (2, 33, 4, 32), (2, 129, 3, 64), (2, 200, 2, 64),
          (2, 224, 1, 64), (2, 230, 1, 64),          # the two sides of the resident-backward limit
          (2, 256, 2, 64), (3, 257, 2, 64), (2, 300, 2, 32), (2, 512, 4, 64),
          (2, 70, 1, 16), (1, 300, 2, 128)]          # bf16: the row-kernel fallback


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('B,S,H,dh', SHAPES)
def test_matches_float64(ops, dtype, B, S, H, dh):
    g = torch.Generator().manual_seed(S + dh)
    d = H * dh
    qd = (torch.randn(B * S, 3 * d, generator=g) * 0.8).to(dtype).cuda()
    dod = torch.randn(B * S, d, generator=g).to(dtype).cuda()
    pad = _pads(B, S)
    padd = pad.cuda()
    o, lse = ops.attn_fwd(qd, padd, B, S, H, dh, causal=True)
    dqkv = ops.attn_bwd(qd, padd, o, dod, lse, B, S, H, dh, causal=True)
    o_ref, lses, g_ref = cr.attention_grads(qd, dod, [S] * B, H, dh, pad.reshape(-1))
    e_o, e_l, e_g = rel_err(o, o_ref), _lse_err(lse, lses, [S] * B), rel_err(dqkv, g_ref)
    print('causal %s (%d,%d,%d,%d): rel_err(o) %.3e  |dlse| %.3e  rel_err(dqkv) %.3e' % (dtype, B, S, H, dh, e_o, e_l, e_g))
    assert e_o < TOL_O[dtype]
    assert e_l < TOL_LSE[dtype]
    assert e_g < TOL_G[dtype]
    # padded keys receive exactly zero dK / dV
    assert float(dqkv[:, d:].reshape(B, S, 2 * d)[0, S - 4:].abs().max()) == 0.0
    # the causal result is not the bidirectional one (row 0 sees one key instead of S)
    o_bi, _ = ops.attn_fwd(qd, padd, B, S, H, dh)
    assert not torch.equal(o_bi, o)
    if dtype == BF16 and S > 256 and dh in (32, 64):
        assert ops.L.lib().b4c_attn_bwd_workspace_bytes(B, S, H, dh, ops.L.BF16) == B * S * H * dh * 4     # the MFMA route ran
        again = ops.attn_bwd(qd, padd, o, dod, lse, B, S, H, dh, causal=True)
        assert torch.equal(again, dqkv)              # key blocks are summed in a fixed order


def test_more_items_than_workgroups(ops):
    """B * H = 700 items on the persistent backward grid, ragged padding, sequences without any gradient, as
    tests/test_gpu_kernels.py::test_attention_bwd_more_items_than_workgroups"""
    g = torch.Generator().manual_seed(11)
    B, S, H, dh = 350, 72, 2, 64
    d = H * dh
    assert B * H > torch.cuda.get_device_properties(0).multi_processor_count
    qkv = torch.randn(B * S, 3 * d, generator=g) * 0.7
    lens = torch.randint(5, S + 1, (B,), generator=g)
    pad = (torch.arange(S)[None, :] >= lens[:, None]).to(torch.uint8)
    do = torch.randn(B, S, d, generator=g)
    do[pad.bool()] = 0.0
    do[::7] = 0.0
    qd, dod, padd = qkv.to(BF16).cuda(), do.reshape(B * S, d).to(BF16).cuda(), pad.cuda()
    o, lse = ops.attn_fwd(qd, padd, B, S, H, dh, causal=True)
    dqkv = ops.attn_bwd(qd, padd, o, dod, lse, B, S, H, dh, causal=True)
    o_ref, lses, g_ref = cr.attention_grads(qd, dod, [S] * B, H, dh, pad.reshape(-1))
    e_o, e_l, e_g = rel_err(o, o_ref), _lse_err(lse, lses, [S] * B), rel_err(dqkv, g_ref)
    print('causal, 700 items: rel_err(o) %.3e  |dlse| %.3e  rel_err(dqkv) %.3e' % (e_o, e_l, e_g))
    assert e_o < TOL_O[BF16] and e_l < TOL_LSE[BF16] and e_g < TOL_G[BF16]
    assert float(dqkv.reshape(B, S, 3 * d)[::7].abs().max()) == 0.0
    again = ops.attn_bwd(qd, padd, o, dod, lse, B, S, H, dh, causal=True)     # item order differs from run to run, the result does not
    assert torch.equal(again, dqkv)


@pytest.mark.parametrize('lens,H,dh', [([1, 5, 32, 33, 64, 200, 257], 2, 64), ([7, 256, 40, 129, 31, 2], 2, 32)])
def test_packed_layout_matches_float64(ops, lens, H, dh):
    """q and k count from cu_seqlens[b]; per sequence against float64; sequences of 8 rows and more pad their last two keys"""
    g = torch.Generator().manual_seed(sum(lens) + dh)
    B, S_arg = len(lens), max(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    d, T = H * dh, int(off[-1])
    cu = torch.tensor(off, dtype=torch.int32, device='cuda')
    qd = (torch.randn(T, 3 * d, generator=g) * 0.8).to(BF16).cuda()
    dod = torch.randn(T, d, generator=g).to(BF16).cuda()
    pad = torch.zeros(T, dtype=torch.uint8)
    for b, L in enumerate(lens):
        if L >= 8:
            pad[off[b] + L - 2:off[b] + L] = 1
    padd = pad.cuda()
    need = ops.L.lib().b4c_attn_bwd_workspace_bytes(B, S_arg, H, dh, ops.L.BF16)
    assert (need > 0) == (S_arg > 256)
    o, lse = ops.attn_fwd(qd, padd, B, S_arg, H, dh, cu, causal=True)
    dqkv = ops.attn_bwd(qd, padd, o, dod, lse, B, S_arg, H, dh, cu, causal=True)
    again = ops.attn_bwd(qd, padd, o, dod, lse, B, S_arg, H, dh, cu, causal=True)
    o_ref, lses, g_ref = cr.attention_grads(qd, dod, lens, H, dh, pad)
    for b, L in enumerate(lens):
        rows = slice(int(off[b]), int(off[b]) + L)
        e_o, e_g = rel_err(o[rows], o_ref[rows]), rel_err(dqkv[rows], g_ref[rows])
        e_l = float((lse[b, :, :L].double().cpu() - lses[b]).abs().max())
        print('causal packed, sequence of %d: rel_err(o) %.3e  |dlse| %.3e  rel_err(dqkv) %.3e' % (L, e_o, e_l, e_g))
        assert e_o < TOL_O[BF16] and e_l < TOL_LSE[BF16] and e_g < TOL_G[BF16], (b, L)
    assert torch.equal(again, dqkv)


# ---- 2. exact properties ---------------------------------------------------------------------------------------------------------
EXACT = [(BF16, 70, 2, 64, 45), (BF16, 300, 2, 64, 31), (BF16, 300, 2, 64, 32), (BF16, 300, 2, 64, 45), (BF16, 300, 2, 64, 290),
         (BF16, 300, 1, 32, 290), (F32, 70, 2, 32, 31), (F32, 300, 1, 32, 290), (BF16, 70, 1, 16, 32)]


@pytest.mark.parametrize('dtype,S,H,dh,p', EXACT)
def test_rows_do_not_depend_on_the_rows_behind_them(ops, dtype, S, H, dh, p):
    """(a) the q / k / v rows of the positions > p replaced by other finite values of magnitude up to 1e4: o and lse of the rows
    <= p keep every bit.  p inside a tile, on a tile edge (31, 32), past 256."""
    g = torch.Generator().manual_seed(S + p)
    B, d = 2, H * dh
    qkv = torch.randn(B, S, 3 * d, generator=g) * 0.8
    other = qkv.clone()
    other[:, p + 1:] = (torch.rand(B, S - p - 1, 3 * d, generator=g) * 2 - 1) * 1e4
    pad = _pads(B, S).cuda()
    out = []
    for t in (qkv, other):
        o, lse = ops.attn_fwd(t.reshape(B * S, 3 * d).to(dtype).cuda(), pad, B, S, H, dh, causal=True)
        out.append((o.view(B, S, d)[:, :p + 1].clone(), lse[:, :, :p + 1].clone(), o.view(B, S, d)[:, p + 1:].clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert bool(torch.isfinite(out[1][0]).all()) and bool(torch.isfinite(out[1][1]).all())
    assert not torch.equal(out[0][2], out[1][2])                               # (the rows behind p did change)
    # the bidirectional launch sees them
    ob = [ops.attn_fwd(t.reshape(B * S, 3 * d).to(dtype).cuda(), pad, B, S, H, dh)[0].view(B, S, d)[:, :p + 1] for t in (qkv, other)]
    assert not torch.equal(ob[0], ob[1])


ZERO_DO = [(BF16, 200, 2, 64, 45), (BF16, 200, 2, 64, 64), (BF16, 256, 1, 64, 32), (BF16, 300, 2, 64, 290), (BF16, 300, 2, 64, 31),
           (BF16, 300, 1, 32, 257), (F32, 70, 2, 32, 31), (F32, 300, 1, 32, 290), (BF16, 70, 1, 16, 33)]


@pytest.mark.parametrize('dtype,S,H,dh,p', ZERO_DO)
def test_rows_without_gradient_behind_p_receive_none(ops, dtype, S, H, dh, p):
    """(b) dO zero on the rows >= p: dQ, dK and dV of the rows >= p are exactly 0 (a key behind every query that carries a
    gradient has no weight in any of them)"""
    g = torch.Generator().manual_seed(3 * S + p)
    B, d = 2, H * dh
    qd = (torch.randn(B * S, 3 * d, generator=g) * 0.8).to(dtype).cuda()
    do = torch.randn(B, S, d, generator=g)
    do[:, p:] = 0.0
    dod = do.reshape(B * S, d).to(dtype).cuda()
    pad = _pads(B, S).cuda()
    o, lse = ops.attn_fwd(qd, pad, B, S, H, dh, causal=True)
    dqkv = ops.attn_bwd(qd, pad, o, dod, lse, B, S, H, dh, causal=True).view(B, S, 3 * d)
    assert float(dqkv[:, p:].abs().max()) == 0.0
    assert float(dqkv[:, :p].abs().max()) > 0 and bool(torch.isfinite(dqkv).all())
    # bidirectional: the keys behind p do receive dK / dV from the queries before p
    o2, lse2 = ops.attn_fwd(qd, pad, B, S, H, dh)
    d2 = ops.attn_bwd(qd, pad, o2, dod, lse2, B, S, H, dh).view(B, S, 3 * d)
    assert float(d2[:, p:, d:].abs().max()) > 0


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('B,S,H,dh', [(2, 33, 2, 32), (2, 130, 1, 64), (2, 200, 2, 16)])
def test_weights_are_zero_above_the_diagonal(ops, dtype, B, S, H, dh):
    """(c) attn_weights(causal=True): exactly 0 above the diagonal, rows sum to 1 within 1e-5, equal to the restatement's
    exp(score - lse) within the bound of lse (d w = w d lse <= d lse)"""
    g = torch.Generator().manual_seed(S)
    d = H * dh
    qd = (torch.randn(B * S, 3 * d, generator=g) * 0.8).to(dtype).cuda()
    pad = _pads(B, S)
    o, lse = ops.attn_fwd(qd, pad.cuda(), B, S, H, dh, causal=True)
    w = ops.attn_weights(qd, pad.cuda(), lse, B, S, H, dh, causal=True).cpu()
    above = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1)
    assert float(w[..., above].abs().max()) == 0.0
    e_sum = float((w.double().sum(-1) - 1).abs().max())
    e_w = float((w.double() - cr.weights(qd.double().cpu().view(B, S, -1), H, dh, pad)).abs().max())
    print('causal weights %s (%d,%d,%d,%d): |rowsum - 1| %.3e  |dw| %.3e' % (dtype, B, S, H, dh, e_sum, e_w))
    assert e_sum < 1e-5
    assert e_w < TOL_LSE[dtype]
    # the bidirectional weights (from a bidirectional lse) are not zero there
    o2, lse2 = ops.attn_fwd(qd, pad.cuda(), B, S, H, dh)
    assert float(ops.attn_weights(qd, pad.cuda(), lse2, B, S, H, dh).cpu()[..., above].abs().max()) > 0


def test_weights_through_the_public_functions(ops):
    """scaled_dot_product_attention(causal=True) and MultiHeadAttention(causal=True): the weights are zero above the diagonal, the
    output is the restatement's; a look-ahead mask handed in as `mask` is refused with a pointer to causal=True"""
    from bert4clickpath_amd._lib import B4CError
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    g = torch.Generator().manual_seed(2)
    B, H, S, dh = 2, 2, 37, 32
    q, k, v = [torch.randn(B, H, S, dh, generator=g) for _ in range(3)]
    pad = _pads(B, S)
    mask = T.create_padding_mask((pad == 0).long()).cuda()          # (B, 1, 1, S), 1 = pad: ids 0 at the pads, 1 elsewhere
    out, w = T.scaled_dot_product_attention(q.cuda(), k.cuda(), v.cuda(), mask, return_weights=True, causal=True)
    want, _ = ad.attention(q.double(), k.double(), v.double(), cr.causal_neg(S, pad), None, 0.0)
    above = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1)
    assert float(w.cpu()[..., above].abs().max()) == 0.0
    assert rel_err(out, want) < TOL_O[F32]
    with pytest.raises(B4CError, match='causal=True'):
        T.scaled_dot_product_attention(q.cuda(), k.cuda(), v.cuda(), T.create_look_ahead_mask(S).cuda())
    torch.manual_seed(3)
    mha = T.MultiHeadAttention(64, 2).cuda()
    x = torch.randn(B, S, 64, generator=g).cuda().requires_grad_(True)
    y, w = mha(x, x, x, pad.cuda(), return_weights=True, causal=True)
    assert float(w.detach().cpu()[..., above].abs().max()) == 0.0
    y[:, :10].sum().backward()                      # a loss on the first 10 positions: nothing behind them takes part
    assert float(x.grad[:, 10:].abs().max()) == 0.0 and float(x.grad[:, :10].abs().max()) > 0
    yb, _ = mha(x, x, x, pad.cuda())
    assert not torch.equal(yb, y)


# ---- 3. leading pads -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,S,H,dh', [(BF16, 100, 2, 64), (BF16, 300, 2, 64), (BF16, 300, 1, 32), (F32, 100, 2, 32), (BF16, 100, 1, 16)])
def test_leading_pads(ops, dtype, S, H, dh):
    """sequence 0 pads its positions 0 .. 6, sequence 1 its positions 0 .. 39 (a whole key tile), sequence 2 none; dO is zero on the
    pad rows.  Every output and gradient is finite; o and lse of the real queries and the gradient of EVERY row (the pad rows' is
    zero on both sides) meet the parity bounds.  The 7 + 40 pad queries per head -- their visible keys are all padded, their
    value is not pinned -- are the only rows left out of the o / lse comparison."""
    g = torch.Generator().manual_seed(S + dh)
    B, d = 3, H * dh
    pad = torch.zeros(B, S, dtype=torch.uint8)
    pad[0, :7] = 1
    pad[1, :40] = 1
    real = (pad == 0)
    assert int((~real).sum()) == 47
    qd = (torch.randn(B * S, 3 * d, generator=g) * 0.8).to(dtype).cuda()
    do = torch.randn(B, S, d, generator=g)
    do[~real] = 0.0
    dod = do.reshape(B * S, d).to(dtype).cuda()
    o, lse = ops.attn_fwd(qd, pad.cuda(), B, S, H, dh, causal=True)
    dqkv = ops.attn_bwd(qd, pad.cuda(), o, dod, lse, B, S, H, dh, causal=True)
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(dqkv).all())
    o_ref, lses, g_ref = cr.attention_grads(qd, dod, [S] * B, H, dh, pad.reshape(-1))
    rows = real.reshape(-1)
    e_o, e_g = rel_err(o.cpu()[rows], o_ref[rows]), rel_err(dqkv, g_ref)
    lse_ref = torch.stack(lses)                                       # [B, H, S]
    sel = real[:, None, :].expand(B, H, S)
    assert int((~sel).sum()) == 47 * H
    e_l = float((lse.double().cpu() - lse_ref)[sel].abs().max())
    print('causal, leading pads %s S=%d dh=%d: rel_err(o) %.3e  |dlse| %.3e  rel_err(dqkv) %.3e' % (dtype, S, dh, e_o, e_l, e_g))
    assert e_o < TOL_O[dtype] and e_l < TOL_LSE[dtype] and e_g < TOL_G[dtype]
    assert float(dqkv.view(B, S, 3 * d)[~real].abs().max()) == 0.0


# ---- 4. dropout x causal ------------------------------------------------------------------------------------------------------
def _recover(ops, dtype, lens, packed, H, dh, seed, rate=0.25):
    """the passes of tests/test_gpu_attn_dropout_routes.py with causal=True -> (fwd, bwd: bool [H, L, L] per sequence,
    [h][query][key]; want: keep AND visible AND NOT pad from the host mask)"""
    B, S_arg = len(lens), max(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    d, T = H * dh, int(off[-1])
    cu = torch.tensor(off, dtype=torch.int32, device='cuda') if packed else None
    pad = torch.zeros(T, dtype=torch.uint8) if packed else ad.recovery_pads(B, S_arg).reshape(-1)
    padd = pad.cuda()
    keep = ops.attn_keep_mask(seed, B, H, S_arg, rate)
    fwd = [torch.zeros(H, L, L, dtype=torch.bool) for L in lens]
    bwd = [torch.zeros(H, L, L, dtype=torch.bool) for L in lens]
    for p in range(ad.recovery_passes(S_arg, dh)):
        qkv, do = ad.recovery_operands(lens, H, dh, p, dtype)
        qkv, do = qkv.cuda(), do.cuda()
        o, lse = ops.attn_fwd(qkv, padd, B, S_arg, H, dh, cu, rate, seed, causal=True)
        dqkv = ops.attn_bwd(qkv, padd, o, do, lse, B, S_arg, H, dh, cu, None, rate, seed, causal=True)
        torch.cuda.synchronize()
        assert not dqkv[:, :2 * d].any(), ('dQ, dK', p)                       # exactly zero: k = 0, and q = 0
        lse = lse.cpu()
        for b, L in enumerate(lens):          # the undropped softmax over the visible real keys: uniform
            n_vis = torch.cumsum((pad[off[b]:off[b] + L] == 0).double(), 0)
            assert float((lse[b, :, :L] - n_vis.log()[None, :]).abs().max()) < 1e-4, ('lse', b, p)
        ad.recovery_collect(fwd, bwd, o.float().cpu(), dqkv[:, 2 * d:].float().cpu(), lens, H, dh, p)
    want = [keep[b, :, :L, :L] & (pad[off[b]:off[b] + L] == 0)[None, None, :] & torch.tril(torch.ones(L, L, dtype=torch.bool))[None]
            for b, L in enumerate(lens)]
    return fwd, bwd, want


@pytest.mark.parametrize('dtype,lens,packed,H,dh', [
    (BF16, [33, 33], False, 2, 64), (BF16, [200, 200], False, 2, 64), (BF16, [300, 300], False, 1, 64),      # dense MFMA
    (F32, [33, 33], False, 2, 32), (F32, [200, 200], False, 1, 32), (F32, [300, 300], False, 1, 32),         # dense row
    (BF16, [33, 1, 20], True, 2, 64), (BF16, [200, 33, 7], True, 2, 32), (BF16, [300, 40, 257, 1], True, 1, 64),      # packed
], ids=lambda v: str(v).replace('torch.', '') if not isinstance(v, list) else 'x'.join(map(str, v)))
def test_dropout_masks_under_the_causal_mask(ops, dtype, lens, packed, H, dh):
    """the recovered keep bit of every visible unpadded (q, k) is ops.attn_keep_mask's -- the bit the bidirectional launch draws --
    and everything above the diagonal is 0, in o (forward) and in dV (backward)"""
    fwd, bwd, want = _recover(ops, dtype, lens, packed, H, dh, 0xCA05A1 + sum(lens) + dh)
    for b, w in enumerate(want):
        above = torch.triu(torch.ones(w.shape[-1], w.shape[-1], dtype=torch.bool), diagonal=1)
        for name, got in (('o', fwd), ('dV', bwd)):
            assert not got[b][:, above].any(), (name, b, 'above the diagonal')
            if not torch.equal(got[b], w):
                bad = (got[b] != w).nonzero()
                raise AssertionError('%s of sequence %d differs from mask AND visible AND NOT pad at %d (head, query, key) triples, '
                                     'the first %s' % (name, b, bad.shape[0], bad[:6].tolist()))
    kept = float(torch.cat([w[:, torch.tril(torch.ones(w.shape[-1], w.shape[-1], dtype=torch.bool))].reshape(-1) for w in want]).float().mean())
    if max(lens) >= 200 and packed:          # no pads: 0.75 of the visible pairs, within a tenth
        assert 0.9 * 0.75 < kept < 1.1 * 0.75


# ---- 5. flags = 0 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lens,packed,rate', [([96, 96], False, 0.0), ([96, 96], False, 0.2), ([300, 40, 257, 1], True, 0.0),
                                              ([300, 40, 257, 1], True, 0.2)])
def test_flags_zero_is_the_existing_entry_point(ops, lens, packed, rate):
    from bert4clickpath_amd import _lib as L
    g = torch.Generator().manual_seed(sum(lens))
    H, dh, seed = 2, 64, 777
    B, S = len(lens), max(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    d, T = H * dh, int(off[-1])
    cu = torch.tensor(off, dtype=torch.int32, device='cuda') if packed else None
    qd = (torch.randn(T, 3 * d, generator=g) * 0.8).to(BF16).cuda()
    dod = torch.randn(T, d, generator=g).to(BF16).cuda()
    padd = torch.zeros(T, dtype=torch.uint8, device='cuda')
    if not packed:
        padd = _pads(B, S).reshape(-1).cuda()
    p, st, dt = ops._p, ops._st(), ops.dt_code(qd.dtype)
    o0 = torch.empty(T, d, dtype=BF16, device='cuda')
    lse0 = torch.full((B, H, S), float('nan'), dtype=torch.float32, device='cuda')
    dq0 = torch.empty_like(qd)
    o1, lse1, dq1 = torch.empty_like(o0), torch.full_like(lse0, float('nan')), torch.empty_like(dq0)
    delta = torch.empty_like(lse0)
    need = L.lib().b4c_attn_bwd_workspace_bytes(B, S, H, dh, dt)
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device='cuda')
    # the left side: raw calls of the existing entry point that the (layout, rate) case names -- b4c_attn_fwd[_varlen][_drop],
    # b4c_attn_bwd_ws / _drop_ws / _varlen[_drop] (ops itself goes through b4c_attn_*_ex)
    layout = (p(cu),) if packed else ()
    drop = (rate, seed) if rate > 0 else ()
    fwd_name = 'b4c_attn_fwd' + ('_varlen' if packed else '') + ('_drop' if drop else '')
    bwd_name = 'b4c_attn_bwd' + ('_varlen' if packed else '') + ('_drop' if drop else '') + ('' if packed else '_ws')
    L.check(getattr(L.lib(), fwd_name)(p(qd), qd.stride(0), p(padd), *layout, p(o0), d, p(lse0), B, S, H, dh, dt, st, *drop), fwd_name)
    L.check(getattr(L.lib(), bwd_name)(p(qd), qd.stride(0), p(padd), *layout, p(o0), d, p(dod), d, p(lse0), p(delta), p(dq0),
                                       dq0.stride(0), B, S, H, dh, p(ws), need, dt, st, *drop), bwd_name)
    if S <= 256 and not packed and not drop:      # the form without a workspace
        dq2 = torch.empty_like(dq0)
        L.check(L.lib().b4c_attn_bwd(p(qd), qd.stride(0), p(padd), p(o0), d, p(dod), d, p(lse0), p(delta), p(dq2), dq2.stride(0),
                                     B, S, H, dh, dt, st), 'b4c_attn_bwd')
        assert torch.equal(dq2, dq0)
    L.check(L.lib().b4c_attn_fwd_ex(p(qd), qd.stride(0), p(padd), p(cu), p(o1), d, p(lse1), B, S, H, dh, dt, st, rate, seed, 0))
    L.check(L.lib().b4c_attn_bwd_ex(p(qd), qd.stride(0), p(padd), p(cu), p(o1), d, p(dod), d, p(lse1), p(delta), p(dq1), dq1.stride(0),
                                    B, S, H, dh, p(ws), need, dt, st, rate, seed, 0))
    torch.cuda.synchronize()
    assert torch.equal(o1, o0) and torch.equal(dq1, dq0)
    for b, Lb in enumerate(lens):
        assert torch.equal(lse1[b, :, :Lb], lse0[b, :, :Lb])
    if not packed and rate == 0.0:
        w0 = torch.empty(B, H, S, S, dtype=torch.float32, device='cuda')
        w1 = torch.empty_like(w0)
        L.check(L.lib().b4c_attn_weights(p(qd), qd.stride(0), p(padd), p(lse0), p(w0), B, S, H, dh, dt, st))
        L.check(L.lib().b4c_attn_weights_ex(p(qd), qd.stride(0), p(padd), p(lse0), p(w1), B, S, H, dh, dt, st, 0))
        assert torch.equal(w1, w0)
        # the packed layout keeps its limits under the new name: fp32 is refused
        q32 = qd.float()
        cu2 = torch.tensor([0, 96, 192], dtype=torch.int32, device='cuda')
        rc = L.lib().b4c_attn_fwd_ex(p(q32), q32.stride(0), p(padd), p(cu2), p(o1), d, p(lse1), B, S, H, dh, L.F32, st, 0.0, 0, 1)
        assert rc != 0 and b'bf16 only' in L.lib().b4c_last_error()


@pytest.mark.parametrize('packed', [False, True], ids=['dense', 'packed'])
def test_ops_without_options_is_the_existing_entry_point(ops, packed):
    """ops.attn_fwd / attn_bwd / attn_weights make one call per direction, b4c_attn_*_ex; without dropout and causal masking their
    results are, bit for bit, those of raw calls of b4c_attn_fwd / b4c_attn_bwd_ws / b4c_attn_weights (dense) and
    b4c_attn_fwd_varlen / b4c_attn_bwd_varlen (packed)"""
    from bert4clickpath_amd import _lib as L
    lens = [5, 32, 33] if packed else [33, 33, 33]
    g = torch.Generator().manual_seed(sum(lens) + 1)
    H, dh = 2, 64
    B, S = len(lens), max(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    d, T = H * dh, int(off[-1])
    cu = torch.tensor(off, dtype=torch.int32, device='cuda') if packed else None
    qd = (torch.randn(T, 3 * d, generator=g) * 0.8).to(BF16).cuda()
    dod = torch.randn(T, d, generator=g).to(BF16).cuda()
    padd = torch.zeros(T, dtype=torch.uint8, device='cuda') if packed else _pads(B, S).reshape(-1).cuda()
    p, st, dt = ops._p, ops._st(), ops.dt_code(qd.dtype)
    o0 = torch.empty(T, d, dtype=BF16, device='cuda')
    lse0 = torch.full((B, H, S), float('nan'), dtype=torch.float32, device='cuda')
    dq0, delta = torch.empty_like(qd), torch.empty_like(lse0)
    lib = L.lib()
    assert lib.b4c_attn_bwd_workspace_bytes(B, S, H, dh, dt) == 0
    if packed:
        L.check(lib.b4c_attn_fwd_varlen(p(qd), qd.stride(0), p(padd), p(cu), p(o0), d, p(lse0), B, S, H, dh, dt, st))
        L.check(lib.b4c_attn_bwd_varlen(p(qd), qd.stride(0), p(padd), p(cu), p(o0), d, p(dod), d, p(lse0), p(delta), p(dq0),
                                        dq0.stride(0), B, S, H, dh, None, 0, dt, st))
    else:
        L.check(lib.b4c_attn_fwd(p(qd), qd.stride(0), p(padd), p(o0), d, p(lse0), B, S, H, dh, dt, st))
        L.check(lib.b4c_attn_bwd_ws(p(qd), qd.stride(0), p(padd), p(o0), d, p(dod), d, p(lse0), p(delta), p(dq0), dq0.stride(0),
                                    B, S, H, dh, None, 0, dt, st))
    o1, lse1 = ops.attn_fwd(qd, padd, B, S, H, dh, cu)
    dq1 = ops.attn_bwd(qd, padd, o1, dod, lse1, B, S, H, dh, cu)
    torch.cuda.synchronize()
    assert torch.equal(o1, o0) and torch.equal(dq1, dq0)
    for b, Lb in enumerate(lens):
        assert torch.equal(lse1[b, :, :Lb], lse0[b, :, :Lb])
    if not packed:
        w0 = torch.empty(B, H, S, S, dtype=torch.float32, device='cuda')
        L.check(lib.b4c_attn_weights(p(qd), qd.stride(0), p(padd), p(lse0), p(w0), B, S, H, dh, dt, st))
        assert torch.equal(ops.attn_weights(qd, padd, lse0, B, S, H, dh), w0)


def test_varlen_entry_points_refuse_a_null_cu_seqlens(ops):
    """b4c_attn_fwd_varlen / b4c_attn_bwd_varlen share their host path with the dense entry points, where cu_seqlens = NULL means the
    dense layout: called with NULL they still are B4C_EINVAL 'null pointer' and launch nothing.  B = 1, S = 32: the buffers hold
    the 32 token rows a dense launch would work on, so a wrongly accepted call stays inside them and shows as changed outputs."""
    from bert4clickpath_amd import _lib as L
    B, S, H, dh = 1, 32, 2, 32
    d = H * dh
    g = torch.Generator().manual_seed(32)
    qd = (torch.randn(B * S, 3 * d, generator=g) * 0.8).to(BF16).cuda()
    dod = torch.randn(B * S, d, generator=g).to(BF16).cuda()
    padd = torch.zeros(B * S, dtype=torch.uint8, device='cuda')
    o = torch.full((B * S, d), 7.0, dtype=BF16, device='cuda')
    lse = torch.full((B, H, S), 7.0, dtype=torch.float32, device='cuda')
    delta, dqkv = torch.full_like(lse, 7.0), torch.full_like(qd, 7.0)
    ws = torch.full((64,), 7, dtype=torch.uint8, device='cuda')
    p, st, dt, lib = ops._p, ops._st(), ops.dt_code(BF16), L.lib()
    rc = lib.b4c_attn_fwd_varlen(p(qd), qd.stride(0), p(padd), None, p(o), d, p(lse), B, S, H, dh, dt, st)
    assert rc == L._C['B4C_EINVAL'] and b'null pointer' in lib.b4c_last_error()
    rc = lib.b4c_attn_bwd_varlen(p(qd), qd.stride(0), p(padd), None, p(o), d, p(dod), d, p(lse), p(delta), p(dqkv), dqkv.stride(0),
                                 B, S, H, dh, p(ws), ws.numel(), dt, st)
    assert rc == L._C['B4C_EINVAL'] and b'null pointer' in lib.b4c_last_error()
    torch.cuda.synchronize()
    for t in (o, lse, delta, dqkv, ws):
        assert bool((t == 7).all())
