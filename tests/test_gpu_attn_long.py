"""The streamed bf16 attention kernels of include/b4c.h (csrc/attn_long.hip: the forward with 256 queries per workgroup and
the keys in double-buffered blocks of 128; the backward as attn_bwd_mfma_kernel's walk over up to 8 key blocks of 256, whose middle
mode -- dq_acc += partial -- runs here for the first time), called through ops.attn_long_fwd / ops.attn_long_bwd.

Every element of o, lse, dq, dk and dv is held to the bound tests/local_bounds.py derives for it, route 'mfma' (the streamed kernels
round where the resident ones round: P once in front of P V, o once, dS once, dQ once after the fp32 sum over all key blocks, dK / dV
once).  Shapes: three key blocks with a one-row last query block and a one-key last key block (513), exact multiples (768), five
blocks (1057), the cap (2048), short S through the same kernels (31, 300); packed lists with sequences that end before a key block,
a length-1 sequence and lengths on block boundaries.

Causal: tests/causal_ref.py in float64 with the tolerance rule of tests/test_gpu_causal_attn.py (relative L2 1.2e-2 on o, 2.5e-2 on
dqkv, 3e-2 absolute on lse); rows do not depend on the rows behind them, bit for bit.  Dropout: the masks recovered exactly
(tests/attn_dropout_ref.py), forward and backward; float64 parity with the regenerated mask at the bounds of
tests/test_gpu_attn_dropout_routes.py.

Worst |error| / bound on the MI355X (RATIO lines of this file; "loose" as in tests/test_gpu_attn_local.py):

  route                                           o               lse             dq              dk              dv
  dense, 14 cases (worst: the 'short' pattern)    0.746           0.023 (loose)   0.287           0.132           0.461
  packed, 2 lists                                 0.400           0.020 (loose)   0.150           0.124           0.421
  a sequence with every key padded                0.191           0.015 (loose)   0.043           0.041           0.171
  S = 512 dense, streamed = resident to 3 digits  0.212           0.014 (loose)   0.058           0.049           0.186
  S = 512 packed, streamed = resident to 3 digits 0.369           0.017 (loose)   0.100           0.095           0.388
Causal and dropout parity (relative L2, every case and sequence): o 1.9e-3 .. 2.4e-3, dqkv 2.3e-3 .. 2.5e-3, |d lse| <= 1.5e-6.
"""
import functools

import numpy as np
import pytest
import torch

import attn_dropout_ref as ad
import causal_ref as cr
import local_bounds as lb

pytestmark = pytest.mark.gpu

NAMES = ('o', 'lse', 'dq', 'dk', 'dv')
BF16 = torch.bfloat16
# the tolerance rule of tests/test_gpu_causal_attn.py / tests/test_gpu_attn_dropout_routes.py for bf16
TOL_O, TOL_LSE, TOL_G = 1.2e-2, 3e-2, 2.5e-2


@pytest.fixture(scope='module')
def ops():
    from bert4clickpath_amd import ops as _ops
    return _ops


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _report(route, tag, ratios):
    print('RATIO attn long %s %s %s' % (route, tag, ' '.join('%s=%.3f' % (n, ratios[n]) for n in NAMES if n in ratios)))


def _long(ops, qd, padd, dod, B, S, H, dh, cu=None, rate=0.0, seed=0, causal=False):
    o, lse = ops.attn_long_fwd(qd, padd, B, S, H, dh, cu=cu, rate=rate, seed=seed, causal=causal)
    dqkv = ops.attn_long_bwd(qd, padd, o, dod, lse, B, S, H, dh, cu=cu, rate=rate, seed=seed, causal=causal)   # the kernel's own o, lse
    return o, lse, dqkv


def _split(o, lse, dqkv, d):
    return {'o': o, 'lse': lse, 'dq': dqkv[:, :d], 'dk': dqkv[:, d:2 * d], 'dv': dqkv[:, 2 * d:]}


# ---- dense ------------------------------------------------------------------------------------------------------------------------
DENSE = [(2, 513, 2, 64), (2, 768, 1, 32), (2, 769, 4, 32), (2, 1057, 2, 64), (1, 2048, 1, 32), (3, 31, 2, 32), (2, 300, 2, 64)]


@functools.lru_cache(maxsize=None)
def _dense_ref(B, S, H, dh, pattern):
    qkv, pad, do = lb.dense_inputs(BF16, B, S, H, dh, pattern)
    return qkv, pad, do, lb.attn_dense(qkv, pad, do, B, S, H, dh, 'mfma')


@pytest.mark.parametrize('pattern', lb.PATTERNS)
@pytest.mark.parametrize('B,S,H,dh', DENSE)
def test_dense_every_element_within_its_bound(ops, B, S, H, dh, pattern):
    qkv, pad, do, res = _dense_ref(B, S, H, dh, pattern)
    d = H * dh
    assert ops.attn_long_supported(BF16, S, dh)
    assert ops.L.lib().b4c_attn_long_bwd_workspace_bytes(B * S, H, dh) == B * S * d * 4
    o, lse, dqkv = _long(ops, qkv.cuda().to(BF16), pad.cuda(), do.cuda().to(BF16), B, S, H, dh)
    got = _split(o, lse, dqkv, d)
    tag = '(%d,%d,%d,%d)-%s' % (B, S, H, dh, pattern)
    ratios = {n: lb.check('%s %s' % (tag, n), got[n], *res[n]) for n in NAMES}
    _report('dense', tag, ratios)
    # padded keys: the bound is an exact 0 there (check() has demanded exact zeros); make sure the case has some
    assert float(res['dk'][1][pad.bool().reshape(-1)].max()) == 0.0 and int(pad.sum()) > 0


# ---- packed -----------------------------------------------------------------------------------------------------------------------
PACKED = [([1100, 513, 1, 512, 40, 700, 257], 2, 64), ([600, 33, 1024], 4, 32)]


@functools.lru_cache(maxsize=None)
def _packed_case(i):
    lens, H, dh = PACKED[i]
    qkv, cu, do = lb.packed_inputs(lens, H, dh)
    return qkv, cu, do


@pytest.mark.parametrize('i', range(len(PACKED)), ids=lambda i: str(PACKED[i][0]).replace(' ', ''))
def test_packed_every_element_within_its_bound(ops, i):
    lens, H, dh = PACKED[i]
    qkv, cu, do = _packed_case(i)
    res = lb.attn_packed(qkv, cu, do, H, dh, 'mfma')
    B, d, T, S_max = len(lens), H * dh, sum(lens), max(lens)
    key_pad = torch.zeros(T, dtype=torch.uint8, device='cuda')
    o, lse, dqkv = _long(ops, qkv.cuda().to(BF16), key_pad, do.cuda().to(BF16), B, S_max, H, dh, cu=cu.cuda())
    got = _split(o, lb.packed_lse(lse.cpu(), cu), dqkv, d)
    ratios = {n: lb.check('packed %s %s' % (lens, n), got[n], *res[n]) for n in NAMES}
    _report('packed', str(lens).replace(' ', ''), ratios)


# ---- padding edge cases -----------------------------------------------------------------------------------------------------------
def test_sequence_with_every_key_padded_gets_uniform_weights(ops):
    """Sequence 1 pads every key: its scores are all -1e9 in fp32 (the score itself is below the spacing of fp32 numbers there), the
    weights uniform over all its keys.  The reference is lb.attn_dense on the statement of that: sequence 1's q rows zero and its
    keys live -- uniform weights, the same o and its bound; the other sequences as they are.  lse of sequence 1 is -1e9 + log S
    within the fp32 spacing at 1e9 (64); its padded keys' dK / dV are exact zeros, and so is its dS: dQ too."""
    B, S, H, dh = 3, 600, 2, 64
    d = H * dh
    qkv, pad, do = lb.dense_inputs(BF16, B, S, H, dh, 'long')
    pad[1, :] = 1
    ref_qkv, ref_pad = qkv.clone(), pad.clone()
    ref_qkv.view(B, S, 3 * d)[1, :, :d] = 0.0
    ref_pad[1, :] = 0
    res = lb.attn_dense(ref_qkv, ref_pad, do, B, S, H, dh, 'mfma')
    o, lse, dqkv = _long(ops, qkv.cuda().to(BF16), pad.cuda(), do.cuda().to(BF16), B, S, H, dh)
    got = _split(o, lse, dqkv, d)
    ratios = {'o': lb.check('all-padded o', got['o'], *res['o'])}
    others = torch.tensor([0, 2])
    rows = torch.cat([torch.arange(b * S, (b + 1) * S) for b in others.tolist()])
    ratios['lse'] = lb.check('all-padded lse', lse.cpu()[others], res['lse'][0][others], res['lse'][1][others])
    for n in ('dq', 'dk', 'dv'):
        ratios[n] = lb.check('all-padded %s' % n, got[n].cpu()[rows], res[n][0][rows], res[n][1][rows])
    _report('dense', 'every-key-padded', ratios)
    assert float((lse[1].double().cpu() - (-1e9 + np.log(S))).abs().max()) <= 64.0
    assert float(dqkv.view(B, S, 3 * d)[1].abs().max()) == 0.0
    # the mean of V, per head: what uniform weights give
    want = qkv.view(B, S, 3 * d)[1, :, 2 * d:].double().mean(0)
    assert float((o.view(B, S, d)[1].double().cpu() - want[None]).abs().max()) < 2.0 ** -7 * float(want.abs().max()) + 1e-6


def test_leading_pads_under_the_causal_mask(ops):
    """S = 600 with the first 300 keys of sequence 0 padded (more than a key block, and whole query tiles whose visible keys are all
    padded), the first 7 of sequence 1, none of sequence 2; dO zero on the pad rows.  Everything is finite; o, lse of the rows from
    the first live key on and the gradient of every row meet the causal parity bounds (tests/test_gpu_causal_attn.py::test_leading_pads)."""
    B, S, H, dh = 3, 600, 2, 64
    d = H * dh
    g = torch.Generator().manual_seed(S + dh)
    pad = torch.zeros(B, S, dtype=torch.uint8)
    pad[0, :300] = 1
    pad[1, :7] = 1
    real = pad == 0
    qd = (torch.randn(B * S, 3 * d, generator=g) * 0.8).to(BF16).cuda()
    do = torch.randn(B, S, d, generator=g)
    do[~real] = 0.0
    dod = do.reshape(B * S, d).to(BF16).cuda()
    o, lse, dqkv = _long(ops, qd, pad.cuda(), dod, B, S, H, dh, causal=True)
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(dqkv).all())
    o_ref, lses, g_ref = cr.attention_grads(qd, dod, [S] * B, H, dh, pad.reshape(-1))
    rows = real.reshape(-1)
    sel = real[:, None, :].expand(B, H, S)
    e_o, e_g = rel_err(o.cpu()[rows], o_ref[rows]), rel_err(dqkv, g_ref)
    e_l = float((lse.double().cpu() - torch.stack(lses))[sel].abs().max())
    print('attn long causal, leading pads: rel_err(o) %.3e  |dlse| %.3e  rel_err(dqkv) %.3e' % (e_o, e_l, e_g))
    assert e_o < TOL_O and e_l < TOL_LSE and e_g < TOL_G
    for b in range(B):          # per sequence too: the padded one is not averaged away
        r = slice(b * S, (b + 1) * S)
        assert rel_err(o.cpu()[r][real[b]], o_ref[r][real[b]]) < TOL_O and rel_err(dqkv[r], g_ref[r]) < TOL_G, b
    assert float(dqkv.view(B, S, 3 * d)[~real].abs().max()) == 0.0


# ---- causal -----------------------------------------------------------------------------------------------------------------------
def _grid_pads(B, S):
    pad = torch.zeros(B, S, dtype=torch.uint8)
    pad[0, S - 4:] = 1
    if B > 1:
        pad[1, 5:S - 1] = 1
    return pad


@pytest.mark.parametrize('B,S,H,dh', [(2, 600, 2, 64), (1, 1057, 2, 32)])
def test_causal_dense_matches_float64(ops, B, S, H, dh):
    g = torch.Generator().manual_seed(S + dh)
    d = H * dh
    qd = (torch.randn(B * S, 3 * d, generator=g) * 0.8).to(BF16).cuda()
    dod = torch.randn(B * S, d, generator=g).to(BF16).cuda()
    pad = _grid_pads(B, S)
    o, lse, dqkv = _long(ops, qd, pad.cuda(), dod, B, S, H, dh, causal=True)
    o_ref, lses, g_ref = cr.attention_grads(qd, dod, [S] * B, H, dh, pad.reshape(-1))
    e_o, e_g = rel_err(o, o_ref), rel_err(dqkv, g_ref)
    e_l = max(float((lse[b].double().cpu() - lses[b]).abs().max()) for b in range(B))
    print('attn long causal (%d,%d,%d,%d): rel_err(o) %.3e  |dlse| %.3e  rel_err(dqkv) %.3e' % (B, S, H, dh, e_o, e_l, e_g))
    assert e_o < TOL_O and e_l < TOL_LSE and e_g < TOL_G
    assert float(dqkv[:, d:].reshape(B, S, 2 * d)[0, S - 4:].abs().max()) == 0.0          # padded keys: exactly zero dK / dV
    o_bi, _ = ops.attn_long_fwd(qd, pad.cuda(), B, S, H, dh)
    assert not torch.equal(o_bi, o)


def test_causal_packed_matches_float64(ops):
    lens, H, dh = PACKED[0]
    qkv, cu, do = _packed_case(0)
    B, d, T, S_max = len(lens), H * dh, sum(lens), max(lens)
    off = [int(c) for c in cu]
    qd, dod = qkv.cuda().to(BF16), do.cuda().to(BF16)
    pad = torch.zeros(T, dtype=torch.uint8)
    for b, L in enumerate(lens):
        if L >= 8:
            pad[off[b] + L - 2:off[b] + L] = 1
    o, lse, dqkv = _long(ops, qd, pad.cuda(), dod, B, S_max, H, dh, cu=cu.cuda(), causal=True)
    o_ref, lses, g_ref = cr.attention_grads(qd, dod, lens, H, dh, pad)
    for b, L in enumerate(lens):
        rows = slice(off[b], off[b] + L)
        e_o, e_g = rel_err(o[rows], o_ref[rows]), rel_err(dqkv[rows], g_ref[rows])
        e_l = float((lse[b, :, :L].double().cpu() - lses[b]).abs().max())
        print('attn long causal packed, sequence of %d: rel_err(o) %.3e  |dlse| %.3e  rel_err(dqkv) %.3e' % (L, e_o, e_l, e_g))
        assert e_o < TOL_O and e_l < TOL_LSE and e_g < TOL_G, (b, L)


def test_causal_rows_behind_the_query_have_no_weight_and_no_gradient(ops):
    """Packed list 0, the sequence of 513 rows (between two others), p = 400.
    Forward: its q | k | v rows behind p replaced by finite values of magnitude up to 1e4 (NaN-free but huge): o and lse of its rows
    <= p keep every bit -- the keys behind a query have weight exactly 0 -- and everything stays finite.
    Backward: dO zero behind p and the rows behind p replaced by other values of ordinary size: the gradient of the rows <= p keeps
    every bit, the gradient of the rows behind p is exactly 0."""
    lens, H, dh = PACKED[0]
    qkv, cu, do = _packed_case(0)
    B, d, T, S_max = len(lens), H * dh, sum(lens), max(lens)
    b, p = 1, 400
    assert lens[b] == 513
    r0 = int(cu[b])
    g = torch.Generator().manual_seed(p)
    front, behind = slice(r0, r0 + p + 1), slice(r0 + p + 1, r0 + lens[b])
    huge, other = qkv.clone(), qkv.clone()
    huge[behind] = ((torch.rand(lens[b] - p - 1, 3 * d, generator=g) * 2 - 1) * 1e4).to(BF16).float()
    other[behind] = (torch.randn(lens[b] - p - 1, 3 * d, generator=g) * 0.8).to(BF16).float()
    do = do.clone()
    do[behind] = 0.0
    key_pad = torch.zeros(T, dtype=torch.uint8, device='cuda')
    cud, dod = cu.cuda(), do.cuda().to(BF16)
    o0, l0, g0 = _long(ops, qkv.cuda().to(BF16), key_pad, dod, B, S_max, H, dh, cu=cud, causal=True)
    o1, l1, g1 = _long(ops, other.cuda().to(BF16), key_pad, dod, B, S_max, H, dh, cu=cud, causal=True)
    o2, l2 = ops.attn_long_fwd(huge.cuda().to(BF16), key_pad, B, S_max, H, dh, cu=cud, causal=True)
    for o_, l_ in ((o1, l1), (o2, l2)):
        assert torch.equal(o0[front], o_[front]) and torch.equal(l0[b, :, :p + 1], l_[b, :, :p + 1])
        assert bool(torch.isfinite(o_).all()) and bool(torch.isfinite(l_[b, :, :lens[b]]).all())
        assert not torch.equal(o0[behind], o_[behind])                                 # (the rows behind p did change)
    assert torch.equal(g0[front], g1[front]) and bool(torch.isfinite(g1).all())
    assert float(g0[behind].abs().max()) == 0.0 and float(g1[behind].abs().max()) == 0.0
    assert float(g0[front].abs().max()) > 0
    # every other sequence is untouched
    keep = torch.ones(T, dtype=torch.bool)
    keep[r0:r0 + lens[b]] = False
    assert torch.equal(o0[keep], o1[keep]) and torch.equal(o0[keep], o2[keep]) and torch.equal(g0[keep], g1[keep])
    # the bidirectional launch sees them
    ob = [ops.attn_long_fwd(t.cuda().to(BF16), key_pad, B, S_max, H, dh, cu=cu.cuda())[0][front] for t in (qkv, other)]
    assert not torch.equal(ob[0], ob[1])


# ---- dropout ----------------------------------------------------------------------------------------------------------------------
RATE = 0.3


def _recover(ops, lens, packed, H, dh, seed):
    """the passes of tests/test_gpu_attn_dropout_routes.py through the streamed kernels -> (fwd, bwd, want): bool [H, L, L] per sequence"""
    B, S_arg = len(lens), max(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    d, T = H * dh, int(off[-1])
    cu = torch.tensor(off, dtype=torch.int32, device='cuda') if packed else None
    pad = torch.zeros(T, dtype=torch.uint8) if packed else ad.recovery_pads(B, S_arg).reshape(-1)
    padd = pad.cuda()
    n_real = [int((pad[off[b]:off[b] + L] == 0).sum()) for b, L in enumerate(lens)]
    keep = ops.attn_keep_mask(seed, B, H, S_arg, RATE)
    fwd = [torch.zeros(H, L, L, dtype=torch.bool) for L in lens]
    bwd = [torch.zeros(H, L, L, dtype=torch.bool) for L in lens]
    for p in range(ad.recovery_passes(S_arg, dh)):
        qkv, do = ad.recovery_operands(lens, H, dh, p, BF16)
        o, lse, dqkv = _long(ops, qkv.cuda(), padd, do.cuda(), B, S_arg, H, dh, cu=cu, rate=RATE, seed=seed)
        assert not dqkv[:, :2 * d].any(), ('dQ, dK', p)                       # exactly zero: k = 0, and q = 0
        lse = lse.cpu()
        for b, L in enumerate(lens):                                          # that of the undropped softmax: uniform probabilities
            assert float((lse[b, :, :L] - float(np.log(n_real[b]))).abs().max()) < 1e-4, ('lse', b, p)
        ad.recovery_collect(fwd, bwd, o.float().cpu(), dqkv[:, 2 * d:].float().cpu(), lens, H, dh, p)
    want = [keep[b, :, :L, :L] & (pad[off[b]:off[b] + L] == 0)[None, None, :] for b, L in enumerate(lens)]
    return fwd, bwd, want


@pytest.mark.parametrize('lens,packed,H,dh', [([600, 600], False, 2, 64), ([600, 33, 700], True, 2, 64)], ids=['dense', 'packed'])
def test_dropout_outputs_are_the_masks(ops, lens, packed, H, dh):
    """q = k = 0 and one-hot V / dO windows: the nonzero patterns of o (forward) and dV (backward) ARE ops.attn_keep_mask's bits AND
    NOT pad, bit for bit -- so the two directions agree on the mask as well"""
    fwd, bwd, want = _recover(ops, lens, packed, H, dh, 0x10C6 + sum(lens) + dh)
    for b, w in enumerate(want):
        for name, got in (('o', fwd), ('dV', bwd)):
            if not torch.equal(got[b], w):
                bad = (got[b] != w).nonzero()
                raise AssertionError('%s of sequence %d differs from mask AND NOT pad at %d (head, query, key) triples, the first %s'
                                     % (name, b, bad.shape[0], bad[:6].tolist()))
        assert torch.equal(fwd[b], bwd[b])
    kept = float(torch.cat([w.reshape(-1) for w in want]).float().mean())
    if packed:
        assert 0.9 * (1 - RATE) < kept < 1.1 * (1 - RATE)


@pytest.mark.parametrize('lens,packed,H,dh', [([600, 600], False, 2, 64), ([600, 33, 700], True, 2, 64)], ids=['dense', 'packed'])
def test_dropout_parity_with_the_regenerated_mask(ops, lens, packed, H, dh):
    seed = 0xD0D0 + sum(lens) + dh
    B, S_arg = len(lens), max(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    d, T = H * dh, int(off[-1])
    g = torch.Generator().manual_seed(T + dh)
    qd = (torch.randn(T, 3 * d, generator=g) * 0.8).to(BF16).cuda()
    dod = torch.randn(T, d, generator=g).to(BF16).cuda()
    cu = torch.tensor(off, dtype=torch.int32, device='cuda') if packed else None
    pad = torch.zeros(T, dtype=torch.uint8) if packed else _grid_pads(B, S_arg).reshape(-1)
    keep = ops.attn_keep_mask(seed, B, H, S_arg, RATE)
    o, lse, dqkv = _long(ops, qd, pad.cuda(), dod, B, S_arg, H, dh, cu=cu, rate=RATE, seed=seed)
    for b, L in enumerate(lens):
        rows = slice(int(off[b]), int(off[b]) + L)
        o_ref, lse_ref, g_ref = ad.attention_grads(qd[rows], dod[rows], pad[rows][None], 1, L, H, dh, keep[b:b + 1, :, :L, :L], RATE)
        e_o, e_g = rel_err(o[rows], o_ref), rel_err(dqkv[rows], g_ref)
        e_l = float((lse[b, :, :L].double().cpu() - lse_ref[0]).abs().max())
        print('attn long dropout %s, sequence of %d: rel_err(o) %.3e  |dlse| %.3e  rel_err(dqkv) %.3e' % ('packed' if packed else 'dense', L, e_o, e_l, e_g))
        assert e_o < TOL_O and e_l < TOL_LSE and e_g < TOL_G, (b, L)
    o0, lse0 = ops.attn_long_fwd(qd, pad.cuda(), B, S_arg, H, dh, cu=cu)                  # the rate-0 launch: another o, the same lse bits
    assert not torch.equal(o0, o)
    for b, L in enumerate(lens):
        assert torch.equal(lse0[b, :, :L], lse[b, :, :L])


# ---- determinism, the resident kernels ------------------------------------------------------------------------------------------------
def test_two_launches_give_the_same_bits(ops):
    B, S, H, dh = 2, 1057, 2, 64
    qkv, pad, do, _ = _dense_ref(B, S, H, dh, 'long')
    qd, padd, dod = qkv.cuda().to(BF16), pad.cuda(), do.cuda().to(BF16)
    for causal, rate in ((False, 0.0), (True, 0.0), (False, RATE)):
        a = _long(ops, qd, padd, dod, B, S, H, dh, rate=rate, seed=99, causal=causal)
        ops._workspace('attn_long_bwd', qd.device, 1).fill_(0xFF)                         # the accumulator's old contents do not matter
        b = _long(ops, qd, padd, dod, B, S, H, dh, rate=rate, seed=99, causal=causal)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (causal, rate)


def test_both_routes_lie_inside_the_bounds_at_512(ops):
    """S = 512, where the resident kernels still run: they and the streamed kernels are two evaluations inside the same element
    bounds, dense and packed (no bit equality: the key blocks are other sums)"""
    B, S, H, dh = 2, 512, 2, 64
    qkv, pad, do, res = _dense_ref(B, S, H, dh, 'long')
    d = H * dh
    qd, padd, dod = qkv.cuda().to(BF16), pad.cuda(), do.cuda().to(BF16)
    o, lse = ops.attn_fwd(qd, padd, B, S, H, dh)
    routes = {'resident': _split(o, lse, ops.attn_bwd(qd, padd, o, dod, lse, B, S, H, dh), d),
              'streamed': _split(*_long(ops, qd, padd, dod, B, S, H, dh), d)}
    for route, got in routes.items():
        _report('dense-512-' + route, '(2,512,2,64)', {n: lb.check('512 %s %s' % (route, n), got[n], *res[n]) for n in NAMES})
    lens = [512, 40, 300]
    qkv, cu, do = lb.packed_inputs(lens, H, dh)
    res = lb.attn_packed(qkv, cu, do, H, dh, 'mfma')
    qd, dod, cud = qkv.cuda().to(BF16), do.cuda().to(BF16), cu.cuda()
    key_pad = torch.zeros(sum(lens), dtype=torch.uint8, device='cuda')
    o, lse = ops.attn_fwd(qd, key_pad, len(lens), 512, H, dh, cud)
    dqkv = ops.attn_bwd(qd, key_pad, o, dod, lse, len(lens), 512, H, dh, cud)
    o2, lse2, dqkv2 = _long(ops, qd, key_pad, dod, len(lens), 512, H, dh, cu=cud)
    for route, got in (('resident', _split(o, lb.packed_lse(lse.cpu(), cu), dqkv, d)), ('streamed', _split(o2, lb.packed_lse(lse2.cpu(), cu), dqkv2, d))):
        _report('packed-512-' + route, str(lens).replace(' ', ''), {n: lb.check('512 packed %s %s' % (route, n), got[n], *res[n]) for n in NAMES})
