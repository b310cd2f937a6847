"""The encoder blocks past the fused routes' row limit: M = 2^24 + 13 token rows, bf16, d_model 128, dropout 0.1, through the
autograd blocks with the arena routes on (the training step's configuration).

b4c_ffn_bwd and b4c_attn_out_bwd address their row chunks with 32-bit byte offsets and refuse M >= 2^24 rows; b4c_gemm_dxdw refuses
a residual of M * pitch * 2 >= 2^32 bytes (the Q | K | V route).  Their predicates (ops.ffn_bwd_supported, attn_out_bwd_supported,
dxdw_supported) send such a batch to the unfused kernels -- b4c_add_dropout_layernorm_bwd, b4c_gemm_nt (gate, residual),
b4c_gemm_tn -- which here run past 2^31 elements for the first time ([M][128] bf16: 2^31 elements end at row 2^24, the last 13
rows; the attention block's [M][384] q | k | v past row 5,592,405).

Every row-local result (the forward's h, z, statistics and output; dX; the attention tail's d_o) is checked on EVERY row against
a float64 restatement taken in chunks on the GPU from the same bf16 inputs and the kernels' own saved activations; the row sums
(dW, db, dgamma, dbeta) against float64 sums over all rows.  The dropout keep-masks come from a restatement of ops.keep_mask
(itself checked against ops.keep_mask on rows at both ends).  The attention kernels cannot take 2^24 tokens in one launch: the
attention block runs with its one-key restatement in their place (see that test).

Inputs (x, dout) have column means of either sign that also change sign and size from one 2^20-row block to the next: the row
sums do not cancel to noise, and rows read from the wrong block move them by the number of rows times the difference of the
block means -- for a wrapped 32-bit offset (millions of rows) far outside the tolerance below.

Tolerances (bf16 rounds to within 2^-8 of a value, fp32 to 2^-24).  Row-local results, entry by entry: a GEMM output (h, q | k | v;
the GEMM epilogues round the product and then product + bias to bf16) within 2^-6 of the sum of the magnitudes of its terms; z
within 2^-6 of |z| + |dropout(y)| (z rounded once, y up to twice); the LayerNorm output within 2^-5 of |out| + |gamma| rstd max|z|
(the kernels normalise the fp32 row before its rounding to the saved z).  dX and d_o within 2^-5 of the row's largest entry
(the roundings of dz, dy, dh in front of them and of the result, through sums that can cancel).  Row sums over M = 16.8 M rows of
products of bf16-rounded intermediates, accumulated in fp32: the bf16 roundings are unbiased and independent between rows, their
sum stays within 2^-8 sqrt(sum of squares of the terms) per rounding, 2^-6 of it allowed; fp32 accumulation is off by at most
2^-24 of the magnitudes added per addition in a chain, and the kernels add rows in chains of at most 2^15 (the grouped dW splits
the rows into at least 8 chunks, 64 rows per MFMA step; gemm_dxdw's 256 workgroups, 32 rows per step), then reduce at most a few
hundred partials: 2^-9 of the sum of the magnitudes -- about 2^15 rows' worth of terms, against the millions of rows a skipped
or wrapped block of rows would move.  The row-local checks see any such row in any case."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M = (1 << 24) + 13
RATE = 0.1
CHUNK = 1 << 20

_ROUNDS = [(13, 15, 26, 6), (17, 29, 16, 24), (13, 15, 26, 6)]


def _keep_rows(seed, r0, r1, rate):
    """ops.keep_mask (Threefry-2x32, ops.rand64_host) for the elements of rows r0 .. r1 - 1 of a [*][128] tensor, on the GPU"""
    m32 = 0xFFFFFFFF
    ctr = torch.arange(r0 * 32, r1 * 32, dtype=torch.int64, device='cuda')       # element e = 128 r + c, counter e >> 2
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & m32, seed >> 32
    k2 = 0x1BD11BDA ^ k0 ^ k1
    x0 = ((ctr & m32) + k0) & m32
    x1 = ((ctr >> 32) + k1) & m32
    for rs, (a0, a1, j) in zip(_ROUNDS, [(k1, k2, 1), (k2, k0, 2), (k0, k1, 3)]):
        for r in rs:
            x0 = (x0 + x1) & m32
            x1 = (((x1 << r) | (x1 >> (32 - r))) & m32) ^ x0
        x0 = (x0 + a0) & m32
        x1 = (x1 + a1 + j) & m32
    u16 = torch.stack([x0 & 0xFFFF, x0 >> 16, x1 & 0xFFFF, x1 >> 16], 1)         # element 4 c + i: 16 bits i of x0 | x1 << 32
    return (u16 >= _threshold(rate)).reshape(r1 - r0, 128)


def _threshold(rate):
    t = np.float32(rate) * np.float32(65536.0)
    return int(t) + (1 if np.float32(int(t)) < t else 0)


def _check_keep(seed):
    from bert4clickpath_amd import ops
    assert np.array_equal(_keep_rows(seed, 0, 40, RATE).cpu().numpy().reshape(-1), ops.keep_mask(seed, 40 * 128, RATE))
    for r0 in (0, M - 40):
        e = np.arange(r0 * 128, (r0 + 40) * 128, dtype=np.uint64)
        h = ops.rand64_host(seed, e >> np.uint64(2))
        u16 = (h >> (np.uint64(16) * (e & np.uint64(3)))) & np.uint64(0xFFFF)
        want = u16 >= np.uint64(_threshold(RATE))
        got = _keep_rows(seed, r0, r0 + 40, RATE).cpu().numpy().reshape(-1)
        assert np.array_equal(got, want), r0


def _arena(*params):
    """the parameters' gradients as an arena's in-place views (ops.grad_sinks: the fused routes' condition)"""
    from bert4clickpath_amd import ops
    c = ops.ArenaContext()
    for p in params:
        p.grad = torch.zeros_like(p)
        p._b4c_ctx = c
    return c


def _close(name, got, ref, bound, r0):
    """row-local results: every entry within its bound (a tensor, or a number per row times the row's largest float64 entry)"""
    err = (got.double() - ref).abs()
    if not torch.is_tensor(bound):
        bound = bound * ref.abs().amax(1, keepdim=True)
    bound = bound.expand_as(err)
    off = (err > bound).any(1)
    bad = off.nonzero().reshape(-1)
    assert bad.numel() == 0, '%s: %d rows off, first %s (worst %s of %s allowed)' % (
        name, bad.numel(), (bad[:6] + r0).tolist(), err[bad[:6]].amax(1).tolist(),
        [float(bound[i][int((err[i] / (bound[i] + 1e-300)).argmax())]) for i in bad[:6].tolist()])


def _dropped(keep, y):
    return torch.where(keep, y / (1.0 - RATE), torch.zeros((), dtype=torch.float64, device=y.device))


class _Sum:
    """a float64 row sum with the masses its tolerance needs"""

    def __init__(self):
        self.s = self.sq = self.l1 = 0

    def add(self, a, b=None):
        """+= a^T b (b None: column sums of a)"""
        if b is None:
            self.s, self.sq, self.l1 = self.s + a.sum(0), self.sq + (a * a).sum(0), self.l1 + a.abs().sum(0)
        else:
            self.s, self.sq, self.l1 = self.s + a.T @ b, self.sq + (a * a).T @ (b * b), self.l1 + a.abs().T @ b.abs()

    def check(self, name, got):
        g = got.double()
        tol = 2 ** -6 * self.sq.sqrt() + 2 ** -9 * self.l1
        err = (g - self.s).abs()
        i = int((err / (tol + 1e-300)).argmax())
        assert bool((err <= tol).all()), '%s: entry %d off by %.3g (sum %.6g, allowed %.3g)' % (
            name, i, float(err.reshape(-1)[i]), float(self.s.reshape(-1)[i]), float(tol.reshape(-1)[i]))


def _stats_close(stats, mean, rstd, z, r0):
    """the kernels take mean and 1 / std of the fp32 row before its rounding to the saved bf16 z (within 2^-8 |z| entry by entry):
    the mean within 2^-8 mean|z|, the variance within 2^-7 mean(|z - mean| |z|) -- twice that allowed"""
    dev = z - mean[:, None]
    var = (dev * dev).mean(1)
    bad = ((stats[:, 0] - mean).abs() > 2 ** -7 * z.abs().mean(1)) | \
        ((stats[:, 1] / rstd - 1).abs() > 2 ** -7 * (dev.abs() * z.abs()).mean(1) / var)
    assert not bool(bad.any()), ('statistics', (bad.nonzero().reshape(-1)[:6] + r0).tolist())


def _ln_bwd(dout, z, stats, gamma, keep):
    mean, rstd = stats[:, :1], stats[:, 1:]
    xh = (z - mean) * rstd
    gv = dout * gamma
    dz = rstd * (gv - gv.mean(1, keepdim=True) - xh * (gv * xh).mean(1, keepdim=True))
    return xh, dz, torch.where(keep, dz / (1.0 - RATE), torch.zeros((), dtype=torch.float64, device=dz.device))


def _ln_fwd(v, gamma, beta):
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    return (v - mean) * rstd * gamma + beta, mean[:, 0], rstd[:, 0]


def _rows(n, scale, g, pattern):
    """[n][128] bf16: scale * (N(0, 1) + a mean per column, uniform in [-1, 1], times pattern(b) in rows block b = row >> 20)"""
    mu = torch.rand(128, generator=g, device='cuda') * 2 - 1
    b = torch.arange(n, device='cuda') >> 20
    f = torch.tensor([pattern(i) for i in range(int(b[-1]) + 1)], dtype=torch.float32, device='cuda')[b]
    return ((torch.randn(n, 128, generator=g, device='cuda') + f[:, None] * mu) * scale).bfloat16()


# block means of x and dout: sign and size change from one 2^20-row block to the next, in two different patterns, so that rows
# read from another block (a wrapped 32-bit offset) move the row sums by (rows) * (difference of the means), whatever the noise
X_MEANS = lambda b: (-1) ** b * (1 + b / 16)
DOUT_MEANS = lambda b: (-1) ** (b // 2) * (1 + (b % 5) / 4)


def _param(shape, scale, g):
    return torch.nn.Parameter((torch.randn(*shape, generator=g, device='cuda') * scale).float())


def test_feed_forward_block_past_the_fused_row_limit():
    """forward b4c_ffn_fwd; backward b4c_add_dropout_layernorm_bwd + b4c_gemm_nt (gate, residual) + grouped b4c_gemm_tn"""
    from bert4clickpath_amd import ops
    seed, F = 4242, 100
    _check_keep(seed)
    g = torch.Generator(device='cuda').manual_seed(7)
    w1, b1 = _param((128, F), 0.09, g), _param((F,), 0.1, g)
    w2, b2 = _param((F, 128), 0.1, g), _param((128,), 0.1, g)
    gamma, beta = torch.nn.Parameter(1.0 + _param((128,), 0.1, g).detach()), _param((128,), 0.1, g)
    params = (w1, b1, w2, b2, gamma, beta)
    pk1, pk2 = ops.PackedLinear([w1], [b1]), ops.PackedLinear([w2], [b2])
    ctx = _arena(*params)
    x = _rows(M, 1.0, g, X_MEANS).requires_grad_(True)

    out = ops.FFNBlockFn.apply(x, w1, b1, w2, b2, gamma, beta, pk1, pk2, RATE, seed, True)
    xs, h, z, stats, _ = out.grad_fn.saved_tensors          # (what the backward reads: kept past it)
    dout = _rows(M, 0.05, g, DOUT_MEANS)
    out.backward(dout)                              # (B4CError from b4c_ffn_bwd while its predicate let 2^24 rows through)
    ops.flush_pending_dw(ctx)
    ops.join_side_work(ctx)
    torch.cuda.synchronize()
    Fp = h.shape[1]
    _, wc1, bb1 = pk1.get(torch.bfloat16, 128, True)        # wc1 [128][Fp]: row = input feature
    _, wc2, bb2 = pk2.get(torch.bfloat16, Fp, True)         # wc2 [Fp][128]: row = hidden column
    W1, W2 = wc1.double()[:, :F], wc2.double()[:F]
    B1, B2, gam, bet = bb1.double()[:F], bb2.double(), gamma.detach().double(), beta.detach().double()

    sums = {n: _Sum() for n in ('dW1', 'db1', 'dW2', 'db2', 'dgamma', 'dbeta')}
    for r0 in range(0, M, CHUNK):
        r1 = min(M, r0 + CHUNK)
        keep = _keep_rows(seed, r0, r1, RATE)
        xr, hr, zr, sr = xs[r0:r1].double(), h[r0:r1, :F].double(), z[r0:r1].double(), stats[r0:r1].double()
        # forward: h from x, z from the kernel's h, statistics and output from the kernel's z
        _close('h', h[r0:r1, :F], torch.relu(xr @ W1 + B1), 2 ** -6 * (xr.abs() @ W1.abs() + B1.abs()), r0)
        z_ref = xr + _dropped(keep, hr @ W2 + B2)
        _close('z', z[r0:r1], z_ref, 2 ** -6 * (z_ref.abs() + _dropped(keep, hr.abs() @ W2.abs() + B2.abs())), r0)
        o_ref, mean, rstd = _ln_fwd(zr, gam, bet)
        _close('out', out[r0:r1].detach(), o_ref, 2 ** -5 * (o_ref.abs() + gam.abs() * (rstd * zr.abs().amax(1))[:, None]), r0)
        _stats_close(sr, mean, rstd, zr, r0)
        # backward from the kernels' saved activations
        xh, dz, dy = _ln_bwd(dout[r0:r1].double(), zr, sr, gam, keep)
        dh = (dy @ W2.T) * (hr > 0)
        _close('dx', x.grad[r0:r1], dh @ W1.T + dz, 2 ** -5, r0)
        sums['dW1'].add(xr, dh)
        sums['db1'].add(dh)
        sums['dW2'].add(hr, dy)
        sums['db2'].add(dy)
        sums['dgamma'].add(dout[r0:r1].double() * xh)
        sums['dbeta'].add(dout[r0:r1].double())
        del keep, xr, hr, zr, sr, z_ref, o_ref, xh, dz, dy, dh
    for n, p in zip(('dW1', 'db1', 'dW2', 'db2', 'dgamma', 'dbeta'), params):
        sums[n].check(n, p.grad)


def test_attention_block_past_the_fused_row_limit():
    """forward gemm_nt (q | k | v) + gemm_nt_add_ln; backward b4c_add_dropout_layernorm_bwd, b4c_gemm_dxdw (output projection, no
    residual: no byte limit), b4c_gemm_nt with the residual + grouped b4c_gemm_tn (q | k | v: [M][384], 6.4 G elements).

    The attention kernels themselves take at most 65,535 (sequence, head) items per launch -- with 2 heads of 64 and sequences of
    at most 512 tokens, fewer than 2^24 tokens -- so here every token is a sequence of its own: attention over one key is
    o = v, and its gradient dq = dk = 0, dv = d_o.  The block runs with that restatement in place of ops.attn_fwd / attn_bwd;
    everything around it is the block's own code and kernels."""
    from bert4clickpath_amd import ops
    seed, H = 5151, 2
    _check_keep(seed)
    g = torch.Generator(device='cuda').manual_seed(11)
    ws = [_param((128, 128), 0.09, g) for _ in range(4)]
    bs = [_param((128,), 0.1, g) for _ in range(4)]
    gamma, beta = torch.nn.Parameter(1.0 + _param((128,), 0.1, g).detach()), _param((128,), 0.1, g)
    params = (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], ws[3], bs[3], gamma, beta)
    pk_qkv, pk_o = ops.PackedLinear(ws[:3], bs[:3]), ops.PackedLinear(ws[3:], bs[3:])
    ctx = _arena(*params)
    key_pad = torch.zeros(M, 1, dtype=torch.uint8, device='cuda')
    x = _rows(M, 1.0, g, X_MEANS).requires_grad_(True)

    seen, real = {}, (ops.attn_fwd, ops.attn_bwd)

    def attn_fwd(qkv, key_pad, B, S, H, dh, cu=None):
        assert (B, S, cu) == (M, 1, None)
        return qkv[:, 256:].contiguous(), torch.zeros(B, H, S, dtype=torch.float32, device=qkv.device)

    def attn_bwd(qkv, key_pad, o, d_o, lse, B, S, H, dh, cu=None, actx=None):
        dqkv = torch.zeros_like(qkv)
        dqkv[:, 256:] = d_o
        seen['d_o'] = d_o
        return dqkv
    ops.attn_fwd, ops.attn_bwd = attn_fwd, attn_bwd
    try:
        out = ops.AttnBlockFn.apply(x, key_pad, *params, pk_qkv, pk_o, M, 1, H, RATE, seed, True)
        xs, _, qkv, o, _, z, stats, _ = out.grad_fn.saved_tensors
        dout = _rows(M, 0.05, g, DOUT_MEANS)
        out.backward(dout)                          # (B4CError from b4c_attn_out_bwd while its predicate let 2^24 rows through)
        ops.join_side_work(ctx)
        torch.cuda.synchronize()
    finally:
        ops.attn_fwd, ops.attn_bwd = real
    d_o = seen['d_o']
    _, wc_qkv, b_qkv = pk_qkv.get(torch.bfloat16, 128, True)    # wc [128][384]: row = input feature
    _, wc_o, b_o = pk_o.get(torch.bfloat16, 128, True)
    Wqkv, Wo, Wv, Bqkv, Bo = wc_qkv.double(), wc_o.double(), wc_qkv.double()[:, 256:], b_qkv.double(), b_o.double()
    gam, bet = gamma.detach().double(), beta.detach().double()

    sums = {n: _Sum() for n in ('dWv', 'dbv', 'dWo', 'dbo', 'dgamma', 'dbeta')}
    for r0 in range(0, M, CHUNK):
        r1 = min(M, r0 + CHUNK)
        keep = _keep_rows(seed, r0, r1, RATE)
        xr, orr, zr, sr = xs[r0:r1].double(), o[r0:r1].double(), z[r0:r1].double(), stats[r0:r1].double()
        # forward: q | k | v from x, z from o (= v), statistics and output from the kernels' z
        _close('qkv', qkv[r0:r1], xr @ Wqkv + Bqkv, 2 ** -6 * (xr.abs() @ Wqkv.abs() + Bqkv.abs()), r0)
        z_ref = xr + _dropped(keep, orr @ Wo + Bo)
        _close('z', z[r0:r1], z_ref, 2 ** -6 * (z_ref.abs() + _dropped(keep, orr.abs() @ Wo.abs() + Bo.abs())), r0)
        o_ref, mean, rstd = _ln_fwd(zr, gam, bet)
        _close('out', out[r0:r1].detach(), o_ref, 2 ** -5 * (o_ref.abs() + gam.abs() * (rstd * zr.abs().amax(1))[:, None]), r0)
        _stats_close(sr, mean, rstd, zr, r0)
        # backward: the tail from the kernels' saved activations, the projections from d_o (dq = dk = 0, dv = d_o)
        xh, dz, dy = _ln_bwd(dout[r0:r1].double(), zr, sr, gam, keep)
        _close('d_o', d_o[r0:r1], dy @ Wo.T, 2 ** -5, r0)
        dv = d_o[r0:r1].double()
        _close('dx', x.grad[r0:r1], dv @ Wv.T + dz, 2 ** -5, r0)
        sums['dWv'].add(xr, dv)
        sums['dbv'].add(dv)
        sums['dWo'].add(orr, dy)
        sums['dbo'].add(dy)
        sums['dgamma'].add(dout[r0:r1].double() * xh)
        sums['dbeta'].add(dout[r0:r1].double())
        del keep, xr, orr, zr, sr, z_ref, o_ref, xh, dz, dy, dv
    for w, b in zip(ws[:2], bs[:2]):
        assert not bool(w.grad.any()) and not bool(b.grad.any())       # (dq = dk = 0: their weights see exact zeros)
    sums['dWv'].check('dWv', ws[2].grad)
    sums['dbv'].check('dbv', bs[2].grad)
    sums['dWo'].check('dWo', ws[3].grad)
    sums['dbo'].check('dbo', bs[3].grad)
    sums['dgamma'].check('dgamma', gamma.grad)
    sums['dbeta'].check('dbeta', beta.grad)
