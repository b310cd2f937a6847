"""Row-by-row float64 references, element-wise derived bounds, launch geometry and input families for the five persistent kernels of
the d_model = 128 encoder: b4c_ffn_fwd, b4c_ffn_bwd, b4c_attn_out_bwd, b4c_ffn_act_fwd, b4c_ffn_act_bwd.

Every output X is compared ELEMENT by element (no tensor-wide scale anywhere) with a float64 restatement X_ref of the same formula
on the same bf16 inputs, under a bound of the form of tests/local_bounds.py,

    |X_gpu - X_ref| <= (1 + 2^-6) ( n u A_X  +  u_out |X_ref|  +  length 2^-24 A_X )  +  2^-109   (only where the rest is > 0)

with u = 2^-8 (bf16), A_X the absolute companion of X (the same formula with every factor replaced by its absolute value and every
subtraction by an addition) and n the number of bf16 roundings on X's path inside the kernel.  The code below carries the error of
every rounded intermediate forward as a tensor of its own (`e_*`): a rounding enters with u times the magnitude of the value that is
rounded (<= its companion), and goes through the later products with the absolute values of the other factors -- that is n u A_X
term by term, never more.  `length` is the number of fp32 additions behind an element: 128 + 8 for a row's LayerNorm sums and for a
128-deep dot product, Fp + 8 for a dot product over the hidden width, M + 8 for a sum over the M rows of a launch (the + 8 covers the
few fp32 products and scale factors beside the sum).  A bound of exactly 0 (a row without dOut, a hidden column behind a closed ReLU
gate, a dropped column) demands an exact 0.

Roundings per output (file:line of the instruction that rounds, under bert4clickpath_amd/csrc/; "out" = the stored output)

  kernel            output        n   where
  ----------------  ------------  --  ------------------------------------------------------------------------------------------
  b4c_ffn_bwd       dz (inside)   0   fp32 formula, -> bf16 ffn_bwd.hip:274 (kept in registers for the residual add)
                    dy (inside)   0   the fp32 dz * 1 / (1 - rate) where kept, -> bf16 ffn_bwd.hip:278 (not the rounded dz again)
                    dW2, db2      1   dy; fp32 sums (MFMA :332, bias :329), fp32 outputs
                    dh (inside)   1   dy; (dy W2^T) o [h > 0] -> bf16 ffn_bwd.hip:352
                    dW1, db1      2   dy, dh; fp32 sums (:200, :197)
                    dx            2   dy, dh through dh W1^T; + the bf16 dz (1 rounding of its own) in fp32 :226; out :227
                    dgamma        0   sum dOut * xhat, xhat in fp32 from the fp32 statistics (:261, :265)
                    dbeta         0   sum of the bf16 dOut in fp32 (:266): one row added to zeros is that row, bit for bit
  b4c_ffn_act_bwd   dz, dy        0   ffn_act_bwd.hip:246, :250
                    dW2, db2      1   dy
                    dh (inside)   2   dy; the fp32 sum dy W2^T -> bf16, times act'(u) in fp32, -> bf16: both ffn_act_bwd.hip:299
                    dW1, db1      3   dy, staged sum, dh
                    dx            3   (+ dz's own); out ffn_act_bwd.hip:196
                    dgamma/dbeta  0
  b4c_attn_out_bwd  dz            0   out attn_out_bwd.hip:179 (the fp32 formula, rounded once)
                    dy (inside)   0   -> bf16 attn_out_bwd.hip:178 / :183
                    d_o           1   dy; out attn_out_bwd.hip:136
                    dW, db        1   dy; fp32
                    dgamma/dbeta  0
  b4c_ffn_fwd       h             0   relu(fp32 sum + b1); out ffn_fwd_body.h:181
                    z             1   the staged bf16 h in front of h W2^T; y stays fp32 (:107); out :129
                    out, stats    1   from the UNROUNDED fp32 z (:114-:128); out :130; stats fp32 :131
  b4c_ffn_act_fwd   u             1   the fp32 sum x W1^T -> bf16 BEFORE the bias ffn_fwd_body.h:174; out :175
                    h             1   act(bf16(sum) + b1) in fp32 (the unrounded u); out :176
                    z             4   staged sum (1), staged h (1), y = bf16(bf16(h W2^T) + b2) (2) ffn_fwd_body.h:112; out :129
                    out, stats    4   as above

The GELU and its derivative are evaluated by the device in fp32 (common.h:237-249: 0.5 x (1 + erf(x / sqrt 2)) or the tanh form;
Phi(u) + u phi(u) or the tanh form's derivative).  Their term in the bound is TWICE the difference between an fp32 CPU evaluation of
that expression and the float64 one, element by element on the case's own u (the doubling covers the hardware's transcendental).
Measured on 2 M points of |u| <= 9 (tests/test_fused_rows_cpu.py): the difference is at most 4.4e-7 for the activation (both forms)
and 1.4e-7 (erf) / 5.6e-7 (tanh) for its derivative -- a few 2^-24 |u|, against the 2^-8 |h| of the stored value.  Where act'(u) is near 0 (u about -0.75) the first-order term |act'| e_u
vanishes and the second-order one, e_u^2 |act''| / 2 with |act''| <= 1, is added.

Launch geometry (read from the host code): 32-row tiles (DD_TOK, dxdw_common.h:7), a four-stage ring (DD_RING, dxdw_common.h:9), a
workgroup's tiles are blockIdx.x + t * gridDim.x, grid = min(tiles, 256) for the backward kernels (ffn_bwd_grid ffn_bwd.hip:440-443,
ao_bwd_grid attn_out_bwd.hip:282, the `grid` line ffn_act_bwd.hip:377) and min(tiles, 512) for the forward ones (the `grid` lines
ffn_fwd.hip:40 and ffn_act_fwd.hip:44).  With these caps 8192 k + 1 rows (k = 1..4) give workgroup 0 of a backward kernel k + 1 tiles,
the last of one row, and 40929 = 32 * 1279 + 1 makes that one-row tile the fifth of workgroup 255; forward: 16384 k + 1 and
81889 = 32 * 2559 + 1 (workgroup 511).  The fifth tile of a workgroup (tile 4 G) is the first to re-use a ring stage.
"""
import functools

import numpy as np
import torch

import paper_encoder_ref as pr
from local_bounds import SECOND_ORDER, U_BF16, U_F32, UNDERFLOW, _finish, bf16r, check  # noqa: F401

TILE, RING, CAP_BWD, CAP_FWD = 32, 4, 256, 512
LN_EPS = 1e-6
U = U_BF16

BWD_KINDS = ('ffn', 'act', 'ao')                 # b4c_ffn_bwd, b4c_ffn_act_bwd, b4c_attn_out_bwd
FWD_KINDS = ('ffn', 'act')
BWD_M = (2, 3, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193, 16385, 24577, 32769, 40929)
FWD_M = (1, 2, 31, 32, 33, 16383, 16384, 16385, 32769, 49153, 65537, 81889)
BWD_WIDE = (33, 8193, 16385, 24577, 32769, 40929)     # the row counts that also get F = 128, 8, 1 and rate 0
FWD_WIDE = (33, 16385, 32769, 49153, 65537, 81889)
BWD_UNLIKE_M, FWD_UNLIKE_M = (33, 8193, 40929), (33, 16385, 81889)
ROW_SUMS = {'ffn': ('dW1', 'db1', 'dW2', 'db2', 'dgamma', 'dbeta'), 'act': ('dW1', 'db1', 'dW2', 'db2', 'dgamma', 'dbeta'),
            'ao': ('dW', 'db', 'dgamma', 'dbeta')}
ROW_LOCAL = {'ffn': ('dx',), 'act': ('dx',), 'ao': ('dz', 'd_o')}
SHIFTS = (1, 2, 4, 16, 32, 8192, 16384)


def shapes(direction, with_width=True):
    """the stated matrix: (M, F, rate); every M at F = 100, rate 0.1; the wide ones also at F = 128, 8, 1 and at rate 0"""
    ms, wide = (BWD_M, BWD_WIDE) if direction == 'bwd' else (FWD_M, FWD_WIDE)
    out = []
    for M in ms:
        out.append((M, 100, 0.1))
        if M in wide:
            if with_width:
                out += [(M, 128, 0.1), (M, 8, 0.1), (M, 1, 0.1)]
            out.append((M, 100, 0.0))
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# launch geometry
# ----------------------------------------------------------------------------------------------------------------------------------
def tile_edges(M, cap):
    """The edge rows of a launch over M rows with a grid cap of `cap` workgroups: sorted, without duplicates, all < M."""
    T = -(-M // TILE)
    G = min(T, cap)
    full = M // TILE - 1                                 # the last full tile (-1: none)
    rows = [0, 31, 32, M - 2, M - 1, TILE * (T - 1), M - 1, TILE * (G - 1), TILE * (G - 1) + 31, TILE * G, TILE * 4 * G]
    if full >= 0:
        rows += [TILE * full, TILE * full + 31]
    for w in (0, G - 1):
        rows.append(TILE * (w + G * ((T - 1 - w) // G)))  # first row of the workgroup's last tile
    return sorted({r for r in rows if 0 <= r < M})


def row_params(M):
    """(m_r, s_r): s cycles through {1/4, 1, 4} (period 3), m / s through {-2 .. 2} (period 5)"""
    r = torch.arange(M)
    s = torch.tensor([0.25, 1.0, 4.0])[r % 3]
    return s * torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0])[r % 5], s


def _unlike(M, g, cols=128):
    m, s = row_params(M)
    return bf16r(m[:, None] + s[:, None] * torch.randn(M, cols, generator=g))


def keep_rows(seed, rows, rate):
    """the dropout keep-mask of rows `rows` of an [M][128] tensor (ops.keep_mask restated for single rows; rows >= M are allowed)"""
    from bert4clickpath_amd import ops
    rows = np.asarray(rows, dtype=np.uint64)
    if rate <= 0:
        return torch.ones(len(rows), 128, dtype=torch.bool)
    # element e of the tensor: counter e >> 2 (32 per row), one 16-bit uniform per element
    h = ops.rand64_host(seed, rows[:, None] * np.uint64(32) + np.arange(32, dtype=np.uint64)[None, :])
    u16 = ((h[:, :, None] >> (np.uint64(16) * np.arange(4, dtype=np.uint64))[None, None, :]) & np.uint64(0xFFFF)).reshape(len(rows), 128)
    t = np.float32(rate) * np.float32(65536.0)
    thr = int(t)
    if np.float32(thr) < t:
        thr += 1
    return torch.from_numpy(u16 >= np.uint64(thr))


@functools.lru_cache(maxsize=2)
def keep_all(seed, M, rate):
    return keep_rows(seed, np.arange(M), rate)


def stats_of(z):
    """[mean, rstd] of the rows of the bf16 z: float64, rounded to fp32"""
    z = z.double()
    return torch.cat([z.mean(1, keepdim=True), 1.0 / torch.sqrt(z.var(1, unbiased=False, keepdim=True) + LN_EPS)], 1).float()


# ----------------------------------------------------------------------------------------------------------------------------------
# the activation in float64 and in fp32 as the source states it (common.h:237-249)
# ----------------------------------------------------------------------------------------------------------------------------------
ACT_CODE = {'gelu': 2, 'gelu_tanh': 3}
_K, _C = 0.79788456080286536, 0.044715


def act64(name, u):
    if name == 'gelu':
        return 0.5 * u * (1.0 + torch.erf(u * 0.70710678118654752))
    return 0.5 * u * (1.0 + torch.tanh(_K * (u + _C * u * u * u)))


def act_grad64(name, u):
    if name == 'gelu':
        return 0.5 * (1.0 + torch.erf(u * 0.70710678118654752)) + u * 0.39894228040143268 * torch.exp(-0.5 * u * u)
    u = u.clamp(-10.0, 10.0)
    u2 = u * u
    t = torch.tanh(_K * (u + _C * u * u2))
    return 0.5 * (1.0 + t) + 0.5 * u * (1.0 - t * t) * _K * (1.0 + 3.0 * _C * u2)


def act32(name, u):
    return act64(name, u.float())                        # the same expression on fp32 tensors: fp32 arithmetic throughout


def act_grad32(name, u):
    return act_grad64(name, u.float())


def act_term(name, u):
    """twice |fp32 evaluation - float64 evaluation| of the activation, on these u"""
    return 2.0 * (act32(name, u).double() - act64(name, u.double())).abs()


def act_grad_term(name, u):
    return 2.0 * (act_grad32(name, u).double() - act_grad64(name, u.double())).abs()


# ----------------------------------------------------------------------------------------------------------------------------------
# float64 restatements (the helpers of tests/test_gpu_ffn_bwd.py, test_gpu_attn_out_bwd.py, test_gpu_ffn_fwd.py, test_gpu_ffn_act.py)
# ----------------------------------------------------------------------------------------------------------------------------------
def _d(t):
    return t.double().cpu()


def _ln_bwd64(dout, z, stats, gamma, keep, rate):
    mean, rstd = stats[:, :1], stats[:, 1:]
    xh = (z - mean) * rstd
    gv = dout * gamma
    dz = rstd * (gv - gv.mean(1, keepdim=True) - xh * (gv * xh).mean(1, keepdim=True))
    dy = torch.where(keep, dz / (1.0 - rate), torch.zeros((), dtype=torch.float64))
    return xh, gv, dz, dy


def ffn_bwd_float64(a, rate, act='relu'):
    """the feed-forward block's backward in float64 from the same bf16 inputs (no intermediate rounding):
    dx, dW1, db1, dW2, db2, dgamma, dbeta.  act: 'relu' (gate h > 0) | 'gelu' | 'gelu_tanh' (gate act'(u), a['u'])"""
    F = a['F']
    dout, z, gamma, h, x = _d(a['dout']), _d(a['z']), _d(a['gamma']), _d(a['h'])[:, :F], _d(a['x'])
    w1, w2 = _d(a['wc1'])[:, :F], _d(a['wc2'])[:F]
    xh, gv, dz, dy = _ln_bwd64(dout, z, _d(a['stats']), gamma, a['keep'], rate)
    gate = (h > 0) if act == 'relu' else pr.act_grad(act, _d(a['u'])[:, :F])
    dh = (dy @ w2.T) * gate
    return dh @ w1.T + dz, x.T @ dh, dh.sum(0), h.T @ dy, dy.sum(0), (dout * xh).sum(0), dout.sum(0)


def attn_out_bwd_float64(a, rate):
    """dz, d_o, dW, db, dgamma, dbeta of the attention block's tail"""
    dout, z, gamma, o, wc = _d(a['dout']), _d(a['z']), _d(a['gamma']), _d(a['o']), _d(a['wc'])
    xh, gv, dz, dy = _ln_bwd64(dout, z, _d(a['stats']), gamma, a['keep'], rate)
    return dz, dy @ wc.T, o.T @ dy, dy.sum(0), (dout * xh).sum(0), dout.sum(0)


def ffn_fwd_float64(a, rate, seed, act='relu', round_h=True):
    """h, (u,) z, out, stats of the block's forward.  round_h: the second Dense reads the bf16 of the float64 h (what the existing
    tests compare with); the bounds below use the unrounded form and count that rounding."""
    from bert4clickpath_amd import ops
    x, wt1, wt2 = _d(a['x']), _d(a['wt1']), _d(a['wt2'])
    M = x.shape[0]
    u = x @ wt1.T + _d(a['b1'])
    h = torch.relu(u) if act == 'relu' else pr.act(act, u)
    hb = h.bfloat16().double() if round_h else h
    y = hb @ wt2.T + _d(a['b2'])
    keep = torch.from_numpy(ops.keep_mask(seed, M * 128, rate)).reshape(M, 128) if rate > 0 else torch.ones(M, 128, dtype=torch.bool)
    z = x + torch.where(keep, y / (1.0 - rate), torch.zeros((), dtype=torch.float64))
    mean, var = z.mean(1, keepdim=True), z.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    res = (z, (z - mean) * rstd * _d(a['gamma']) + _d(a['beta']), torch.cat([mean, rstd], 1))
    return ((h,) if act == 'relu' else (h, u)) + res


# ----------------------------------------------------------------------------------------------------------------------------------
# the input families.  Cases are dicts of CPU fp32 tensors holding bf16 values (stats, gamma, biases: fp32)
# ----------------------------------------------------------------------------------------------------------------------------------
DOUT_SCALE = (1.0, 2.0, 0.5, 4.0, 0.25, 3.0, 1.5)


@functools.lru_cache(maxsize=2)
def _bwd_base(kind, M):
    g = torch.Generator().manual_seed(1000 * M + {'ffn': 0, 'act': 1, 'ao': 2}[kind])
    c = dict(kind=kind, M=M, seed=77 + M)
    c['z'] = _unlike(M, g)
    c['stats'] = stats_of(c['z'])
    c['gamma'] = 1.0 + 0.1 * torch.randn(128, generator=g)
    c['dout'] = bf16r(0.05 * torch.tensor(DOUT_SCALE)[torch.arange(M) % 7][:, None] * torch.randn(M, 128, generator=g))
    if kind == 'ao':
        c['o'] = _unlike(M, g)
        c['wc'] = bf16r(torch.randn(128, 128, generator=g) * 0.09)
    else:
        c['x'] = _unlike(M, g)
    return c


@functools.lru_cache(maxsize=2)
def bwd_case(kind, M, F=100, act='gelu'):
    """Unlike rows for a backward kernel: x / z / o rows m_r + s_r randn, a dense dOut with a per-row scale of period 7, stats from
    the bf16 z.  The ReLU h is relu(s_r (randn + 1)) (84 % of the gates open); the GELU u is (m_r / s_r) / 2 + 1.5 randn with
    h = act(u).  Hidden column 0 is open (h > 0, u > 0) in every row of tile_edges, so that a one-row launch at F = 1 carries a dW1."""
    c = dict(_bwd_base(kind, M))
    if kind == 'ao':
        return c
    g = torch.Generator().manual_seed(3000 * M + F)
    m, s = row_params(M)
    Fp = (F + 7) // 8 * 8
    c.update(F=F, Fp=Fp, act=act)
    edges = torch.tensor(tile_edges(M, CAP_BWD))
    v = torch.randn(M, F, generator=g)
    h = torch.zeros(M, Fp)
    if kind == 'ffn':
        h[:, :F] = torch.relu(s[:, None] * (v + 1.0))
        h[edges, 0] = s[edges] * (v[edges, 0].abs() + 0.25)
    else:
        u = torch.zeros(M, Fp)
        u[:, :F] = 0.5 * (m / s)[:, None] + 1.5 * v
        u[edges, 0] = u[edges, 0].abs() + 0.25
        c['u'] = bf16r(u)
        h[:, :F] = act64(act, c['u'][:, :F].double()).float()
    c['h'] = bf16r(h)
    # the weights are drawn again until the share condition of the impulse family (share_condition below: a lost row must fail) holds
    # in every row of tile_edges at both dropout rates -- decided on the float64 reference alone.  (At F = 1 the hidden gradient of a
    # row is ONE 128-term dot product, and about one draw in ten cancels to under its own bound.)
    for _ in range(64):
        wc1, wc2 = torch.zeros(128, Fp), torch.zeros(Fp, 128)
        wc1[:, :F] = torch.randn(128, F, generator=g) * 0.09
        wc2[:F] = torch.randn(F, 128, generator=g) * 0.1
        c['wc1'], c['wc2'] = bf16r(wc1), bf16r(wc2)
        if all(min(share_condition(c, int(r), rate).values()) >= 0.5 for r in edges for rate in (0.1, 0.0)):
            return c
    raise AssertionError('no weights with the share condition in 64 draws: %s M = %d F = %d' % (kind, M, F))


@functools.lru_cache(maxsize=3)
def fwd_case(M, F):
    g = torch.Generator().manual_seed(2000 * M + F)
    Fp = (F + 7) // 8 * 8
    c = dict(M=M, F=F, Fp=Fp, seed=177 + M, x=_unlike(M, g))
    wt1, wt2, b1 = torch.zeros(Fp, 128), torch.zeros(128, Fp), torch.zeros(Fp)
    wt1[:F] = torch.randn(F, 128, generator=g) * 0.09
    wt2[:, :F] = torch.randn(128, F, generator=g) * 0.1
    b1[:F] = torch.randn(F, generator=g) * 0.1
    c['wt1'], c['wt2'], c['b1'] = bf16r(wt1), bf16r(wt2), b1
    c['b2'] = torch.randn(128, generator=g) * 0.1
    c['gamma'], c['beta'] = 1.0 + 0.1 * torch.randn(128, generator=g), 0.1 * torch.randn(128, generator=g)
    return c


# ----------------------------------------------------------------------------------------------------------------------------------
# backward: reference and bounds over a set of rows (every other row of dOut is zero and contributes an exact nothing)
# ----------------------------------------------------------------------------------------------------------------------------------
def bwd_ref(c, rows, rate):
    """-> {name: (ref, bound)}: the row-local outputs at `rows` ([len(rows), 128]) and the row sums over `rows`, float64.
    `rows`: LongTensor of rows carrying dOut (all rows: the dense family)."""
    kind, M = c['kind'], c['M']
    rows = torch.as_tensor(rows, dtype=torch.long)
    t = lambda n: c[n][rows].double()      # noqa: E731
    dout, z, st, gamma = t('dout'), t('z'), t('stats'), c['gamma'].double()
    keep = keep_rows(c['seed'], rows.numpy(), rate)
    ik = 1.0 / (1.0 - rate)
    xh, gv, dz, dy = _ln_bwd64(dout, z, st, gamma, keep, rate)
    rstd = st[:, 1:]
    A_dz = rstd * (gv.abs() + gv.abs().mean(1, keepdim=True) + xh.abs() * (gv * xh).abs().mean(1, keepdim=True))
    e_o = (128 + 8) * U_F32 * A_dz                          # the fp32 dz before any rounding
    e_dy = U * dy.abs() + keep * (ik * e_o)                 # the bf16 dy image
    LM = (M + 8) * U_F32
    out = {}

    def rowsum(name, left, val, e_val, n_extra=0):
        ref = left.T @ val
        out[name] = (ref, left.abs().T @ e_val + (LM + n_extra * U_F32) * (left.abs().T @ val.abs()) + U_F32 * ref.abs())

    def colsum(name, val, e_val, n_extra=0):
        ref = val.sum(0)
        out[name] = (ref, e_val.sum(0) + (LM + n_extra * U_F32) * val.abs().sum(0) + U_F32 * ref.abs())
    colsum('dgamma', dout * xh, torch.zeros_like(dout), n_extra=8)
    colsum('dbeta', dout, torch.zeros_like(dout))
    if kind == 'ao':
        o, wc = t('o'), c['wc'].double()
        d_o = dy @ wc.T
        out['dz'] = (dz, U * dz.abs() + e_o)
        out['d_o'] = (d_o, e_dy @ wc.abs().T + (128 + 8) * U_F32 * (dy.abs() @ wc.abs().T) + U * d_o.abs())
        rowsum('dW', o, dy, e_dy)
        colsum('db', dy, e_dy)
    else:
        F, Fp = c['F'], c['Fp']
        h, x = t('h')[:, :F], t('x')
        w1, w2 = c['wc1'].double()[:, :F], c['wc2'].double()[:F]
        pre = dy @ w2.T
        e_pre = e_dy @ w2.abs().T + (128 + 8) * U_F32 * (dy.abs() @ w2.abs().T)
        if kind == 'ffn':
            gate = (h > 0).double()
            dh = pre * gate
            e_dh = gate * (U * dh.abs() + e_pre)
        else:
            u = t('u')[:, :F]
            gate = act_grad64(c['act'], u)
            dh = pre * gate
            e_dh = gate.abs() * (U * pre.abs() + e_pre) + pre.abs() * act_grad_term(c['act'], u) + (U + 4 * U_F32) * dh.abs()
        dx = dh @ w1.T + dz
        e_dx = e_dh @ w1.abs().T + (U * dz.abs() + e_o) + (Fp + 8) * U_F32 * (dh.abs() @ w1.abs().T + dz.abs()) + U * dx.abs()
        out['dx'] = (dx, e_dx)
        rowsum('dW1', x, dh, e_dh)
        colsum('db1', dh, e_dh)
        rowsum('dW2', h, dy, e_dy)
        colsum('db2', dy, e_dy)
    return {n: (a, _finish(b)) for n, (a, b) in out.items()}


def share_condition(c, row, rate):
    """{row sum: share of its entries whose |reference| exceeds twice their own bound} in a launch with dOut in `row` alone"""
    ref = bwd_ref(c, [row], rate)
    return {n: float((ref[n][0].abs() > 2.0 * ref[n][1]).double().mean()) for n in ROW_SUMS[c['kind']]}


def _note(record, name, ratio):
    if record is not None:
        record[name] = max(record.get(name, 0.0), ratio)


def check_bwd(c, rows, rate, got, record=None, tag=''):
    """Every check of a backward launch whose dOut is non-zero in `rows` only.  got: {row-local name: [len(rows), 128] tensor at `rows`,
    row-sum name: tensor, 'nz': {row-local name: rows of the WHOLE output with any non-zero entry}}."""
    kind = c['kind']
    rows = torch.as_tensor(rows, dtype=torch.long)
    ref = bwd_ref(c, rows, rate)
    live = set(rows[(c['dout'][rows] != 0).any(1)].tolist())
    for n in ROW_LOCAL[kind]:
        extra = sorted(set(int(r) for r in got['nz'][n]) - live)
        assert not extra, '%s%s: non-zero in %d rows without dOut, first %s' % (tag, n, len(extra), extra[:8])
    for n in ROW_LOCAL[kind] + ROW_SUMS[kind]:
        _note(record, n, check(tag + n, got[n], ref[n][0], ref[n][1]))
    if len(rows) == 1:
        assert torch.equal(got['dbeta'].float().cpu(), c['dout'][rows[0]].float()), '%sdbeta of a one-row launch is not that row of dOut' % tag
    return ref


# ----------------------------------------------------------------------------------------------------------------------------------
# forward: reference and bounds (all rows)
# ----------------------------------------------------------------------------------------------------------------------------------
def fwd_ref(c, kind, rate, act='gelu'):
    """-> {name: (ref, bound)} for h [M, F], (u [M, F],) z, out [M, 128], stats [M, 2]"""
    M, F, Fp = c['M'], c['F'], c['Fp']
    x, wt1, wt2 = c['x'].double(), c['wt1'].double()[:F], c['wt2'].double()[:, :F]
    b1, b2, gamma, beta = c['b1'].double()[:F], c['b2'].double(), c['gamma'].double(), c['beta'].double()
    keep = keep_all(c['seed'], M, rate).double()
    ik = 1.0 / (1.0 - rate)
    out = {}
    s = x @ wt1.T
    e_s = (128 + 8) * U_F32 * (x.abs() @ wt1.abs().T)
    u = s + b1
    if kind == 'ffn':
        h = torch.relu(u)
        e_h = e_s + U_F32 * u.abs()                        # |relu(a) - relu(b)| <= |a - b|
        e_y2 = 0.0
    else:
        e_u = U * s.abs() + e_s + U_F32 * u.abs()          # bf16(sum) + b1 in fp32
        out['u'] = (u, e_u + U * u.abs())
        h = act64(act, u)
        e_h = act_grad64(act, u).abs() * e_u + 0.5 * e_u * e_u + act_term(act, u) + U_F32 * h.abs()
    b_h = e_h + U * h.abs()
    out['h'] = (h, b_h)
    acc = h @ wt2.T
    e_acc = b_h @ wt2.abs().T + (Fp + 8) * U_F32 * (h.abs() @ wt2.abs().T)
    y = acc + b2
    if kind == 'ffn':
        e_y = e_acc + U_F32 * y.abs()
    else:
        e_y = e_acc + U * acc.abs() + U * y.abs()          # bf16(bf16(sum) + b2)
    ky = keep * y * ik
    v = x + ky
    e_v = keep * ik * e_y + 2 * U_F32 * (x.abs() + ky.abs())
    out['z'] = (v, e_v + U * v.abs())
    mean = v.mean(1, keepdim=True)
    e_mean = e_v.mean(1, keepdim=True) + (128 + 8) * U_F32 * v.abs().mean(1, keepdim=True)
    dlt = v - mean
    e_d = e_v + e_mean + U_F32 * dlt.abs()
    var = (dlt * dlt).mean(1, keepdim=True)
    e_var = (2 * dlt.abs() * e_d + e_d * e_d).mean(1, keepdim=True) + (128 + 8) * U_F32 * var
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    e_rstd = 0.5 * rstd ** 3 * e_var + 4 * U_F32 * rstd
    o = dlt * rstd * gamma + beta
    e_o = (e_d * rstd + dlt.abs() * e_rstd) * gamma.abs() + 4 * U_F32 * ((dlt * rstd * gamma).abs() + beta.abs()) + U * o.abs()
    out['out'] = (o, e_o)
    out['stats'] = (torch.cat([mean, rstd], 1), torch.cat([e_mean + U_F32 * mean.abs(), e_rstd], 1))
    return {n: (a, _finish(b)) for n, (a, b) in out.items()}


def check_fwd(ref, got, record=None, tag=''):
    for n in ref:
        _note(record, n, check(tag + n, got[n], ref[n][0], ref[n][1]))


# ----------------------------------------------------------------------------------------------------------------------------------
# CPU emulations of the kernels' rounding steps (fp32 arithmetic, bf16 where the source rounds), with the launch geometry, and the
# wrong variants tests/test_fused_rows_cpu.py must see rejected
# ----------------------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    'last_row_left_out': 'row M - 1 is missing from every row sum',
    'tile_G_twice': 'the rows of tile G (the second tile of workgroup 0) enter the row sums twice',
    'odd_last_row_stats': 'an odd M: row M - 1 takes the first half of its statistics window, row M - 2',
    'stats_halves_swapped': 'an even row whose window lies inside the tensor takes the second half, row r + 1',
    'keep_shifted': 'row r is masked with the keep bits of row r + 1',
    'past_M_into_dbeta': 'the rows of the last tile past M add the row they read, M - 1, into dbeta',
    'padded_hidden_columns': 'the hidden columns F .. Fp - 1 carry a copy of column F - 1 that is folded into db1 / dW1 (F < Fp only)',
    'fwd_stats_row_xor_1': 'the forward writes the statistics of row r to row r ^ 1',
    'tile_4G_previous_occupant': 'the fifth tile of workgroup 0 reads the ring stage before its DMA landed: the rows of tile 0',
}


def _stage_source(rows, M, cap, mutant):
    """the row whose ring-stage operands (h | x | u, o, the forward's x) a row reads: itself, or with the 4G mutant the same row of
    the stage's previous occupant, tile 0 of workgroup 0"""
    G = min(-(-M // TILE), cap)
    src = rows.clone()
    if mutant == 'tile_4G_previous_occupant':
        hit = (rows // TILE) == 4 * G
        src[hit] = rows[hit] - TILE * 4 * G
    return src


def emulate_bwd(c, rows, rate, mutant=None):
    """What a backward launch with dOut in `rows` alone returns, in the layout check_bwd takes."""
    kind, M = c['kind'], c['M']
    rows = torch.as_tensor(rows, dtype=torch.long)
    T = -(-M // TILE)
    G = min(T, CAP_BWD)
    f = lambda n, r: c[n][r].float()      # noqa: E731
    dout, z, gamma = f('dout', rows), f('z', rows), c['gamma'].float()
    srow = rows.clone()                                   # the row whose statistics a row uses
    if mutant == 'odd_last_row_stats' and M % 2 == 1:
        srow[rows == M - 1] = M - 2
    if mutant == 'stats_halves_swapped':
        hit = (rows % 2 == 0) & (rows + 1 < M)
        srow[hit] = rows[hit] + 1
    st = c['stats'][srow]
    mean, rstd = st[:, :1], st[:, 1:]
    keep = keep_rows(c['seed'], (rows + (1 if mutant == 'keep_shifted' else 0)).numpy(), rate)
    ik = np.float32(1.0) / (np.float32(1.0) - np.float32(rate)) if rate > 0 else np.float32(1.0)
    xh = (z - mean) * rstd
    gv = dout * gamma
    o = rstd * (gv - gv.sum(1, keepdim=True) * (1.0 / 128.0) - xh * ((gv * xh).sum(1, keepdim=True) * (1.0 / 128.0)))
    dz = bf16r(o)
    dy = bf16r(torch.where(keep, o * float(ik), torch.zeros(()))) if rate > 0 else dz
    w = torch.ones(len(rows))                             # how often a row enters the sums
    if mutant == 'last_row_left_out':
        w[rows == M - 1] = 0.0
    if mutant == 'tile_G_twice':
        w[(rows // TILE) == G] = 2.0
    w = w[:, None]
    src = _stage_source(rows, M, CAP_BWD, mutant)
    got = {'dgamma': (w * dout * xh).sum(0), 'dbeta': (w * dout).sum(0)}
    if mutant == 'past_M_into_dbeta' and bool((rows == M - 1).any()):
        got['dbeta'] = got['dbeta'] + (TILE * T - M) * c['dout'][M - 1].float()
    if kind == 'ao':
        wc, oo = c['wc'].float(), f('o', src)
        got['dz'], got['d_o'] = dz, bf16r(dy @ wc.T)
        got['dW'], got['db'] = oo.T @ (w * dy), (w * dy).sum(0)
    else:
        F, Fp = c['F'], c['Fp']
        h, x = f('h', src), f('x', src)
        pre = dy @ c['wc2'].float().T
        if kind == 'ffn':
            dh = torch.where(h > 0, bf16r(pre), torch.zeros(()))
        else:
            dh = bf16r(bf16r(pre) * act_grad32(c['act'], f('u', src)))
        got['dx'] = bf16r(dh @ c['wc1'].float().T + dz)
        dW1, db1 = x.T @ (w * dh), (w * dh).sum(0)
        if mutant == 'padded_hidden_columns' and Fp > F:  # the padded columns repeat column F - 1 and are folded into it
            dW1[:, F - 1] *= 1 + Fp - F
            db1[F - 1] *= 1 + Fp - F
        got['dW1'], got['db1'] = dW1[:, :F], db1[:F]
        got['dW2'], got['db2'] = (h.T @ (w * dy))[:F], (w * dy).sum(0)
    got['nz'] = {n: rows[(got[n] != 0).any(1)] for n in ROW_LOCAL[kind]}
    return got


def emulate_fwd(c, kind, rate, act='gelu', mutant=None):
    M, F, Fp = c['M'], c['F'], c['Fp']
    rows = torch.arange(M)
    x = c['x'].float()[_stage_source(rows, M, CAP_FWD, mutant)]
    s = x @ c['wt1'].float().T
    got = {}
    if kind == 'ffn':
        h = bf16r(torch.relu(s + c['b1'].float()))
    else:
        u = bf16r(s) + c['b1'].float()
        got['u'] = bf16r(u)[:, :F]
        h = bf16r(act32(act, u))
    got['h'] = h[:, :F]
    acc = h @ c['wt2'].float().T
    y = acc + c['b2'].float() if kind == 'ffn' else bf16r(bf16r(acc) + c['b2'].float())
    if rate > 0:
        ik = float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))
        y = torch.where(keep_all(c['seed'], M, rate), y * ik, torch.zeros(()))
    v = x + y
    mean = v.sum(1, keepdim=True) * (1.0 / 128.0)
    dlt = v - mean
    rstd = 1.0 / torch.sqrt((dlt * dlt).sum(1, keepdim=True) * (1.0 / 128.0) + np.float32(LN_EPS))
    got['z'], got['out'] = bf16r(v), bf16r(dlt * rstd * c['gamma'].float() + c['beta'].float())
    stats = torch.cat([mean, rstd], 1)
    if mutant == 'fwd_stats_row_xor_1':
        dst = rows ^ 1
        ok = dst < M
        sw = stats.clone()
        sw[dst[ok]] = stats[rows[ok]]
        stats = sw
    got['stats'] = stats
    return got
