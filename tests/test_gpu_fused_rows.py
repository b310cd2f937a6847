"""The five persistent kernels of the d_model = 128 encoder (b4c_ffn_fwd, b4c_ffn_bwd, b4c_attn_out_bwd, b4c_ffn_act_fwd,
b4c_ffn_act_bwd) row by row against float64, every element held to the bound tests/fused_rows_ref.py derives for it (no tensor-wide
scale), at row counts from the ABI's minimum up: grids of one and two workgroups, tiles whose prefetches all lie past the end, one-row
last tiles on both parities of the paired tile loop, the first re-use of a ring stage.

Impulse family (backward): dOut is zero except in the rows of fused_rows_ref.tile_edges, one launch per row and one with all of them.
Rows without dOut must come back as exact zeros, the row sums must be the float64 sum over the impulse rows alone, and dbeta of a
one-row launch is that row of dOut bit for bit: this is what says WHICH rows a workgroup owns.  Unlike-rows family (all five): every
row has a mean and a scale unlike those of its neighbours at every distance the kernels know (lane group, wave, tile, ring stage,
grid stride).  Pitched operands: the same bits with x / h / u / o as column slices of wider buffers.  b4c_gemm_dxdw: the integer-exact
check of tests/test_gpu_dxdw.py from one row up.

Worst |error| / bound per kernel and output on the MI355X (over every case of this file; n = bf16 roundings counted on the path, see
the table in fused_rows_ref.py; the bounds are derived, not tuned to these figures):

  kernel            family    worst |error| / bound
  ----------------  --------  ------------------------------------------------------------------------------------------------
  b4c_ffn_bwd       impulse   dx 0.819  dW1 0.293  db1 0.293  dW2 0.972  db2 0.972  dgamma 0.092  dbeta 0.000
  b4c_ffn_bwd       unlike    dx 0.939  dW1 0.092  db1 0.080  dW2 0.623  db2 0.404  dgamma 0.066  dbeta 0.006
  b4c_ffn_act_bwd   impulse   dx 0.777  dW1 0.391  db1 0.391  dW2 0.970  db2 0.970  dgamma 0.099  dbeta 0.004
  b4c_ffn_act_bwd   unlike    dx 0.955  dW1 0.141  db1 0.124  dW2 0.854  db2 0.464  dgamma 0.086  dbeta 0.000
  b4c_attn_out_bwd  impulse   dz 0.967  d_o 0.305  dW 0.965  db 0.965  dgamma 0.095  dbeta 0.000
  b4c_attn_out_bwd  unlike    dz 0.978  d_o 0.414  dW 0.517  db 0.433  dgamma 0.045  dbeta 0.000
  b4c_ffn_fwd       unlike    h 0.975  z 0.980  out 0.975  stats 0.462
  b4c_ffn_act_fwd   unlike    h 0.969  u 0.974  z 0.977  out 0.936  stats 0.179

An output stored in bf16 (or a one-row sum of one bf16 dy) sits near 1 whenever its own rounding is the whole bound: a value just under a
rounding boundary uses all of u |X|.  The row sums of the unlike-rows family are far below 1: their bounds are worst cases over M terms.
(`pytest -s` prints a RATIO line per case.)
"""
import pytest
import torch

import fused_rows_ref as fr

pytestmark = pytest.mark.gpu
KERNEL = {'ffn': 'b4c_ffn_bwd', 'act': 'b4c_ffn_act_bwd', 'ao': 'b4c_attn_out_bwd'}
FWD_KERNEL = {'ffn': 'b4c_ffn_fwd', 'act': 'b4c_ffn_act_fwd'}


@pytest.fixture(scope='module')
def ops():
    from bert4clickpath_amd import ops as o
    return o


def _dev(t, dt=torch.bfloat16):
    return t.to(dt).cuda().contiguous()


def _bwd_dev(c):
    d = {n: _dev(c[n]) for n in ('dout', 'z', 'x', 'h', 'u', 'o', 'wc', 'wc1', 'wc2') if n in c}
    d['stats'], d['gamma'] = c['stats'].cuda(), c['gamma'].cuda()
    return d


def _bwd_launch(ops, c, d, dout, rate, over=None):
    """one launch with fresh zeroed gradient outputs -> {name: device tensor}; over: operands that replace those of d"""
    kind = c['kind']
    a = dict(d, **(over or {}))
    z = lambda *s: torch.zeros(*s, device='cuda')      # noqa: E731
    if kind == 'ao':
        out = dict(dW=z(128, 128), db=z(128), dgamma=z(128), dbeta=z(128))
        out['dz'], out['d_o'] = ops.attn_out_bwd(dout, a['z'], a['stats'], a['gamma'], rate, c['seed'], a['o'], a['wc'], out['dW'], out['db'],
                                                 out['dgamma'], out['dbeta'])
        return out
    F = c['F']
    out = dict(dW1=z(128, F), db1=z(F), dW2=z(F, 128), db2=z(128), dgamma=z(128), dbeta=z(128))
    sinks = (out['dW1'], out['db1'], out['dW2'], out['db2'], out['dgamma'], out['dbeta'])
    if kind == 'ffn':
        out['dx'] = ops.ffn_bwd(dout, a['z'], a['stats'], a['gamma'], rate, c['seed'], a['h'], a['x'], a['wc2'], a['wc1'], F, *sinks)
    else:
        out['dx'] = ops.ffn_act_bwd(dout, a['z'], a['stats'], a['gamma'], rate, c['seed'], fr.ACT_CODE[c['act']], a['h'], a['u'], a['x'],
                                    a['wc2'], a['wc1'], F, *sinks)
    return out


def _bwd_got(kind, out, rows):
    """what check_bwd takes: the row-local outputs at `rows`, the rows of the WHOLE output with a non-zero entry (found on the device)"""
    idx = torch.as_tensor(rows, dtype=torch.long).cuda()
    got = {n: out[n].float().cpu() for n in fr.ROW_SUMS[kind]}
    got['nz'] = {}
    for n in fr.ROW_LOCAL[kind]:
        got[n] = out[n][idx].float().cpu()
        got['nz'][n] = (out[n] != 0).any(1).nonzero().reshape(-1).cpu()
    return got


def _report(kernel, case, rec):
    print('RATIO fused_rows %s %s %s' % (kernel, '-'.join(str(x) for x in case), ' '.join('%s=%.3f' % kv for kv in sorted(rec.items()))))


BWD_PARAMS = [(kind, M, F, rate) for kind in fr.BWD_KINDS for M, F, rate in fr.shapes('bwd', with_width=kind != 'ao')]


@pytest.mark.parametrize('kind,M,F,rate', BWD_PARAMS)
def test_impulse_rows_backward(ops, kind, M, F, rate):
    c = fr.bwd_case(kind, M, F)
    edges = fr.tile_edges(M, fr.CAP_BWD)
    for r in edges:       # the condition of the family, on the reference: a lost row could not pass
        share = fr.share_condition(c, r, rate)
        assert min(share.values()) >= 0.5, (r, share)
    d, rec = _bwd_dev(c), {}
    for rows in [[r] for r in edges] + [edges]:
        idx = torch.tensor(rows).cuda()
        dout = torch.zeros(M, 128, dtype=torch.bfloat16, device='cuda')
        dout[idx] = d['dout'][idx]
        out = _bwd_launch(ops, c, d, dout, rate)
        fr.check_bwd(c, rows, rate, _bwd_got(kind, out, rows), rec, tag='dOut in rows %s: ' % (rows if len(rows) == 1 else 'tile_edges'))
    _report(KERNEL[kind], ('impulse', M, F, rate), rec)


@pytest.mark.parametrize('kind,M,F,rate', [p for p in BWD_PARAMS if p[1] in fr.BWD_UNLIKE_M])
def test_unlike_rows_backward(ops, kind, M, F, rate):
    """Every row with statistics unlike its neighbours', a dense dOut: dx / dz / d_o element by element, the row sums against their
    element bounds.  Those worst-case row-sum bounds grow with M (M 2^-24 A on top of the roundings) and CANNOT see one lost row
    among thousands: which rows a workgroup owns is the impulse family's job, not this one's."""
    for act in (('gelu', 'gelu_tanh') if kind == 'act' and F == 100 and rate > 0 else ('gelu',)):
        c = fr.bwd_case(kind, M, F, act)
        d, rec, rows = _bwd_dev(c), {}, torch.arange(M)
        out = _bwd_launch(ops, c, d, d['dout'], rate)
        fr.check_bwd(c, rows, rate, _bwd_got(kind, out, rows), rec)
        _report(KERNEL[kind], ('unlike', M, F, rate, act), rec)


def _fwd_dev(c):
    d = {n: _dev(c[n]) for n in ('x', 'wt1', 'wt2')}
    d.update({n: c[n].cuda() for n in ('b1', 'b2', 'gamma', 'beta')})
    return d


def _fwd_launch(ops, c, d, kind, rate, act, save=True, x=None):
    x = d['x'] if x is None else x
    args = (x, d['wt1'], d['b1'], d['wt2'], d['b2'], d['gamma'], d['beta'], c['F'], c['Fp'])
    if kind == 'ffn':
        h, z, out, stats = ops.ffn_fwd(*args, rate, c['seed'], save=save)
        return dict(h=h, z=z, out=out, stats=stats)
    h, u, z, out, stats = ops.ffn_act_fwd(*args, fr.ACT_CODE[act], rate, c['seed'], save=save)
    return dict(h=h, u=u, z=z, out=out, stats=stats)


@pytest.mark.parametrize('kind', fr.FWD_KINDS)
@pytest.mark.parametrize('M,F,rate', fr.shapes('fwd'))
def test_rows_forward(ops, kind, M, F, rate):
    """unlike rows through the forward kernels at every row count of the matrix: h, (u,) z, out and stats element by element; the
    hidden columns F .. Fp - 1 are exact zeros; the inference form (save=False) returns the same out and h bits"""
    c = fr.fwd_case(M, F)
    d = _fwd_dev(c)
    for act in (('gelu', 'gelu_tanh') if kind == 'act' and F == 100 and rate > 0 and M in fr.FWD_UNLIKE_M else ('gelu',)):
        ref, rec = fr.fwd_ref(c, kind, rate, act), {}
        res = _fwd_launch(ops, c, d, kind, rate, act)
        got = {n: t.float().cpu() for n, t in res.items()}
        for n in ('h', 'u'):
            if n in got:
                assert not bool((got[n][:, F:] != 0).any()), '%s: non-zero in the padded hidden columns' % n
                got[n] = got[n][:, :F]
        fr.check_fwd(ref, got, rec)
        inf = _fwd_launch(ops, c, d, kind, rate, act, save=False)
        assert inf['z'] is None and inf['stats'] is None and inf.get('u') is None
        assert torch.equal(inf['out'], res['out']) and torch.equal(inf['h'], res['h'])
        _report(FWD_KERNEL[kind], ('unlike', M, F, rate, act), rec)


def _pitched(t, pitch, off=8):
    """t as a column slice (from column `off`: still 16-byte aligned) of a buffer of `pitch` columns whose other columns hold 1e4"""
    buf = torch.full((t.shape[0], pitch), 1e4, dtype=t.dtype, device=t.device)
    view = buf[:, off:off + t.shape[1]]
    view.copy_(t)
    assert view.stride(0) == pitch and not view.is_contiguous()
    return view


@pytest.mark.parametrize('kind', fr.BWD_KINDS)
def test_pitched_operands_backward(ops, kind):
    M, F, rate = 8193, 100, 0.1
    c = fr.bwd_case(kind, M, F)
    d = _bwd_dev(c)
    base = _bwd_launch(ops, c, d, d['dout'], rate)
    for pitches in ((136, 264), (264, 136)):
        over = {n: _pitched(d[n], p) for n, p in zip(('x', 'h', 'u', 'o'), pitches * 2) if n in d}
        got = _bwd_launch(ops, c, d, d['dout'], rate, over)
        for n in base:
            assert torch.equal(base[n], got[n]), (n, pitches)


@pytest.mark.parametrize('kind', fr.FWD_KINDS)
def test_pitched_operands_forward(ops, kind):
    M, F, rate = 16385, 100, 0.1
    c = fr.fwd_case(M, F)
    d = _fwd_dev(c)
    base = _fwd_launch(ops, c, d, kind, rate, 'gelu')
    for pitch in (136, 264):
        got = _fwd_launch(ops, c, d, kind, rate, 'gelu', x=_pitched(d['x'], pitch))
        for n in base:
            assert torch.equal(base[n], got[n]), (n, pitch)


@pytest.mark.parametrize('n_seg', [1, 3])
@pytest.mark.parametrize('M', [1, 2, 31, 33, 8193, 32769])
def test_fused_dense_backward_is_exact_on_integer_data_from_one_row_up(ops, M, n_seg):
    from test_gpu_dxdw import _case
    x, G, W, res = _case(M, n_seg, seed=M + n_seg)
    exact_dx = G.double() @ W.double().T
    exact_dw = (x.double().T @ G.double() + 1.0).cpu()
    exact_db = (G.double().sum(0) + 1.0).cpu()
    for r in (res, None):
        dWs = [torch.ones(128, 128, device='cuda') for _ in range(n_seg)]
        dbs = [torch.ones(128, device='cuda') for _ in range(n_seg)]
        dx = ops.gemm_dxdw(x, G, W, dWs, dbs, residual=r)
        want = (exact_dx + (r.double() if r is not None else 0.0)).float().bfloat16()      # (an integer < 2^24: one rounding, as the kernel's)
        wrong = (dx != want).any(1).nonzero().reshape(-1)
        assert wrong.numel() == 0, (wrong.numel(), wrong[:8].tolist())
        assert torch.equal(torch.cat(dWs, 1).double().cpu(), exact_dw)
        assert torch.equal(torch.cat(dbs).double().cpu(), exact_db)
