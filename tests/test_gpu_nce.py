"""The in-batch contrastive loss on the device (NO REFERENCE ORACLE: an extension -- the float64 restatement and the derived bounds
are tests/nce_ref.py, written from the comment of include/b4c.h): both kernels (the bf16 matrix-core sweep, the fp32 row kernel)
on the committed cases, element by element; two launches bit for bit; a permutation of the rows; refused arguments that write
nothing; the autograd block against torch autograd over a dense float64 evaluation.

Gate of the element-wise comparisons: the derived bound of nce_ref.bounds times max(2, 2 x MEASURED_RATIO), where MEASURED_RATIO =
0.127 is the worst distance of the restatement's float32 mode from float64 in units of that bound on these very inputs (measured on
the CPU: tests/test_nce_cpu.py::test_measured_ratio_is_current) -- so the gate is 2 x the bound.  An element whose bound is 0
(ignored rows; batches where every live row's only key is its positive) must be exact."""
import functools

import numpy as np
import pytest
import torch

import nce_ref as nr

pytestmark = pytest.mark.gpu

GATE = nr.gate_factor()
SENTINEL = -12288.0          # (a bf16 value: the dz buffer holds it too)
DTYPES = [pytest.param(False, id='f32'), pytest.param(True, id='bf16')]


@pytest.fixture(scope='module')
def ops():
    from bert4clickpath_amd import ops as o
    return o


def _check(name, got, ref, bound):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64) * GATE
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    assert np.isfinite(got).all(), '%s: non-finite values' % name
    err = np.abs(got - ref)
    bad = err > bound
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print('%s: worst |err| / gate = %.3f' % (name, ratio))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError('%s: %d of %d elements outside their gate (worst |err| / gate = %.3g); first at %s: got %.9g, ref %.9g, gate '
                             '%.3g' % (name, int(bad.sum()), bad.size, ratio, i, got[i], ref[i], bound[i]))


@functools.lru_cache(maxsize=None)
def _reference(case, bf16):
    """inputs, float64 restatement and bounds of one case (computed once, never written to)"""
    N, K, pad, pattern, gkind, sim, temp = case
    zf, pos, group = nr.inputs(case, bf16)
    live = nr.structure(pos, group, N)[0]
    gscale = float(np.float32(0.7 / max(int(live.sum()), 1)))                # an upstream gradient of 0.7 folded in
    ref = nr.restate(zf[:, :K], pos, group, nr.inv_temp(temp), sim == 'cos', gscale=gscale)
    bd = nr.bounds(zf[:, :K], ref, nr.inv_temp(temp), sim == 'cos', bf16=bf16)
    return zf, pos, group, gscale, ref, bd


def _device(case, bf16, perm=None):
    """-> z [N, K] view of the [N, ld] device buffer (NaN behind K), pos, group, gscale on the device"""
    N, K = case[0], case[1]
    zf, pos, group, gscale, _, _ = _reference(case, bf16)
    if perm is not None:          # row perm[i] of the case becomes row i
        inv = np.empty(N, np.int64)
        inv[perm] = np.arange(N)
        zf = zf[perm]
        pos = np.where((pos >= 0) & (pos < N), inv[np.clip(pos, 0, N - 1)], pos)[perm].astype(np.int32)
        group = None if group is None else group[perm]
    z = torch.from_numpy(np.ascontiguousarray(zf)).cuda()
    z = (z.bfloat16() if bf16 else z)[:, :K]
    return (z, torch.from_numpy(pos).cuda(), None if group is None else torch.from_numpy(group).cuda(),
            torch.tensor([gscale], dtype=torch.float32, device='cuda'))


@pytest.mark.parametrize('bf16', DTYPES)
@pytest.mark.parametrize('case', nr.CASES, ids=nr.case_id)
def test_kernels_against_float64(ops, case, bf16):
    """lse, item_loss, rnorm and dz of every committed case inside the gate; a second launch gives the same bits"""
    N, K, pad, pattern, gkind, sim, temp = case
    _, _, _, _, ref, bd = _reference(case, bf16)
    z, pos, group, gscale = _device(case, bf16)
    assert z.stride(0) == K + pad
    item, lse, rnorm = ops.nce_fwd(z, pos, group, temp, sim)
    dz = ops.nce_bwd(z, pos, group, temp, sim, rnorm, lse, gscale)
    item2, lse2, rnorm2 = ops.nce_fwd(z, pos, group, temp, sim)
    dz2 = ops.nce_bwd(z, pos, group, temp, sim, rnorm2, lse2, gscale)
    torch.cuda.synchronize()
    assert torch.equal(item, item2) and torch.equal(lse, lse2) and torch.equal(dz, dz2)
    if sim == 'cos':
        assert torch.equal(rnorm, rnorm2)
        _check('rnorm', rnorm.cpu().numpy(), ref['rn'], np.abs(ref['rn']) * nr.gamma(K + 4))
    else:
        assert rnorm is None
    _check('lse', lse.cpu().numpy(), ref['lse'], bd['lse'])
    _check('item_loss', item.cpu().numpy(), ref['item'], bd['item'])
    assert dz.dtype == z.dtype and dz.shape == (N, K)
    _check('dz', dz.float().cpu().numpy(), ref['dz'], bd['dz'])
    dead = ~ref['live']
    assert not item.cpu().numpy()[dead].any() and not lse.cpu().numpy()[dead].any()


PERM_CASES = [nr.CASES[2], nr.CASES[5], nr.CASES[10], nr.CASES[12], nr.CASES[16]]


@pytest.mark.parametrize('bf16', DTYPES)
@pytest.mark.parametrize('case', PERM_CASES, ids=nr.case_id)
def test_a_permutation_of_the_rows_permutes_the_losses(ops, case, bf16):
    """rows shuffled across the tiles, pos and group remapped: every row's loss is its own row's of the restatement, inside the gate"""
    N, K, pad, pattern, gkind, sim, temp = case
    _, _, _, _, ref, bd = _reference(case, bf16)
    perm = np.random.default_rng(5 + N).permutation(N)
    z, pos, group, gscale = _device(case, bf16, perm)
    item, lse, rnorm = ops.nce_fwd(z, pos, group, temp, sim)
    dz = ops.nce_bwd(z, pos, group, temp, sim, rnorm, lse, gscale)
    _check('item_loss (permuted)', item.cpu().numpy(), ref['item'][perm], bd['item'][perm])
    _check('lse (permuted)', lse.cpu().numpy(), ref['lse'][perm], bd['lse'][perm])
    _check('dz (permuted)', dz.float().cpu().numpy(), ref['dz'][perm], bd['dz'][perm])


@pytest.mark.parametrize('bf16', DTYPES)
def test_refused_arguments_write_nothing(bf16):
    """B4C_EINVAL with real device pointers: the outputs keep their sentinel"""
    from bert4clickpath_amd import _lib as L
    lib = L.lib()
    N, K = 130, 64
    dt = torch.bfloat16 if bf16 else torch.float32
    z = torch.randn(N, K + 8, device='cuda').to(dt)
    pos = torch.arange(N, dtype=torch.int32, device='cuda').roll(1)
    outs = [torch.full((N,), SENTINEL, device='cuda') for _ in range(4)]
    rnorm, lse, item, gs = outs
    dz = torch.full((N, K + 8), SENTINEL, device='cuda').to(dt)
    st = torch.cuda.current_stream().cuda_stream
    code = L.BF16 if bf16 else L.F32
    p = lambda t: t.data_ptr()      # noqa: E731

    def fwd(ld=K + 8, n=N, k=K, d=code, it=1.0, fl=0, zp=None, rn=p(rnorm)):
        return lib.b4c_nce_fwd(p(z) if zp is None else zp, ld, n, k, d, p(pos), None, it, fl, rn, p(lse), p(item), st)

    def bwd(ld=K + 8, ldd=K + 8, n=N, k=K, d=code, it=1.0, fl=0, rn=p(rnorm)):
        return lib.b4c_nce_bwd(p(z), ld, n, k, d, p(pos), None, it, fl, rn, p(lse), p(gs), p(dz), ldd, st)

    bad = [fwd(k=60), fwd(k=136), fwd(d=7), fwd(it=0.0), fwd(it=float('nan')), fwd(fl=2), fwd(fl=1, rn=None), fwd(n=1 << 24),
           fwd(ld=K - 8), fwd(ld=K + 2), fwd(zp=p(z) + 4),
           bwd(k=60), bwd(d=7), bwd(it=-1.0), bwd(fl=4), bwd(fl=1, rn=None), bwd(n=1 << 24), bwd(ldd=K - 8), bwd(ldd=K + 1), bwd(ld=K + 2)]
    torch.cuda.synchronize()
    assert all(rc == L._C['B4C_EINVAL'] for rc in bad), bad
    for t in outs + [dz]:
        assert bool((t.float() == SENTINEL).all())


GRAD_CASES = [nr.CASES[2], nr.CASES[4], nr.CASES[7], nr.CASES[11], nr.CASES[13]]


@pytest.mark.parametrize('bf16', DTYPES)
@pytest.mark.parametrize('case', GRAD_CASES, ids=nr.case_id)
def test_autograd_block_against_torch_autograd(ops, case, bf16):
    """ops.InfoNCEFn: the mean over the live rows and its gradient by z (an upstream factor of 0.7 folded into gscale on the device)
    against torch autograd over the dense float64 evaluation of the definition (nce_ref.dense_loss)"""
    N, K, pad, pattern, gkind, sim, temp = case
    zf, pos_np, group_np, gscale, ref, bd = _reference(case, bf16)
    z, pos, group, _ = _device(case, bf16)
    z = z.contiguous().requires_grad_(True)
    loss = ops.InfoNCEFn.apply(z, pos, group, temp, sim)
    (loss * 0.7).backward()
    z64 = torch.tensor(zf[:, :K], dtype=torch.float64, requires_grad=True)
    want = nr.dense_loss(z64, pos_np, group_np, nr.inv_temp(temp), sim == 'cos')
    (want * (gscale * max(int(ref['live'].sum()), 1))).backward()
    nlive = max(int(ref['live'].sum()), 1)
    d_loss = (bd['item'].sum() + nr.gamma(N + 2) * np.abs(ref['item']).sum()) / nlive + 4 * nr.U_F32 * abs(float(want.detach()))
    _check('loss', np.array([float(loss.detach())]), np.array([float(want.detach())]), np.array([d_loss]))
    assert z.grad.dtype == z.dtype
    _check('dz', z.grad.float().cpu().numpy(), z64.grad.numpy(), bd['dz'])
