"""The two kernels of csrc/pre_ln.hip, the backward of a pre-LN encoder half's input norm.

b4c_layernorm_bwd_add: dx = res + LNbwd(dout; x, stats, gamma), dgamma / dbeta through the workspace in a fixed order.

Exact facts (no tolerance): dout == 0 gives dx == res bit for bit and leaves dgamma / dbeta as they were; res == 0 gives the bits of
b4c_layernorm_bwd(gate = NULL) in dx, dgamma and dbeta; two launches give the same bits; nothing is written around dx.
Otherwise every element against float64 under the derived bound of tests/pre_ln_bounds.py (a ratio above 1 fails).


b4c_gemm_nt_ln_bwd_add: the same with dout = bf16(A . Bt^T) formed on the matrix cores and never stored.  Every element of dx,
dgamma and dbeta against float64 under the derived bound (the accumulator's bf16 rounding counted), bit-repeatable, canaries around dx,
and against the composed pair (b4c_gemm_nt with bf16 output, then b4c_layernorm_bwd_add) under the same bound.

Worst |error| / bound per route, as measured on the MI355X (printed by the tests; RATIOS below):
    b4c_layernorm_bwd_add   fp32  dx 0.157  dgamma 0.437  dbeta 0.322        bf16  dx 0.980  dgamma 0.450  dbeta 0.001
    b4c_gemm_nt_ln_bwd_add  dx 0.811  dgamma 0.936  dbeta 0.936  (the composed pair: the same three figures)
    b4c_gemm_nt_ln_bwd_add against the pair  dx 0.113  dgamma 0.000  dbeta 0.000; bit-identical in 16 of the 80 shapes"""
import pytest
import torch

import pre_ln_bounds as pb
import pre_ln_ref as plr

pytestmark = pytest.mark.gpu

# the worst |error| / bound the MI355X run printed, per route and output (bf16 dx: the store's own rounding, half an ulp, is nearly
# the whole bound; the matrix-core kernel's dgamma / dbeta peak at M = 1, where the bf16 rounding of dn is nearly the whole bound)
RATIOS = {'b4c_layernorm_bwd_add fp32': {'dx': 0.157, 'dgamma': 0.437, 'dbeta': 0.322},
          'b4c_layernorm_bwd_add bf16': {'dx': 0.980, 'dgamma': 0.450, 'dbeta': 0.001},
          'b4c_gemm_nt_ln_bwd_add': {'dx': 0.811, 'dgamma': 0.936, 'dbeta': 0.936},
          'b4c_gemm_nt + b4c_layernorm_bwd_add (the pair)': {'dx': 0.811, 'dgamma': 0.936, 'dbeta': 0.936},
          'b4c_gemm_nt_ln_bwd_add against the pair': {'dx': 0.113, 'dgamma': 0.0, 'dbeta': 0.0, 'bit-identical shapes': '16 of 80'}}

ROWS = [1, 5, 257, 4099]            # one row; a partial row group; more than one workgroup at every d; the grid-stride loop at d = 1024
DS = [8, 64, 128, 136, 256, 1024]   # one lane per row; 8 and 16 lanes; a width that is no power of two; 32 lanes; two passes of 64
DT = [torch.float32, torch.bfloat16]
GUARD = 3                            # canary rows around dx


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops as o
    return o


_cases = {}


def _case(ops, rows, d, dtype):
    """the operands of one shape on the device (made once): x, dout, gamma, the stats b4c_layernorm_fwd saved, res as a [rows, d] view
    of a wider buffer (pitch d + 8), and the float64 reference with its bounds for zero sinks"""
    key = (rows, d, dtype)
    if key not in _cases:
        g = torch.Generator().manual_seed(rows * 1031 + d)
        x = (torch.randn(rows, d, generator=g) * 1.5 + 0.25).to(dtype).cuda()
        dout = torch.randn(rows, d, generator=g).to(dtype).cuda()
        gamma = (1 + 0.1 * torch.randn(d, generator=g)).cuda()
        beta = torch.zeros(d).cuda()
        wide = torch.randn(rows, d + 8, generator=g).to(dtype).cuda()
        res = wide[:, :d]
        assert res.stride(0) == d + 8
        _, stats = ops.layernorm_fwd(x, gamma, beta)
        ref = pb.ln_bwd_add(dout, x, stats[:, 0], stats[:, 1], gamma, res, dtype)
        _cases[key] = dict(x=x, dout=dout, gamma=gamma, res=res, stats=stats, ref=ref)
    return _cases[key]


def _launch(ops, c, dout=None, res=None, sinks=None):
    """one launch into a dx with canary rows around it -> (dx, dgamma, dbeta); the canaries are checked here"""
    x = c['x']
    rows, d = x.shape
    buf = torch.full((rows + 2 * GUARD, d), 777.0, dtype=x.dtype, device='cuda')
    dx = buf[GUARD:GUARD + rows]
    dg, db = sinks if sinks is not None else (torch.zeros(d, device='cuda'), torch.zeros(d, device='cuda'))
    ops.layernorm_bwd_add(c['dout'] if dout is None else dout, x, c['stats'], c['gamma'], c['res'] if res is None else res,
                          into=(dg, db), dx=dx)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 777.0).all()) and bool((buf[GUARD + rows:] == 777.0).all()), 'wrote outside dx'
    return dx, dg, db


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('d', DS)
@pytest.mark.parametrize('rows', ROWS)
def test_row_kernel_exact_facts(ops, rows, d, dtype):
    c = _case(ops, rows, d, dtype)
    # dout == 0: dx is res, the sinks keep their bits
    g = torch.Generator().manual_seed(7)
    s0 = (torch.randn(d, generator=g).cuda(), torch.randn(d, generator=g).cuda())
    sinks = (s0[0].clone(), s0[1].clone())
    dx, dg, db = _launch(ops, c, dout=torch.zeros_like(c['dout']), sinks=sinks)
    assert torch.equal(_bits(dx), _bits(c['res'])), 'dout == 0: dx != res'
    assert torch.equal(_bits(dg), _bits(s0[0])) and torch.equal(_bits(db), _bits(s0[1])), 'dout == 0: the sinks moved'
    # res == 0: b4c_layernorm_bwd
    zero = torch.zeros(rows, d + 8, dtype=dtype, device='cuda')[:, :d]
    dx, dg, db = _launch(ops, c, res=zero, sinks=(s0[0].clone(), s0[1].clone()))
    wdx, wdg, wdb = ops.layernorm_bwd(c['dout'], c['x'], c['stats'], c['gamma'], into=(s0[0].clone(), s0[1].clone()))
    assert torch.equal(_bits(dx), _bits(wdx)), 'res == 0: dx differs from b4c_layernorm_bwd'
    assert torch.equal(_bits(dg), _bits(wdg)) and torch.equal(_bits(db), _bits(wdb)), 'res == 0: dgamma / dbeta differ'
    # two launches: the same bits
    a, b = _launch(ops, c), _launch(ops, c)
    for u, v in zip(a, b):
        assert torch.equal(_bits(u), _bits(v)), 'two launches differ'


_worst = {}


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('d', DS)
@pytest.mark.parametrize('rows', ROWS)
def test_row_kernel_matches_float64_per_element(ops, rows, d, dtype):
    c = _case(ops, rows, d, dtype)
    dx, dg, db = _launch(ops, c)
    route = _worst.setdefault('bf16' if dtype == torch.bfloat16 else 'fp32', {})
    for name, got in (('dx', dx), ('dgamma', dg), ('dbeta', db)):
        ref, bound = c['ref'][name]
        ratio = pb.check('%s rows %d d %d %s' % (name, rows, d, dtype), got, ref, bound)
        route[name] = max(route.get(name, 0.0), ratio)
        print('%s rows %d d %d %s: worst |err| / bound %.3f' % (name, rows, d, dtype, ratio))
    print('worst so far', {r: {k: round(v, 3) for k, v in w.items()} for r, w in _worst.items()})


@pytest.mark.parametrize('dtype', DT)
def test_row_kernel_adds_into_sinks_that_hold_something(ops, dtype):
    rows, d = 257, 136
    c = _case(ops, rows, d, dtype)
    g = torch.Generator().manual_seed(11)
    s0 = (torch.randn(d, generator=g).cuda() * 3, torch.randn(d, generator=g).cuda() * 3)
    ref = pb.ln_bwd_add(c['dout'], c['x'], c['stats'][:, 0], c['stats'][:, 1], c['gamma'], c['res'], dtype, s0[0], s0[1])
    dx, dg, db = _launch(ops, c, sinks=(s0[0].clone(), s0[1].clone()))
    for name, got in (('dx', dx), ('dgamma', dg), ('dbeta', db)):
        pb.check(name, got, *ref[name])
    # and the closed form is the autograd of the LayerNorm it inverts (float64 stats against the kernel's fp32 ones: 1e-5)
    adx, _, _ = plr.ln_bwd_add_autograd(c['dout'].cpu(), c['x'].cpu(), c['gamma'].cpu(), c['res'].cpu())
    assert float((adx - ref['dx'][0]).abs().max()) < 1e-4


def test_wrapper_refuses_what_the_kernel_cannot_take(ops):
    from bert4clickpath_amd._lib import B4CError
    c = _case(ops, 5, 64, torch.float32)
    with pytest.raises(B4CError, match='res'):
        ops.layernorm_bwd_add(c['dout'], c['x'], c['stats'], c['gamma'], c['res'].to(torch.bfloat16))
    with pytest.raises(B4CError, match='res'):
        ops.layernorm_bwd_add(c['dout'], c['x'], c['stats'], c['gamma'], c['res'][:4])
    with pytest.raises(B4CError, match='stats'):
        ops.layernorm_bwd_add(c['dout'], c['x'], c['stats'][:4], c['gamma'], c['res'])
    small = torch.empty(16, dtype=torch.float32, device='cuda')
    with pytest.raises(B4CError, match='workspace'):
        ops.layernorm_bwd_add(c['dout'], c['x'], c['stats'], c['gamma'], c['res'], workspace=small)


# ---- b4c_gemm_nt_ln_bwd_add ------------------------------------------------------------------------------------------------------------
MS = [1, 63, 64, 65, 300]           # one row; one below, on and one above the 64-row tile; several tiles with a partial last one
NS = [64, 128, 136, 256]            # one wave's columns; two; a width that is no multiple of 32; all four
KS = [64, 104, 384, 768]            # one K stage; a partial second one (the padded dff of the reference); 3 d at d = 128 and at d = 256
_mm_cases = {}
_mm_worst = {}


def _mm_case(ops, M, N, K):
    """A [M, K] (pitch K + 8), Bt [N, K] (pitch K + 16), x [M, N], res [M, N] (pitch N + 8): bf16 on the device, made once, with the
    float64 reference, its bounds, and what the composed pair gives"""
    key = (M, N, K)
    if key not in _mm_cases:
        g = torch.Generator().manual_seed(M * 7919 + N * 31 + K)
        A = torch.randn(M, K + 8, generator=g).bfloat16().cuda()[:, :K]
        Bt = (torch.randn(N, K + 16, generator=g) / K ** 0.5).bfloat16().cuda()[:, :K]
        x = (torch.randn(M, N, generator=g) * 1.5 + 0.25).bfloat16().cuda()
        res = torch.randn(M, N + 8, generator=g).bfloat16().cuda()[:, :N]
        gamma = (1 + 0.1 * torch.randn(N, generator=g)).cuda()
        _, stats = ops.layernorm_fwd(x, gamma, torch.zeros(N).cuda())
        assert A.stride(0) == K + 8 and Bt.stride(0) == K + 16 and res.stride(0) == N + 8
        ref = pb.gemm_ln_bwd_add(A, Bt, x, stats[:, 0], stats[:, 1], gamma, res)
        dn = ops.gemm_nt(A, Bt, N)
        pair = ops.layernorm_bwd_add(dn, x, stats, gamma, res)
        torch.cuda.synchronize()
        _mm_cases[key] = dict(A=A, Bt=Bt, x=x, res=res, gamma=gamma, stats=stats, ref=ref, dn=dn, pair=pair)
    return _mm_cases[key]


def _mm_launch(ops, c):
    M, N = c['x'].shape
    buf = torch.full((M + 2 * GUARD, N), 777.0, dtype=torch.bfloat16, device='cuda')
    dx = buf[GUARD:GUARD + M]
    dg, db = torch.zeros(N, device='cuda'), torch.zeros(N, device='cuda')
    ops.gemm_nt_ln_bwd_add(c['A'], c['Bt'], c['x'], c['stats'], c['gamma'], c['res'], into=(dg, db), dx=dx)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 777.0).all()) and bool((buf[GUARD + M:] == 777.0).all()), 'wrote outside dx'
    return dx, dg, db


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('M', MS)
def test_matrix_core_kernel_matches_float64_the_pair_and_itself(ops, M, N, K):
    c = _mm_case(ops, M, N, K)
    got = _mm_launch(ops, c)
    again = _mm_launch(ops, c)
    for u, v in zip(got, again):
        assert torch.equal(_bits(u), _bits(v)), 'two launches differ'
    # the pair's GEMM is held to the bound of dn: the reference point of "the bf16 value b4c_gemm_nt would have stored"
    pb.check('dn of b4c_gemm_nt M %d N %d K %d' % (M, N, K), c['dn'], *c['ref']['dn'])
    identical = True
    for name, g, pr in zip(('dx', 'dgamma', 'dbeta'), got, c['pair']):
        ref, bound = c['ref'][name]
        ratio = pb.check('%s M %d N %d K %d' % (name, M, N, K), g, ref, bound)
        pair_ratio = pb.check('%s of the pair M %d N %d K %d' % (name, M, N, K), pr, ref, bound)
        diff = pb.check('%s against the pair M %d N %d K %d' % (name, M, N, K), g, pr.double().cpu(), bound)
        identical = identical and torch.equal(_bits(g), _bits(pr))
        for tag, v in ((name, ratio), (name + ' pair', pair_ratio), (name + ' vs pair', diff)):
            _mm_worst[tag] = max(_mm_worst.get(tag, 0.0), v)
    _mm_worst['bit-identical cases'] = _mm_worst.get('bit-identical cases', 0) + int(identical)
    _mm_worst['cases'] = _mm_worst.get('cases', 0) + 1
    print('worst so far (mfma)', {k: round(v, 3) for k, v in _mm_worst.items()})


def test_matrix_core_kernel_adds_into_sinks_and_walks_tiles_grid_stride(ops):
    """M = 70,000 rows: 1,094 row tiles on at most 1,024 workgroups -- some take two -- and sinks that hold something"""
    M, N, K = 70000, 128, 104
    g = torch.Generator().manual_seed(3)
    A = torch.randn(M, K, generator=g).bfloat16().cuda()
    Bt = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().cuda()
    x = (torch.randn(M, N, generator=g) * 1.5).bfloat16().cuda()
    res = torch.randn(M, N, generator=g).bfloat16().cuda()
    gamma = (1 + 0.1 * torch.randn(N, generator=g)).cuda()
    s0 = (torch.randn(N, generator=g).cuda(), torch.randn(N, generator=g).cuda())
    _, stats = ops.layernorm_fwd(x, gamma, torch.zeros(N).cuda())
    ref = pb.gemm_ln_bwd_add(A, Bt, x, stats[:, 0], stats[:, 1], gamma, res, s0[0], s0[1])
    dx, dg, db = ops.gemm_nt_ln_bwd_add(A, Bt, x, stats, gamma, res, into=(s0[0].clone(), s0[1].clone()))
    for name, got in (('dx', dx), ('dgamma', dg), ('dbeta', db)):
        print('%s M %d: worst |err| / bound %.3f' % (name, M, pb.check(name, got, *ref[name])))


def test_matrix_core_wrapper_refuses_what_the_kernel_cannot_take(ops):
    from bert4clickpath_amd._lib import B4CError
    c = _mm_case(ops, 63, 64, 64)
    with pytest.raises(B4CError, match='bf16'):
        ops.gemm_nt_ln_bwd_add(c['A'].float(), c['Bt'].float(), c['x'], c['stats'], c['gamma'], c['res'])
    with pytest.raises(B4CError, match='x and dx'):
        ops.gemm_nt_ln_bwd_add(c['A'], c['Bt'], c['x'][:60], c['stats'], c['gamma'], c['res'])
    with pytest.raises(B4CError, match='res'):
        ops.gemm_nt_ln_bwd_add(c['A'], c['Bt'], c['x'], c['stats'], c['gamma'], c['res'][:60])
    assert not ops.gemm_ln_bwd_supported(c['A'].float(), c['Bt'], 64) and not ops.gemm_ln_bwd_supported(c['A'], c['Bt'], 264)
