"""nt_cases.py on the CPU (no GPU): every committed case sits on the route and in the instantiation it is listed for and the route
classes stay populated; the exact cases tell the vec route's two roundings from a single one; the exact checker rejects the emulation
with one mistake built in (a wrong kernel cannot be run on purpose); the real-valued bound accepts the kernels' rounding steps emulated
in float32 and rejects a one-ulp perturbation; and b4c_gemm_nt_act refuses what it must, each with its own message."""
import math

import pytest
import torch

import local_bounds as lb
import nt_cases as nc

EXACT_IDS = [nc.case_id(c) for c in nc.EXACT]
REAL_IDS = [nc.case_id(c) for c in nc.REAL]


def test_case_ids_are_unique():
    ids = EXACT_IDS + REAL_IDS
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)


# ------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize('c', nc.EXACT + nc.REAL, ids=EXACT_IDS + REAL_IDS)
def test_every_case_takes_the_route_it_is_listed_for(c):
    assert nc.expected_route(c) == tuple(c['expect']), (nc.case_id(c), nc.route(c))


def test_route_classes_stay_populated():
    routes = [nc.route(c) for c in nc.EXACT]
    insts = {r['inst'] for r in routes if r['kernel'] != 'wide'}
    want = {(t, o, e, a) for t, o in (('f32', 'f32'), ('bf16', 'f32'), ('bf16', 'bf16')) for e in (False, True) for a in (False, True)}
    assert insts == want                                                     # all 12 instantiations of gemm_nt_kernel
    assert {r['kernel'] for r in routes} == {'wide', 'vec', 'scalar'}
    for kernel in ('vec', 'scalar'):
        assert {r['xcd_map'] for r in routes if r['kernel'] == kernel} == {0, 1}, kernel
    assert {r['tiles_per_chunk'] for r in routes if r['kernel'] == 'wide'} == {1, 2, 3}
    # the scalar epilogue with bf16 output and every epilogue operand, for each reason the host has to leave the vector one
    sc = [c for c in nc.EXACT if c['out'] == 'bf16' and nc.route(c)['kernel'] == 'scalar' and c['bias'] and c['gate'] and c['residual'] and c['pre']]
    assert len(sc) >= 8
    # the vec route with each single epilogue operand, and `pre` beside a gate / a residual
    vec = [c for c in nc.EXACT if nc.route(c)['kernel'] == 'vec' and (c['M'], c['N'], c['K']) == (129, 136, 72)]
    forms = {(c['bias'], c['act'], c['gate'], c['residual'], c['pre']) for c in vec}
    for f in ((False, 'none', 'relu', False, False), (False, 'none', None, True, False), (False, 'none', 'relu', False, True),
              (False, 'none', None, True, True), (True, 'relu', 'relu', True, True)):
        assert f in forms, f


def test_the_named_tile_maps():
    by = {(c['M'], c['N'], c['K'], c['bias_off']): nc.route(c) for c in nc.EXACT if c['dtype'] == 'bf16' and c['out'] == 'bf16'}
    r = by[(1025, 136, 8, 0)]
    assert r['xcd_map'] == 1 and r['blocks'] == 16 * 2                      # 9 M tiles rounded to 16: 14 workgroups return early
    assert by[(129, 1032, 72, 0)]['xcd_map'] == 0 and by[(129, 1032, 72, 0)]['blocks'] == 2 * 9
    r = by[(129, 2048, 8, 0)]
    assert (r['kernel'], r['mt'], r['chunks'], r['tiles_per_chunk']) == ('wide', 2, 16, 1)
    assert by[(129, 2048, 8, 1)]['kernel'] == 'scalar'                        # the misaligned bias
    r = by[(8321, 5128, 104, 0)]
    assert (r['mt'], math.ceil(5128 / 128), r['chunks'], r['tiles_per_chunk']) == (66, 41, 21, 2) and 41 - 20 * 2 == 1 and 5128 % 128 == 8
    r = by[(12673, 6664, 8, 0)]
    assert (r['mt'], math.ceil(6664 / 128), r['chunks'], r['tiles_per_chunk']) == (100, 53, 18, 3) and 53 - 17 * 3 == 2


def test_wide_cases_sit_on_the_row_pitch_of_the_ops_module():
    from bert4clickpath_amd import ops
    wide = [c for c in nc.EXACT if nc.route(c)['kernel'] == 'wide']
    assert len(wide) == 3
    for c in wide:
        assert c['ldc'] == ops.row_pitch(c['N']) and c['bias']
    assert sum(c['ldc'] > c['N'] for c in wide) == 2


# ------------------------------------------------------------------------------------------ inputs, witness
@pytest.mark.parametrize('c', nc.EXACT, ids=EXACT_IDS)
def test_exact_inputs_and_witness(c):
    """The inputs are what the docstring says (integers, half-integer bias, -0.0 among the gates, NaN around every view, partial sums
    below 2^24), and the two rounding orders of the table part on >= 1 % of the elements a ReLU or a closed gate left alone wherever a
    bias or a residual stands between the roundings -- and nowhere else."""
    inp = nc.inputs(c)
    M, N, K = c['M'], c['N'], c['K']
    a, bt = nc.view(c, 'A', inp['A']).double(), nc.view(c, 'Bt', inp['Bt']).double()
    r = nc.operand_range(K)
    assert float(a.abs().max()) <= r and float(bt[:N].abs().max()) <= r and bool((a == a.round()).all())
    assert bool(torch.isnan(bt[N:]).all()) and (c['bt_rows'] == N or bt[N:].numel() > 0)
    peak = float((a.abs() @ bt[:N].abs().T).max()) + 2.5 + 64
    assert peak < 2.0 ** 24 and peak < abs(nc.CANARY)
    for name in ('A', 'Bt', 'gate', 'res'):
        if inp[name] is None:
            continue
        buf = inp[name].float()
        n_view = nc.view(c, name, inp[name]).numel()
        assert int(torch.isnan(buf).sum()) == buf.numel() - n_view + (bt[N:].numel() if name == 'Bt' else 0), name
    if c['bias']:
        b = nc.view(c, 'bias', inp['bias'])
        assert bool((b * 2 == (b * 2).round()).all()) and float(b.abs().max()) <= 2.5
        assert int(torch.isnan(inp['bias']).sum()) == inp['bias'].numel() - N
    if c['gate'] is not None:
        g = nc.view(c, 'gate', inp['gate']).float()
        assert float(g.abs().max()) <= 2
        if g.numel() >= 64:
            zeros = g == 0
            assert bool((zeros & torch.signbit(g)).any()) and bool((zeros & ~torch.signbit(g)).any()) and bool((g > 0).any()) and bool((g < 0).any())
    if c['out'] != 'bf16':
        return
    two, one = nc.emulate(c, inp, 0, nc.BLOCK_ROWS, kind='double'), nc.emulate(c, inp, 0, nc.BLOCK_ROWS, kind='single')
    if not (c['bias'] or c['residual']):
        assert torch.equal(nc.bits(two['C']), nc.bits(one['C']))                  # rounding twice finds a bf16 number
        return
    differ = nc.bits(two['C']) != nc.bits(one['C'])
    rows = two['C'].shape[0]
    live = torch.ones(rows, N, dtype=torch.bool)
    if c['gate'] is not None:
        live &= nc.view(c, 'gate', inp['gate'])[:rows].float() > 0
    if c['act'] == 'relu':
        pre = nc.emulate(dict(c, pre=True), inp, 0, nc.BLOCK_ROWS, kind='single')['pre'].float()
        live &= pre > 0
    share = float(differ[live].float().mean())
    print('%s: the two rounding orders differ on %.2f %% of the %d live elements' % (nc.case_id(c), 100 * share, int(live.sum())))
    assert share >= 0.01
    if c['pre'] and c['bias']:
        assert float((nc.bits(two['pre']) != nc.bits(one['pre'])).float().mean()) >= 0.01


# ------------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize('c', nc.EXACT, ids=EXACT_IDS)
def test_exact_checker_accepts_the_emulation_and_rejects_every_mutant(c):
    inp = nc.inputs(c)
    nc.check_exact(c, inp, nc.emulate_buffers(c, inp))
    tried = 0
    for wrong in nc.WRONG + nc.WRONG_BUFFER:
        if not nc.applies(c, wrong):
            continue
        tried += 1
        with pytest.raises(AssertionError):
            nc.check_exact(c, inp, nc.emulate_buffers(c, inp, wrong=wrong))
    assert tried >= 1


def test_every_mutant_is_tried_on_both_bf16_routes():
    for wrong in nc.WRONG + nc.WRONG_BUFFER:
        kernels = {nc.route(c)['kernel'] for c in nc.EXACT if c['out'] == 'bf16' and nc.applies(c, wrong)}
        assert {'vec', 'scalar'} <= kernels, (wrong, kernels)
    for wrong in ('rounding', 'row_from_next_tile', 'chunk_shifted', 'canary'):
        assert all(nc.applies(c, wrong) for c in nc.EXACT if nc.route(c)['kernel'] == 'wide'), wrong


# ------------------------------------------------------------------------------------------ the bound
def test_lipschitz_factors():
    assert abs(nc.lipschitz('gelu') - 1.128904) < 1e-6
    assert abs(nc.lipschitz('gelu_tanh') - 1.128993) < 1e-6
    u = torch.linspace(-8, 8, 200001, dtype=torch.float64)
    for name in ('gelu', 'gelu_tanh'):
        assert float(nc.gelu_grad64(name, u).abs().max()) <= nc.lipschitz(name)
        x = u.clone().requires_grad_(True)
        nc.gelu64(name, x).sum().backward()
        assert float((x.grad - nc.gelu_grad64(name, u)).abs().max()) < 1e-12            # act_gelu_grad's formula IS gelu'
    assert nc.EVAL == 2 * nc.EVAL_MEASURED


def _ulp_bf16(x):
    """the spacing of the bf16 numbers around x (x != 0)"""
    return 2.0 ** (torch.floor(torch.log2(x.abs().double())) - 7)


@pytest.mark.parametrize('c', nc.REAL, ids=REAL_IDS)
def test_bound_holds_for_the_emulated_roundings_and_is_tight(c):
    inp = nc.inputs(c)
    ref = nc.real_ref(c, inp)
    emu = nc.real_emulate(c, inp)
    ratio = lb.worst_ratio(emu['C'], ref['C'], ref['bound'])
    print('%s: emulation worst |err| / bound %.3f' % (nc.case_id(c), ratio))
    assert lb.accepts(emu['C'], ref['C'], ref['bound'])
    assert float(ref['v'].min()) < -2.5 and float(ref['v'].max()) > 2.5          # both tails of the GELU are in the case
    # one bf16 ulp on the largest 1 % of the outputs, all up or all down
    y = emu['C'].double()
    k = max(1, y.numel() // 100)
    top = torch.zeros(y.numel(), dtype=torch.bool)
    top[y.abs().reshape(-1).topk(k).indices] = True
    top = top.reshape(y.shape)
    for sign in (1.0, -1.0):
        moved = torch.where(top, y + sign * _ulp_bf16(y), y)
        assert not lb.accepts(moved, ref['C'], ref['bound']), sign
    # the n = 0 bound rejects the vec route's double rounding (and the n = 1 bound is not handed to the scalar route)
    if c['out'] == 'bf16':
        other = dict(c, ldc=c['N'] if c['ldc'] != c['N'] else c['N'] + 4)
        assert nc.rounding(other) != nc.rounding(c) and nc.real_ref(other, inp)['n'] == 1 - ref['n']


# ------------------------------------------------------------------------------------------ host refusals
FAKE = 4096          # a non-null, 16-byte aligned "pointer": every call below is refused before anything is launched or followed


def _act_call(L, M=8, N=8, K=8, lda=8, ldb=8, ldc=8, bias=None, act=0, gate=None, ldg=0, gate_act=1, res=None, ldr=0, pre=None, ldp=0,
              dtype=1, out_dtype=1):
    return L.b4c_gemm_nt_act(FAKE, lda, FAKE, ldb, FAKE, ldc, M, N, K, bias, act, gate, ldg, gate_act, res, ldr, pre, ldp, dtype, out_dtype, None)


@pytest.mark.parametrize('kw,message', [
    (dict(N=16, ldc=8), b'ldc 8 < N 16'),
    (dict(N=16, ldc=16, pre=FAKE, ldp=8), b'ldp 8 < N 16'),
    (dict(dtype=0, out_dtype=1), b'out_dtype 1'),
    (dict(act=4), b'act 4'),
    (dict(act=-1), b'act -1'),
    (dict(gate=FAKE, ldg=8, gate_act=0), b'gate_act 0'),
    (dict(gate=FAKE, ldg=8, gate_act=4), b'gate_act 4'),
    (dict(K=12, lda=16, ldb=16, dtype=1), b'K=12 lda=16 ldb=16 must be multiples of 8'),
    (dict(K=6, lda=8, ldb=8, dtype=0, out_dtype=0), b'K=6 lda=8 ldb=8 must be multiples of 4'),
    (dict(lda=1 << 22, dtype=1), b'2^30 bytes'),
    (dict(ldb=1 << 22, dtype=0, out_dtype=0), b'2^30 bytes'),
], ids=['ldc', 'ldp', 'bf16-out-of-f32', 'act', 'act-negative', 'gate_act-none', 'gate_act', 'K-bf16', 'K-f32', 'pitch-A', 'pitch-Bt'])
def test_host_refusals(kw, message):
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    rc = _act_call(L, **kw)
    err = L.b4c_last_error()
    assert rc != 0 and message in err and b'gemm_nt' in err, (rc, err)


def test_an_unknown_gate_act_without_a_gate_is_not_what_refuses():
    """gate_act is looked at only beside a gate (b4c_gemm_nt passes ACT_RELU always): without one the call gets past that check and
    is refused by the next thing wrong with it"""
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    rc = _act_call(L, gate_act=9, pre=FAKE, ldp=4)
    assert rc != 0 and b'ldp 4 < N 8' in L.b4c_last_error()
