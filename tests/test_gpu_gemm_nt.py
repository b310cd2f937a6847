"""b4c_gemm_nt / b4c_gemm_nt_act on the cases of tests/nt_cases.py: the exact cases against the CPU emulation of each route's rounding
order, bit for bit, with the canaries around C and pre intact; both entry points bit-identical; the GELU forms against float64 inside
the element-wise bound of nt_cases.real_ref."""
import pytest
import torch

import local_bounds as lb
import nt_cases as nc

pytestmark = pytest.mark.gpu

EXACT_IDS = [nc.case_id(c) for c in nc.EXACT]
REAL_IDS = [nc.case_id(c) for c in nc.REAL]


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import _lib, ops
    return ops, _lib


def _upload(inp):
    return {k: (None if v is None else v.cuda()) for k, v in inp.items()}


def _c_buffer(ops, c):
    """the canary-filled flat buffer of C on the device; the wide cases take theirs from ops.empty_rows (the pitch the model uses)"""
    if nc.route(c)['kernel'] != 'wide':
        return nc.out_buffer(c, 'C').cuda()
    t = ops.empty_rows(c['M'] + nc.EXTRA_ROWS, c['N'], torch.bfloat16, 'cuda')
    assert t.stride(0) == c['ldc'] and c['c_off'] == 0
    base = t if t.is_contiguous() else t._base
    base.fill_(nc.CANARY)
    return base.view(-1)


def _run(gpu, c, dev, entry='act', act=None, use_gate=True, use_pre=True):
    """one launch into fresh canary buffers -> {'C': flat buffer, 'pre': flat buffer or None} (device)"""
    ops, L = gpu
    act = c['act'] if act is None else act
    gate = dev['gate'] if use_gate else None
    got = {'C': _c_buffer(ops, c), 'pre': nc.out_buffer(c, 'pre').cuda() if (c['pre'] and use_pre) else None}

    def p(name, buf):
        return None if buf is None else nc.view(c, name, buf).data_ptr()
    head = (p('A', dev['A']), c['lda'], p('Bt', dev['Bt']), c['ldb'], p('C', got['C']), c['ldc'], c['M'], c['N'], c['K'],
            p('bias', dev['bias']), nc.ACT_CODE[act], p('gate', gate), c['ldg'] if gate is not None else 0)
    res = (p('res', dev['res']), c['ldr'] if dev['res'] is not None else 0)
    types = (ops.dt_code(nc.DT[c['dtype']]), ops.dt_code(nc.DT[c['out']]), ops._st())
    if entry == 'act':
        gate_act = nc.ACT_CODE[c['gate'] or 'relu']
        rc = L.lib().b4c_gemm_nt_act(*head, gate_act, *res, p('pre', got['pre']), c['ldp'] if got['pre'] is not None else 0, *types)
    else:
        assert got['pre'] is None and (gate is None or c['gate'] == 'relu') and act in ('none', 'relu')
        rc = L.lib().b4c_gemm_nt(*head, *res, *types)
    L.check(rc, 'gemm_nt (%s)' % entry)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize('c', nc.EXACT, ids=EXACT_IDS)
def test_exact_cases_bit_for_bit(gpu, c):
    """C and pre equal the emulation of the case's route bit for bit (fp32 output: the float64 reference too), every canary element
    around them is unchanged; through b4c_gemm_nt the same launch stores the same bits."""
    assert (gpu[1].ACT_NONE, gpu[1].ACT_RELU, gpu[1].ACT_GELU, gpu[1].ACT_GELU_TANH) == tuple(nc.ACT_CODE[a] for a in ('none', 'relu', 'gelu', 'gelu_tanh'))
    inp = nc.inputs(c)
    dev = _upload(inp)
    got = _run(gpu, c, dev, 'act')
    nc.check_exact(c, inp, got)
    if not c['pre']:
        plain = _run(gpu, c, dev, 'plain')
        assert torch.equal(nc.bits(plain['C']), nc.bits(got['C'])), 'b4c_gemm_nt and b4c_gemm_nt_act differ'


@pytest.mark.parametrize('c', nc.REAL, ids=REAL_IDS)
def test_real_cases_inside_the_elementwise_bound(gpu, c):
    """The GELU forms against float64, every element inside its own bound; `pre` is what the plain launch of the same geometry stores
    (rounded to the input type where C is fp32), C is the same with and without `pre`, and the canaries hold."""
    inp = nc.inputs(c)
    dev = _upload(inp)
    ref = nc.real_ref(c, inp)
    got = _run(gpu, c, dev, 'act')
    for n in ('C', 'pre'):
        nc.check_canary(c, n, got[n])
    C = nc.view(c, 'C', got['C']).cpu()
    ratio = lb.worst_ratio(C, ref['C'], ref['bound'])
    print('%s: worst |err| / bound %.3f; |err| / (2^-24 (|v| + |ref| + 1)) = %.3f' % (nc.case_id(c), ratio, nc.eval_ratio(C, ref)))
    lb.check(nc.case_id(c), C, ref['C'], ref['bound'])
    without = _run(gpu, c, dev, 'act', use_pre=False)
    assert torch.equal(nc.bits(without['C']), nc.bits(got['C'])), 'C changes with pre'
    plain = _run(gpu, c, dev, 'plain', act='none', use_gate=False, use_pre=False)
    want = nc.view(c, 'C', plain['C']).to(nc.DT[c['dtype']])
    assert torch.equal(nc.bits(nc.view(c, 'pre', got['pre'])), nc.bits(want)), 'pre is not the plain launch'
