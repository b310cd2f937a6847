"""The attention kernels against float64, element by element: every output (o, lse, dq, dk, dv) of every route is held to the bound
tests/local_bounds.py derives for that ELEMENT from the kernel's rounding steps -- no tensor-wide scale, so a sequence with small
gradients is checked as closely as the one whose six live keys make its dK / dV huge.  (The whole-tensor assertions of
test_gpu_kernels.py / test_gpu_packed.py / test_gpu_mq.py admit a 60 - 185 % error on the long sequence's dQ / dK;
tests/test_local_bounds_cpu.py keeps that on record.)

Routes: bf16 MFMA forward (one and two query tiles per wave), resident backward (S <= 256) and key-block backward (S > 256), dense
and packed layout; the fp32 row kernels (head depths 16 .. 128); the masked-query kernels in both dtypes.  Every dense case runs in two
padding patterns ('short': sequence 1 keeps about six live keys; 'long': every sequence long), so the large and the small gradients
both sit on every route.

Worst |error| / bound per output and route on the MI355X (n = bf16 roundings counted on the path, see the table in local_bounds.py;
"loose" = the derived worst-case bound is far from what the kernel does, it is not tuned down):

  route                                     n (o/lse/dq/dk/dv)   o               lse             dq              dk              dv
  bf16 MFMA, resident backward (S <= 256)   1 / 0 / 1 / 1 / 1    0.754           0.029 (loose)   0.274           0.149           0.573          
  bf16 MFMA, key-block backward (S > 256)   1 / 0 / 1 / 1 / 1    0.765           0.021 (loose)   0.233           0.062 (loose)   0.269          
  bf16 MFMA, packed layout                  1 / 0 / 1 / 1 / 1    0.581           0.024 (loose)   0.157           0.151           0.675          
  fp32 row kernels                          0 (u = 2^-24)        0.009 (loose)   0.052 (loose)   0.003 (loose)   0.003 (loose)   0.007 (loose)  
  masked-query bf16 MFMA                    1 / 0 / 1 / 1 / 1    0.758           0.027 (loose)   0.222           0.346           0.886          
  masked-query fp32                         0 (u = 2^-24)        0.007 (loose)   0.023 (loose)   0.002 (loose)   0.004 (loose)   0.011 (loose)  
"""
import functools

import pytest
import torch

import local_bounds as lb

pytestmark = pytest.mark.gpu

NAMES = ('o', 'lse', 'dq', 'dk', 'dv')


@pytest.fixture(scope='module')
def ops():
    from bert4clickpath_amd import ops as _ops
    return _ops


def _id(case):
    return '-'.join(str(c).replace('torch.', '').replace(' ', '') for c in case)


def _report(route, tag, ratios):
    print('RATIO attn %s %s %s' % (route, tag, ' '.join('%s=%.3f' % (n, ratios[n]) for n in NAMES)))


@functools.lru_cache(maxsize=None)
def _dense_ref(case):
    dtype, B, S, H, dh, pattern = case
    qkv, pad, do = lb.dense_inputs(*case)
    return qkv, pad, do, lb.attn_dense(qkv, pad, do, B, S, H, dh, 'row_f32' if dtype == torch.float32 else 'mfma')


@pytest.mark.parametrize('case', lb.dense_cases(), ids=_id)
def test_dense_attention_every_element_within_its_bound(ops, case):
    dtype, B, S, H, dh, pattern = case
    qkv, pad, do, res = _dense_ref(case)
    d = H * dh
    qd, dod, padd = qkv.cuda().to(dtype), do.cuda().to(dtype), pad.cuda()
    o, lse = ops.attn_fwd(qd, padd, B, S, H, dh)
    dqkv = ops.attn_bwd(qd, padd, o, dod, lse, B, S, H, dh)           # the kernel's own o and lse, as in training
    got = {'o': o, 'lse': lse, 'dq': dqkv[:, :d], 'dk': dqkv[:, d:2 * d], 'dv': dqkv[:, 2 * d:]}
    if dtype == torch.bfloat16:
        ws = ops.L.lib().b4c_attn_bwd_workspace_bytes(B, S, H, dh, ops.L.BF16)
        assert ws == (B * S * H * dh * 4 if S > 256 else 0)              # key-block route above 256 keys, resident below
        route = 'mfma-keyblocks' if S > 256 else 'mfma-resident'
    else:
        route = 'row_f32'
    ratios = {n: lb.check('%s %s' % (_id(case), n), got[n], *res[n]) for n in NAMES}
    _report(route, _id(case), ratios)
    # padded keys: the bound is an exact 0 there (check() has demanded exact zeros); make sure the case has some
    assert float(res['dk'][1][pad.bool().reshape(-1)].max()) == 0.0 and int(pad.sum()) > 0


@pytest.mark.parametrize('lens,H,dh', lb.PACKED_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_packed_attention_every_element_within_its_bound(ops, lens, H, dh):
    qkv, cu, do = lb.packed_inputs(lens, H, dh)
    res = lb.attn_packed(qkv, cu, do, H, dh, 'mfma')
    B, d, T, S_max = len(lens), H * dh, sum(lens), max(lens)
    qd, dod, cud = qkv.cuda().bfloat16(), do.cuda().bfloat16(), cu.cuda()
    key_pad = torch.zeros(T, dtype=torch.uint8, device='cuda')
    o, lse = ops.attn_fwd(qd, key_pad, B, S_max, H, dh, cud)
    dqkv = ops.attn_bwd(qd, key_pad, o, dod, lse, B, S_max, H, dh, cud)
    got = {'o': o, 'lse': lb.packed_lse(lse.cpu(), cu), 'dq': dqkv[:, :d], 'dk': dqkv[:, d:2 * d], 'dv': dqkv[:, 2 * d:]}
    ratios = {n: lb.check('packed %s %s' % (lens, n), got[n], *res[n]) for n in NAMES}
    _report('mfma-packed', str(lens).replace(' ', ''), ratios)


@pytest.mark.parametrize('case', lb.MQ_CASES, ids=_id)
def test_masked_query_attention_every_element_within_its_bound(ops, case):
    dtype, H, dh, smax, mmax, pad = case
    cu, moff, q, kv, go, key_pad = lb.mq_inputs(*case)
    route = 'row_f32' if dtype == torch.float32 else 'mq_mfma'
    res = lb.attn_mq(q, kv, cu, moff, go, H, dh, route, key_pad)
    B, d, dev = len(cu) - 1, H * dh, 'cuda'
    kp = key_pad.to(dev) if key_pad is not None else None
    o, lse = ops.attn_mq_fwd(q.to(dev), kv.to(dev), cu.to(dev), moff.to(dev), B, smax, H, dh, kp)
    dq, dkv = ops.attn_mq_bwd(q.to(dev), kv.to(dev), cu.to(dev), moff.to(dev), o, go.to(dev), lse, B, smax, H, dh, kp)
    got = {'o': o, 'lse': lse, 'dq': dq, 'dk': dkv[:, :d], 'dv': dkv[:, d:]}          # dk and dv each against its own bound
    ratios = {n: lb.check('mq %s %s' % (_id(case), n), got[n], *res[n]) for n in NAMES}
    _report('mq-' + route, _id(case), ratios)
