"""The element-wise comparator of tests/local_bounds.py, tested without a GPU.

1. It accepts honest rounding: the kernels' rounding steps (the table in local_bounds.py), emulated in torch on the CPU, stay inside the
   bound on every case the GPU tests commit to -- the reference alone never trips it.
2. It rejects planted LOCAL errors, each applied to the float64 reference itself, and the whole-tensor metrics the suite used before
   (max error over the max of the whole tensor at 2.5e-2; 1 % of the whole tensor's L2 norm) accept the same errors on the cases
   they were measured on: the reason this module exists, kept on record.
3. The input conditions of the committed cases hold: under 5 % of the checked elements receive clip-decision slack, and every named
   kernel edge of the vocabulary-head edge cases carries a reference gradient of at least 10 % of the median of its peers."""
import functools

import numpy as np
import pytest
import torch

import local_bounds as lb

NAMES = ('o', 'lse', 'dq', 'dk', 'dv')


def _route(dtype, mq=False):
    return 'row_f32' if dtype == torch.float32 else ('mq_mfma' if mq else 'mfma')


def _id(case):
    return '-'.join(str(c).replace('torch.', '') for c in case)


@functools.lru_cache(maxsize=None)
def _dense(case):
    dtype, B, S, H, dh, pattern = case
    qkv, pad, do = lb.dense_inputs(*case)
    return qkv, pad, do, lb.attn_dense(qkv, pad, do, B, S, H, dh, _route(dtype))


def test_bf16_unit_roundoff_is_two_to_the_minus_eight():
    """One bf16 rounding reaches a relative error of almost 2^-8; 2^-9 is not a bound for it."""
    x = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -12], dtype=torch.float64)
    err = float(((lb.bf16r(x) - x) / x).abs())
    assert 2.0 ** -9 < err <= lb.U_BF16 == 2.0 ** -8
    g = torch.Generator().manual_seed(0)
    y = torch.randn(100000, generator=g, dtype=torch.float64)
    assert float(((lb.bf16r(y) - y) / y).abs().max()) <= lb.U_BF16


# ------------------------------------------------------------------------------------------------------------------
# 1. honest rounding is accepted
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', lb.dense_cases(), ids=_id)
def test_dense_attention_emulated_rounding_is_accepted(case):
    dtype, B, S, H, dh, pattern = case
    qkv, pad, do, res = _dense(case)
    d = H * dh
    items = [(b * S, (b + 1) * S, b * S, (b + 1) * S) for b in range(B)]
    em = lb.attn_emulate(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], do, items, ~pad.bool().reshape(-1), H, dh, _route(dtype))
    em['lse'] = em['lse'].reshape(B, S, H).permute(0, 2, 1)
    for n in NAMES:
        lb.check('%s %s' % (_id(case), n), em[n], *res[n])
    # padded keys: the bound itself is an exact zero
    live = ~pad.bool().reshape(-1)
    for n in ('dk', 'dv'):
        assert float(res[n][1][~live].abs().max()) == 0.0 and float(res[n][0][~live].abs().max()) == 0.0


@pytest.mark.parametrize('lens,H,dh', lb.PACKED_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_packed_attention_emulated_rounding_is_accepted(lens, H, dh):
    qkv, cu, do = lb.packed_inputs(lens, H, dh)
    res = lb.attn_packed(qkv, cu, do, H, dh, 'mfma')
    d = H * dh
    items = [(int(cu[b]), int(cu[b + 1]), int(cu[b]), int(cu[b + 1])) for b in range(len(lens))]
    em = lb.attn_emulate(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], do, items, torch.ones(sum(lens), dtype=torch.bool), H, dh, 'mfma')
    for n in NAMES:
        lb.check('packed %s %s' % (lens, n), em[n], *res[n])


@pytest.mark.parametrize('case', lb.MQ_CASES, ids=_id)
def test_masked_query_attention_emulated_rounding_is_accepted(case):
    dtype, H, dh, smax, mmax, pad = case
    cu, moff, q, kv, go, key_pad = lb.mq_inputs(*case)
    route = _route(dtype, mq=True)
    res = lb.attn_mq(q, kv, cu, moff, go, H, dh, route, key_pad)
    d = H * dh
    items = [(int(moff[b]), int(moff[b + 1]), int(cu[b]), int(cu[b + 1])) for b in range(len(cu) - 1)]
    live = torch.ones(kv.shape[0], dtype=torch.bool) if key_pad is None else ~key_pad.bool()
    em = lb.attn_emulate(q, kv[:, :d], kv[:, d:], go, items, live, H, dh, route)
    for n in NAMES:
        lb.check('mq %s %s' % (_id(case), n), em[n], *res[n])
    for b in range(len(cu) - 1):                    # sequences without a query row: bound 0, exact zeros demanded
        if moff[b + 1] == moff[b]:
            rows = slice(int(cu[b]), int(cu[b + 1]))
            assert float(res['dk'][1][rows].max()) == 0.0 and float(res['dv'][1][rows].max()) == 0.0


@functools.lru_cache(maxsize=None)
def _vocab(R, V, K, scale, n_ign, variant, seed, edge=None):
    h, W, b, y = lb.vocab_inputs(R, V, K, scale, n_ign, seed, edge=edge)
    return h, W, b, y, lb.vocab_ref(h, W, b, y, variant)


def _vocab_all():
    out = [c + (None,) for c in lb.VOCAB_CASES]
    for R, V, K, scale, variant, seed in lb.VOCAB_EDGE_CASES:
        for form in lb.EDGE_FORMS:
            out.append((R, V, K, scale, 0, variant, seed, form))
    return out


@pytest.mark.parametrize('case', _vocab_all(), ids=_id)
def test_vocabulary_head_emulated_rounding_is_accepted_and_input_conditions_hold(case):
    R, V, K, scale, n_ign, variant, seed, edge = case
    h, W, b, y, ref = _vocab(*case)
    assert max(ref['slack_share'].values()) < lb.SLACK_CAP, ref['slack_share']
    em = lb.vocab_emulate(h, W, b, y, variant, ref)
    for n in ('dh', 'dW', 'db'):
        lb.check('%s %s' % (_id(case), n), em[n], *ref[n])
    ign = y < 0
    if ign.any():
        assert float(ref['dh'][1][torch.from_numpy(ign)].max()) == 0.0          # ignored rows: exact zeros demanded
    if edge is not None:
        rep = lb.edge_report(ref, V, R)
        if edge == 'ignored':         # the last row (and, where it is the last token tile's only row, that tile) is ignored: exact zeros
            rep = {k: v for k, v in rep.items() if not k.startswith('dh')}
        assert rep and min(rep.values()) >= lb.EDGE_MIN, rep


def test_the_old_tail_case_does_not_stand_for_the_tail():
    """(130, 129, 64, 2.0, 'tf'), commented "vocabulary tail of one row" in test_gpu_vocab_ce.py: at operand scale 2.0 nearly every
    probability is outside the clip range; the tail column's and the last row's gradients are (next to) nothing."""
    h, W, b, y, ref = _vocab(130, 129, 64, 2.0, 0, 'tf', 1)
    rep = lb.edge_report(ref, 129, 130)
    assert min(rep.values()) < lb.EDGE_MIN


# ------------------------------------------------------------------------------------------------------------------
# 2. planted local errors: rejected here, accepted by the whole-tensor metrics
# ------------------------------------------------------------------------------------------------------------------
WHY = [(2, 200, 2, 64), (2, 256, 2, 64), (3, 257, 2, 64), (2, 300, 2, 32), (2, 512, 4, 64)]       # the issue's table: bf16, 'short' pattern


def _old_bwd_metric(res, **planted):
    """test_attention_fwd_bwd: max |got - ref| / max |ref| over dq | dk | dv of all sequences, < 2.5e-2"""
    ref = torch.cat([res[n][0] for n in ('dq', 'dk', 'dv')], 1)
    got = torch.cat([planted.get(n, res[n][0]) for n in ('dq', 'dk', 'dv')], 1)
    return lb.old_rel_max(got, ref)


def _head_tensors(qkv, pad, do, b, h, S, H, dh):
    d = H * dh
    rows, cs = slice(b * S, (b + 1) * S), slice(h * dh, (h + 1) * dh)
    q64 = qkv.double()
    q, k, v = q64[rows, cs], q64[rows, d + h * dh:d + (h + 1) * dh], q64[rows, 2 * d + h * dh:2 * d + (h + 1) * dh]
    c = 1.0 / float(np.sqrt(np.float32(dh)))
    P = torch.softmax((q @ k.T) * c + pad[b].double()[None, :] * -1e9, 1)
    g = do.double()[rows, cs]
    dS = P * (g @ v.T - (g * (P @ v)).sum(1, keepdim=True))
    return rows, cs, q, k, v, P, dS, c


@pytest.mark.parametrize('B,S,H,dh', WHY)
def test_planted_attention_errors(B, S, H, dh):
    qkv, pad, do, res = _dense((torch.bfloat16, B, S, H, dh, 'short'))
    d = H * dh
    # sequence 0's dQ x 1.1
    dq = res['dq'][0].clone()
    dq[:S] *= 1.1
    assert not lb.accepts(dq, *res['dq'])
    assert _old_bwd_metric(res, dq=dq) < 2.5e-2
    # one head's dK zeroed (sequence 0, head 0): a 100 % error, which the old metric admits where the issue's table says so
    dk = res['dk'][0].clone()
    dk[:S, :dh] = 0.0
    assert not lb.accepts(dk, *res['dk'])
    if S > 200:
        assert _old_bwd_metric(res, dk=dk) < 2.5e-2
    # the second key block's dQ partial doubled (the S > 256 route sums two blocks), on every long sequence (all but sequence 1, whose
    # six live keys are what sets the old metric's scale)
    if S > 256:
        dq = res['dq'][0].clone()
        for b in range(B):
            if b == 1:
                continue
            for h in range(H):
                rows, cs, q, k, v, P, dS, c = _head_tensors(qkv, pad, do, b, h, S, H, dh)
                dq[rows, cs] += (dS[:, 256:] @ k[256:]) * c
        assert not lb.accepts(dq, *res['dq'])
        assert _old_bwd_metric(res, dq=dq) < 2.5e-2
    # the last live key dropped from one query row of o: the row of sequence 0, head 0 with the median weight on that key
    rows, cs, q, k, v, P, dS, c = _head_tensors(qkv, pad, do, 0, 0, S, H, dh)
    kl = S - 5
    row = int(P[:, kl].argsort()[S // 2])
    o = res['o'][0].clone()
    o[row, cs] -= P[row, kl] * v[kl]
    assert not lb.accepts(o, *res['o'])
    assert lb.old_rel_max(o, res['o'][0]) < 1.2e-2
    # one query row's lse off by 1e-2 (the old bound: 3e-2 absolute)
    lse = res['lse'][0].clone()
    lse[0, 0, 3] += 1e-2
    assert not lb.accepts(lse, *res['lse'])
    assert float((lse - res['lse'][0]).abs().max()) < 3e-2


OLD_VOCAB = [(300, 1000, 128, 0.3, 0, 'tf', 1), (130, 129, 64, 2.0, 0, 'tf', 1), (257, 700, 128, 1.2, 7, 'plain', 1)]


def _vocab_plants(ref, R, V):
    dh, dW, db = ref['dh'][0], ref['dW'][0], ref['db'][0]
    tail = (V - 1) // 128 * 128
    out = {}
    x = dW.clone(); x[:, V - 1] = 0.0; out['dW[:, V-1] zeroed'] = ('dW', x)
    x = db.clone(); x[V - 1] = 0.0; out['db[V-1] zeroed'] = ('db', x)
    x = dW.clone(); x[:, tail:] *= 1.1; out['dW of the tail tile x 1.1'] = ('dW', x)
    if R > 128:
        x = dh.clone(); x[128:256] *= 1.05; out['dh rows 128..255 x 1.05'] = ('dh', x)
    x = dh.clone(); x[R - 1] = 0.0; out['last row of dh zeroed'] = ('dh', x)
    return out


@pytest.mark.parametrize('case', [lb.VOCAB_CASES[0] + (None,)] + [c[:4] + (0,) + c[4:] + ('labels',) for c in lb.VOCAB_EDGE_CASES], ids=_id)
def test_planted_vocabulary_head_errors_are_rejected(case):
    R, V, K = case[:3]
    h, W, b, y, ref = _vocab(*case)
    for what, (name, planted) in _vocab_plants(ref, R, V).items():
        assert not lb.accepts(planted, *ref[name]), what


@pytest.mark.parametrize('case', OLD_VOCAB, ids=_id)
def test_the_whole_tensor_l2_metric_accepts_planted_tail_errors(case):
    """The old assertion: ||got - ref|| / ||ref|| < 1e-2 per tensor.  What it lets through on the cases the issue measured: a missing
    last vocabulary column, a missing last bias entry, a tail tile off by 10 %; on the clip-regime case also a missing last token row and
    rows 128.. off by 5 % (its tail carries next to no gradient at all)."""
    R, V, K = case[:3]
    h, W, b, y, ref = _vocab(*case)
    plants = _vocab_plants(ref, R, V)
    accepted = ['dW[:, V-1] zeroed']
    if V == 129:
        accepted += ['db[V-1] zeroed', 'dW of the tail tile x 1.1', 'dh rows 128..255 x 1.05', 'last row of dh zeroed']
    for what in accepted:
        name, planted = plants[what]
        assert lb.old_rel_l2(planted, ref[name][0]) < 1e-2, what
