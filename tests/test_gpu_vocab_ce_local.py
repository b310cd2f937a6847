"""The logits-free vocabulary head (csrc/vocab_ce.hip) against float64, element by element: dh, dW and db of every route are held to
the bound tests/local_bounds.py derives for each ELEMENT (bf16 P in front of P W, bf16 dlogit in front of h^T dlogit, db from the
unrounded dlogit), so a missing last vocabulary column, bias entry or token row is a failure and not 0.2 % of a norm.

Cases: every split count (V in {50, 129, 300, 640, 700, 1000, 1301}, R <= 400; R = 5000 for a token split in the dW sweep), the clip
regime of the TF variant, and edge cases with V and R on / below / above the 128 tile edges whose labels sit on columns 0, 127, 128 and
V - 1 and whose ignored rows sit at rows 0, 127, 128 and R - 1.  Two input conditions are asserted on the reference before any GPU
comparison: under 5 % of the checked elements receive clip-decision slack, and every named edge of an edge case carries a reference
gradient of at least 10 % of the median of its peers.

Routes: b4c_vocab_ce_fwd (item losses at 2e-4, dh, the row lse in rowscal), b4c_vocab_lse, b4c_vocab_ce_dw atomic and deterministic,
b4c_vocab_ce_dw_sweep foreground and background + b4c_vocab_ce_dw_labels; everything once more in a child process with the 256-token
sweeps.

Worst |error| / bound per output and route on the MI355X (n = bf16 roundings counted on the path, see the table in local_bounds.py;
"loose" = the derived worst-case bound is far from what the kernel does, it is not tuned down):

  output   n   route                          128-token sweeps   256-token sweeps
  dh       1   b4c_vocab_ce_fwd               0.555              0.769
  lse      0   b4c_vocab_ce_fwd (rowscal)     0.018 (loose)      0.018 (loose)
  lse      0   b4c_vocab_lse                  0.018 (loose)      0.018 (loose)
  dW       1   b4c_vocab_ce_dw, atomic        0.879              0.879
  dW       1   b4c_vocab_ce_dw, deterministic 0.879              0.879
  dW       1   dw_sweep foreground + dw_labels 0.879              0.879
  dW       1   dw_sweep background + dw_labels 0.879              0.879
  db       0   b4c_vocab_ce_dw, atomic        0.134              0.134
  db       0   b4c_vocab_ce_dw, deterministic 0.134              0.134
  db       0   dw_sweep foreground + dw_labels 0.134              0.134
  db       0   dw_sweep background + dw_labels 0.134              0.134
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import local_bounds as lb

pytestmark = pytest.mark.gpu
LN2 = 0.6931471805599453


@pytest.fixture(scope='module')
def ops():
    from bert4clickpath_amd import ops as o
    return o


def _id(case):
    return '-'.join(str(c) for c in case)


def _cases():
    out = [c + (None,) for c in lb.VOCAB_CASES]
    for R, V, K, scale, variant, seed in lb.VOCAB_EDGE_CASES:
        for form in lb.EDGE_FORMS:
            out.append((R, V, K, scale, 0, variant, seed, form))
    return out


@functools.lru_cache(maxsize=None)
def _ref(case):
    R, V, K, scale, n_ign, variant, seed, edge = case
    h, W, b, y = lb.vocab_inputs(R, V, K, scale, n_ign, seed, edge=edge)
    return h, W, b, y, lb.vocab_ref(h, W, b, y, variant)


@pytest.mark.parametrize('case', _cases(), ids=_id)
def test_vocab_ce_every_element_within_its_bound(ops, case):
    from bert4clickpath_amd import _lib as L
    R, V, K, scale, n_ign, variant, seed, edge = case
    h, W, b, y, ref = _ref(case)
    # input conditions, on the reference
    assert max(ref['slack_share'].values()) < lb.SLACK_CAP, ref['slack_share']
    if edge is not None:
        rep = lb.edge_report(ref, V, R)
        if edge == 'ignored':
            rep = {k: v for k, v in rep.items() if not k.startswith('dh')}
        assert rep and min(rep.values()) >= lb.EDGE_MIN, rep
    dev = 'cuda'
    hd = torch.tensor(h, device=dev).bfloat16()
    Vp = (V + 7) // 8 * 8
    wt = torch.zeros(Vp, K, device=dev, dtype=torch.bfloat16)
    wt[:V] = torch.tensor(W, device=dev).bfloat16()
    bd = torch.zeros(Vp, device=dev)
    bd[:V] = torch.tensor(b, device=dev)
    yd = torch.tensor(y, device=dev)
    gs = torch.tensor([ref['gs']], device=dev, dtype=torch.float32)
    item, dh, rowscal = ops.vocab_ce_fwd(hd, wt, bd, yd, gs, V, L.CE_TF if variant == 'tf' else L.CE_PLAIN)
    item_o = ref['item'].numpy()
    np.testing.assert_allclose(item.cpu().numpy(), item_o, rtol=2e-4, atol=2e-4)
    assert abs(float(item.sum()) * ref['gs'] - ref['loss']) < 2e-4 * max(1.0, abs(ref['loss']))
    ratios = {'dh': lb.check('dh', dh, *ref['dh'])}
    valid = torch.from_numpy(y >= 0)
    ign = ~valid
    if bool(ign.any()):
        assert float(item.cpu()[ign].abs().max()) == 0.0 and float(dh.float().cpu()[ign].abs().max()) == 0.0
    # the row lse: what the forward leaves for the dW sweep (valid rows), and b4c_vocab_lse (every row)
    lse_ref, lse_b = ref['lse']
    ratios['lse fwd'] = lb.check('lse (rowscal)', rowscal[:, 0].cpu()[valid] * LN2, lse_ref[valid], lse_b[valid])
    lse2 = torch.empty(R, dtype=torch.float32, device=dev)
    ws = ops._vce_workspace(hd, R, V, K)
    L.check(L.lib().b4c_vocab_lse(ops._p(hd), hd.stride(0), ops._p(wt), wt.stride(0), ops._p(bd), ops._p(lse2), ws.data_ptr(), ws.numel(),
                                  R, V, K, ops._st()), 'vocab_lse')
    ratios['lse'] = lb.check('lse (b4c_vocab_lse)', lse2.cpu() * LN2, lse_ref, lse_b)

    def dw_routes():
        prev = ops.deterministic_vocab_dw
        nt = (V + 127) // 128
        try:
            for det in (False, True):
                ops.deterministic_vocab_dw = det
                dW, db = torch.zeros(K, V, device=dev), torch.zeros(V, device=dev)
                ops.vocab_ce_dw(hd, wt, bd, yd, rowscal, V, dW, db)
                yield ('dw det' if det else 'dw atomic'), dW, db
            ops.deterministic_vocab_dw = False
            for bg in (0, 3):
                dW, db = torch.zeros(K, V, device=dev), torch.zeros(V, device=dev)
                ops.vocab_ce_dw_labels(hd, yd, rowscal, V, dW, db)
                cut = nt // 2
                ops.vocab_ce_dw_sweep(hd, wt, bd, rowscal, V, dW, db, 0, cut, bg)
                ops.vocab_ce_dw_sweep(hd, wt, bd, rowscal, V, dW, db, cut, nt, bg)
                yield ('sweep bg' if bg else 'sweep fg'), dW, db
        finally:
            ops.deterministic_vocab_dw = prev
    for name, dW, db in dw_routes():
        ratios['dW ' + name] = lb.check('dW (%s)' % name, dW, *ref['dW'])
        ratios['db ' + name] = lb.check('db (%s)' % name, db, *ref['db'])
    print('RATIO vce tokens=%s %s %s' % (os.environ.get('B4C_VCE_TOKENS', 'default'), _id(case),
                                         ' '.join('%s=%.3f' % (k.replace(' ', '_'), v) for k, v in ratios.items())))


def test_the_256_token_sweeps_stay_within_the_same_bounds():
    """B4C_VCE_TOKENS=256 selects the 256-tokens-per-workgroup sweeps (the form of R >= 16,384) at any R; the switch is read once per
    process, so the cases above run again in a child process."""
    if os.environ.get('B4C_VCE_TOKENS'):
        pytest.skip('already inside the child run')
    env = dict(os.environ, B4C_VCE_TOKENS='256', B4C_VCE_SCAN_TOKENS='256')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-s', '-p', 'no:cacheprovider',
                        '-k', 'every_element'], capture_output=True, text=True, env=env, timeout=900,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print('\n'.join(ln for ln in r.stdout.splitlines() if ln.startswith('RATIO') or 'RATIO vce' in ln))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert '%d passed' % len(_cases()) in r.stdout, r.stdout[-500:]
