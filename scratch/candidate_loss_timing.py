"""Times the candidate-loss kernels at C2 training size (R = 40,960 rows, K = 128, V = 50,000, bf16 h, the fp32 master table read
at row offset 10): b4c_candidate_loss_fwd and b4c_candidate_loss_bwd at C = 2 (SASRec: one negative) and C = 101, lists drawn by
b4c_sample_candidates (uniform).  Device events around `iters` back-to-back launches, after a warm-up; median [min, max] of `reps`
windows; one JSON line.  Beside each backward time: the table gradient's added bytes R C K 4 over the time, to be read against
the chip-wide float-atomic rate (about 1.3 TB/s)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4clickpath_amd import ops  # noqa: E402
from candidates_timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=40960)
    ap.add_argument('--V', type=int, default=50000)
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    R, V, K, off = a.rows, a.V, a.K, 10
    g = torch.Generator(device='cuda').manual_seed(0)
    h = (torch.randn(R, K, device='cuda', generator=g) * 0.5).bfloat16()
    table = torch.randn(V + off + 1, K, device='cuda', generator=g) * 0.3
    bias = torch.randn(V, device='cuda', generator=g)
    y = torch.randint(0, V, (R,), device='cuda', generator=g, dtype=torch.int32)
    dtable, dbias = torch.zeros_like(table), torch.zeros_like(bias)
    gscale = torch.full((1,), 1.0 / R, device='cuda')
    res = {'rows': R, 'V': V, 'K': K}
    for N in (1, 100):
        C = N + 1
        cand, _ = ops.sample_candidates(y, V, N, seed=1)
        for kind in ('bce', 'softmax'):
            _, coef, _ = ops.candidate_loss_fwd(h, table, bias, cand, V, kind, off)
            fwd = timed(lambda: ops.candidate_loss_fwd(h, table, bias, cand, V, kind, off), a.iters, a.reps)
            bwd = timed(lambda: ops.candidate_loss_bwd(h, table, cand, coef, gscale, V, dtable, dbias, off), a.iters, a.reps)
            res['C%d_%s' % (C, kind)] = {'fwd_ms': fwd, 'bwd_ms': bwd, 'gather_GB': R * C * K * 4 / 1e9,
                                         'fwd_gather_TBps': R * C * K * 4 / 1e9 / fwd[0],
                                         'bwd_atomic_TBps': R * C * K * 4 / 1e9 / bwd[0]}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
