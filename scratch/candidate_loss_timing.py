"""Times the candidate-loss kernels at C2 training size (R = 40,960 rows, K = 128, V = 50,000, bf16 h, the fp32 master table read
at row offset 10): b4c_candidate_loss_fwd and b4c_candidate_loss_bwd at C = 2 (SASRec: one negative) and C = 101, lists drawn by
b4c_sample_candidates (uniform).  Device events around `iters` back-to-back launches, after a warm-up; median [min, max] of `reps`
windows; one JSON line.  Beside each backward time: the table gradient's added bytes R C K 4 over the time, to be read against
the chip-wide float-atomic rate (about 1.3 TB/s).

The forward of b4c_candidate_loss_fwd_ex (include/b4c.h) is timed beside them: BPR, and the kinds with a per-item
correction (a random fp32 [V] vector: the cost is one more gathered float per entry).

--parent_lib PATH: a libb4c_hip.so built from the commit before the extended forward.  Its b4c_candidate_loss_fwd is timed against
this tree's in the same process, the windows of the two alternating (new, parent, new, parent, ...), and the outputs of the two are
compared bit for bit.  `within` is the acceptance rule: new median <= parent median + the parent's own spread (max - min) + 2 %."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4clickpath_amd import _lib, ops  # noqa: E402
from candidates_timing import timed  # noqa: E402

EX_SETTINGS = (('bpr', 1.0, False, False), ('bpr', 1.0, True, False), ('bce', 0.37, True, False), ('softmax', 1.0, True, False),
               ('softmax', 1.0, True, True))


def timed_alternating(fns, iters, reps):
    """timed() for several functions whose windows alternate -> [(median, min, max)] in their order"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[i].append(a.elapsed_time(b) / iters)
    return [(sorted(o)[len(o) // 2], min(o), max(o)) for o in out]


def raw_forward(lib):
    """b4c_candidate_loss_fwd of a build of the library through the bare binding, into outputs the caller keeps: the same host
    path for this tree's build and for another one (the entry point's argument list did not change)"""
    fn = lib.b4c_candidate_loss_fwd
    fn.restype, fn.argtypes = _lib.signatures()['b4c_candidate_loss_fwd']

    def fwd(h, table, bias, cand, V, kind, off, item, g):
        R, K = h.shape
        C = cand.shape[1]
        rc = fn(h.data_ptr(), h.stride(0), table.data_ptr(), table.stride(0), table.shape[0], off, bias.data_ptr(), cand.data_ptr(),
                cand.stride(0), R, C, V, K, _lib.BF16, ops.CAND_LOSS_KINDS[kind], item.data_ptr(), g.data_ptr(), C, None, 0,
                torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError('b4c_candidate_loss_fwd refused the call (rc = %d)' % rc)
    return fwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=40960)
    ap.add_argument('--V', type=int, default=50000)
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--parent_lib', default=None, help='a libb4c_hip.so of the parent commit: its forward, alternating with this one')
    a = ap.parse_args()
    R, V, K, off = a.rows, a.V, a.K, 10
    g = torch.Generator(device='cuda').manual_seed(0)
    h = (torch.randn(R, K, device='cuda', generator=g) * 0.5).bfloat16()
    table = torch.randn(V + off + 1, K, device='cuda', generator=g) * 0.3
    bias = torch.randn(V, device='cuda', generator=g)
    corr = torch.randn(V, device='cuda', generator=g)
    y = torch.randint(0, V, (R,), device='cuda', generator=g, dtype=torch.int32)
    dtable, dbias = torch.zeros_like(table), torch.zeros_like(bias)
    gscale = torch.full((1,), 1.0 / R, device='cuda')
    new, parent = (raw_forward(_lib.lib()), raw_forward(ctypes.CDLL(a.parent_lib))) if a.parent_lib else (None, None)
    res = {'rows': R, 'V': V, 'K': K}
    for N in (1, 100):
        C = N + 1
        cand, _ = ops.sample_candidates(y, V, N, seed=1)
        for kind in ('bce', 'softmax'):
            item, coef, _ = ops.candidate_loss_fwd(h, table, bias, cand, V, kind, off)
            row = {}
            fwd = timed(lambda: ops.candidate_loss_fwd(h, table, bias, cand, V, kind, off), a.iters, a.reps)
            if parent is not None:
                item_n, coef_n = torch.full_like(item, -1.0), torch.full_like(coef, -1.0)
                item_p, coef_p = torch.full_like(item, -2.0), torch.full_like(coef, -2.0)
                new(h, table, bias, cand, V, kind, off, item_n, coef_n)
                parent(h, table, bias, cand, V, kind, off, item_p, coef_p)
                torch.cuda.synchronize()
                row['bits_equal_parent'] = bool(torch.equal(item_n.view(torch.int32), item_p.view(torch.int32))
                                                and torch.equal(coef_n.view(torch.int32), coef_p.view(torch.int32))
                                                and torch.equal(item_n.view(torch.int32), item.view(torch.int32)))
                mine, old = timed_alternating([lambda: new(h, table, bias, cand, V, kind, off, item_n, coef_n),
                                               lambda: parent(h, table, bias, cand, V, kind, off, item_p, coef_p)], a.iters, a.reps)
                row.update({'raw_fwd_ms': mine, 'raw_parent_fwd_ms': old,
                            'within': bool(mine[0] <= old[0] + (old[2] - old[1]) + 0.02 * old[0])})
            bwd = timed(lambda: ops.candidate_loss_bwd(h, table, cand, coef, gscale, V, dtable, dbias, off), a.iters, a.reps)
            row.update({'fwd_ms': fwd, 'bwd_ms': bwd, 'gather_GB': R * C * K * 4 / 1e9, 'fwd_gather_TBps': R * C * K * 4 / 1e9 / fwd[0],
                        'bwd_atomic_TBps': R * C * K * 4 / 1e9 / bwd[0]})
            res['C%d_%s' % (C, kind)] = row
        for kind, beta, with_corr, target in EX_SETTINGS:
            q = corr if with_corr else None
            fwd = timed(lambda: ops.candidate_loss_fwd_ex(h, table, bias, cand, V, kind, off, False, beta, q, target), a.iters, a.reps)
            name = kind + ('' if beta == 1.0 else '_beta%g' % beta) + ('_corr' if with_corr else '') + ('_target' if target else '')
            res['C%d_ex_%s' % (C, name)] = {'fwd_ms': fwd, 'fwd_gather_TBps': R * C * K * 4 / 1e9 / fwd[0]}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
