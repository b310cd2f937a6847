"""Times the candidate-list kernels at C2 scoring size (R = 40,960 [MASK] rows, C = 1 + 100, V = 50,000, bf16, K = 128):
b4c_sample_candidates (popularity, 200 seen items excluded per row), b4c_candidate_score with rank (scores in LDS only),
with rank + top-10, with the scores written, and the logits-free full-vocabulary rank (b4c_vocab_rank) beside them.
Device events around `iters` back-to-back launches, after a warm-up; median of `reps` windows; one JSON line.
Bytes: the algorithmic gather (R*K*2 + R*C*K*2 + R*C*4) over the median time."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4clickpath_amd import ops  # noqa: E402


def timed(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=40960)
    ap.add_argument('--V', type=int, default=50000)
    ap.add_argument('--K', type=int, default=128)
    ap.add_argument('--negatives', type=int, default=100)
    ap.add_argument('--seen', type=int, default=200)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    R, V, K, N = a.rows, a.V, a.K, a.negatives
    g = torch.Generator(device='cuda').manual_seed(0)
    h = (torch.randn(R, K, device='cuda', generator=g) * 0.5).bfloat16()
    Vp = (V + 7) // 8 * 8
    wt = torch.zeros(Vp, K, device='cuda', dtype=torch.bfloat16)
    wt[:V] = (torch.randn(V, K, device='cuda', generator=g) * 0.3).bfloat16()
    bias = torch.zeros(Vp, device='cuda')
    bias[:V] = torch.randn(V, device='cuda', generator=g)
    y = torch.randint(0, V, (R,), device='cuda', generator=g, dtype=torch.int32)
    counts = torch.randint(1, 50, (V,), device='cuda', generator=g).to(torch.int64)
    cdf = torch.cumsum(counts, 0)
    ex = ops.exclusions(torch.randint(0, V, (R, a.seen), device='cuda', generator=g), V, y)
    cand, short = ops.sample_candidates(y, V, N, seed=1, exclude=ex, item_cdf=cdf)
    C = N + 1
    res = {'rows': R, 'V': V, 'K': K, 'C': C, 'seen': a.seen, 'short_rows': int(short)}
    ms = timed(lambda: ops.sample_candidates(y, V, N, seed=1, exclude=ex, item_cdf=cdf), a.iters, a.reps)
    res['sample_ms'] = ms
    ms = timed(lambda: ops.sample_candidates(y, V, N, seed=1), a.iters, a.reps)
    res['sample_uniform_noexcl_ms'] = ms
    gb = (R * K * 2 + R * C * K * 2 + R * C * 4) / 1e9
    res['gather_GB'] = gb
    for name, kw in (('score_rank', dict(want_scores=False)), ('score_rank_top10', dict(want_scores=False, k=10)),
                     ('score_rank_scores', dict(want_scores=True))):
        ms = timed(lambda: ops.candidate_scores(h, wt, bias, cand, V, labels=y, **kw), a.iters, a.reps)
        res[name + '_ms'] = ms
        res[name + '_TBps'] = gb / ms[0]             # GB per ms = TB/s
    logits = torch.randn(R, Vp, device='cuda', generator=g)
    ms = timed(lambda: ops.candidate_rank_rows(logits, V, cand, y, 10), a.iters, a.reps)
    res['rank_rows_fp32_ms'] = ms
    del logits
    ms = timed(lambda: ops.vocab_rank(h, wt, bias, y, V), 5, a.reps)
    res['vocab_rank_full_ms'] = ms
    # the rank's duplicate check (the LDS first-occurrence table; the position scan it replaced depended on the label's rank):
    # worst case, every listed item beats the label (label items carry bias -1e4), against the best case, none does (+1e4)
    for C2, R2 in ((101, R), (1024, 8192)):
        y2 = torch.randint(0, 100, (R2,), device='cuda', generator=g, dtype=torch.int32)
        c2 = torch.randint(100, V, (R2, C2), device='cuda', generator=g, dtype=torch.int32)
        for name, sign in (('worst', -1.0), ('best', 1.0)):
            b2 = bias.clone()
            b2[:100] = sign * 1e4
            ms = timed(lambda: ops.candidate_scores(h[:R2], wt, b2, c2, V, labels=y2, want_scores=False), a.iters // 5 or 1, a.reps)
            res['dedupe_scan_C%d_R%d_%s_ms' % (C2, R2, name)] = ms
    print(json.dumps(res))


if __name__ == '__main__':
    main()
