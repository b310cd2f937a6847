"""Device time of the next-item batch builder against the route composed from the pieces that existed before it (DESIGN, "Next-item
batches").

Rows: B = 4096 whole-sequence windows of 20 .. 200 inputs (the lengths and the Zipf(1.1) items of input_pipeline.synthetic_cloze_batch,
bench.py's workload), W = 200, V = 50,000, holdout 1, N = 1 and N = 100 negatives per target.
  (a) DeviceCloze.next_item_window_batch with the window indices on the device already (ops.next_item_batch and the cumsum in
      front of it): items, flat_idx, labels, candidates.
  (b) the same four tensors from cloze_history (the row's items, which are also the sequence's history) -> ids, flat_idx / labels
      by the torch construction of tests/test_gpu_causal_model.py, the history gathered per target, ops.exclusions,
      ops.sample_candidates.  Its lists are drawn at other counters, so only their validity is compared, not their bits.
The two take turns; per round `--iters` calls each between two device events (the composed route synchronises inside: its boolean
indexing reads a count back); median [min, max] over the rounds after one warm-up round; (b)'s peak extra device memory; then one
training step model.next_item_loss(loss='bce') + backward + Adam on the bf16 causal example model at the same shape.  One JSON line.

    python scratch/next_item_cost.py"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bert4clickpath_amd import ops, optim  # noqa: E402
from bert4clickpath_amd.cloze_batches import DeviceCloze  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return [round(x, 4) for x in (xs[len(xs) // 2], xs[0], xs[-1])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=4096)
    ap.add_argument('--W', type=int, default=200)
    ap.add_argument('--V', type=int, default=50000)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=6)
    a = ap.parse_args()
    B, W, V = a.B, a.W, a.V
    rng = np.random.default_rng(4321)
    lens = rng.integers(20, W + 1, size=B)                         # inputs per row
    n = lens + 2                                                   # + the last training item (a target only) + the held-out item
    offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    ranks = np.arange(1, V + 1, dtype=np.float64)
    cdf = np.cumsum(ranks ** -1.1)
    items = np.searchsorted(cdf / cdf[-1], rng.random(int(offsets[-1]))).astype(np.int32).clip(0, V - 1)
    dc = DeviceCloze(items, offsets, V=V, holdout=1)
    win = rng.permutation(B)
    win_dev = dc._upload(win)
    seq_dev = win_dev
    n_in = dc.next_item_counts(win)
    R = int(n_in.sum())
    S = W + 3
    E = int(n.max()) - 1

    def new(N):
        return dc._next_batch(ops.NEXT_TRAIN, win, win_dev, seq_dev, n_in, n_in, dc._next_train()[1], 7, W, N, 'history', None, None, 1)

    def composed(N):
        hist = ops.cloze_history(dc.items_dev, dc.offsets_dev, seq_dev, E, 1)          # (B, E): the training view, -1 padded
        row = hist[:, :W]
        nxt = torch.cat([hist[:, 1:W + 1], hist.new_full((B, max(W + 1 - E, 0)), -1)], 1)[:, :W]
        src = (row >= 0) & (nxt >= 0)                                                   # an item followed by an item of the view
        ids = torch.where(src, row.long() + 10, torch.zeros_like(row, dtype=torch.int64))
        flat = (torch.arange(B * S, device='cuda', dtype=torch.int32).view(B, S)[:, 2:2 + W])[src]
        lab = nxt[src]
        ex = ops.exclusions(hist[(flat // S).long()], V, lab)                           # (R, E), twice
        cand, short = ops.sample_candidates(lab, V, N, 7, 0, ex)
        return {'items': ids, 'flat_idx': flat, 'labels': lab, 'candidates': cand, 'short': short}

    res = {'what': 'ms per batch, median [min, max] of %d rounds x %d calls, interleaved' % (a.rounds, a.iters), 'B': B, 'W': W, 'V': V,
           'targets': R}
    for N in (1, 100):
        x, y = new(N), composed(N)
        torch.cuda.synchronize()
        for k in ('items', 'flat_idx', 'labels'):
            assert torch.equal(x[k], y[k]), k
        assert torch.equal(x['candidates'][:, 0], y['candidates'][:, 0]) and int(x['short']) == int(y['short']) == 0
        seen = ops.cloze_history(dc.items_dev, dc.offsets_dev, seq_dev, E, 1)[(x['flat_idx'] // S).long()]
        assert not bool((x['candidates'][:20000, 1:, None] == seen[:20000, None, :64]).any())      # (a spot check)
        del x, y, seen
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        composed(N)
        torch.cuda.synchronize()
        res['composed_peak_extra_MB_N%d' % N] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        torch.cuda.reset_peak_memory_stats()
        new(N)
        torch.cuda.synchronize()
        res['next_item_peak_extra_MB_N%d' % N] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        ms = {'next_item_batch': [], 'composed': []}
        for r in range(a.rounds + 1):
            for k, f in (('next_item_batch', new), ('composed', composed)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    f(N)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    ms[k].append(e0.elapsed_time(e1) / a.iters)
        res['N%d' % N] = {k: spread(v) for k, v in ms.items()}
        res['N%d' % N]['composed_over_next_item'] = round(res['N%d' % N]['composed'][0] / res['N%d' % N]['next_item_batch'][0], 2)
    # one training step beside the builder
    from examples.beauty_hitrate import build_model
    model = build_model(V, 0.1, torch.bfloat16, attention='causal', tied_head=True).cuda()
    opt = optim.Adam(model.parameters())
    step_ms, build_ms = [], []
    for s in range(a.steps + 2):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        b = new(1)
        e1.record()
        opt.zero_grad()
        loss = model.next_item_loss(b, loss='bce')
        loss.backward()
        opt.step()
        e2.record()
        torch.cuda.synchronize()
        if s >= 2:
            build_ms.append(e0.elapsed_time(e1))
            step_ms.append(e1.elapsed_time(e2))
    res['train_step_bce_N1'] = {'model': 'examples build_model: bf16, causal, tied head, d = 64, 2 layers', 'loss': float(loss.detach()),
                                'step_ms': spread(step_ms), 'builder_ms_in_loop': spread(build_ms)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
