"""Device time of the side-feature gather (ops.batch_features) against the route composed from the pieces that existed before it
(DESIGN, "Side features of device-built batches").

Rows: B = 4096 whole-sequence windows of 20 .. 200 items (the lengths and the Zipf(1.1) items of input_pipeline.synthetic_cloze_batch,
bench.py's workload), W = 200, V = 50,000, holdout 1.  Two features: an action per event (7 values, kept at [MASK]) and a category
per item (50 values, masked with the item).  Two layouts: the Cloze TRAIN rows and the next-item TRAIN rows; the item rows are built
once by the real builders and both routes take them as given.
  (a) ops.batch_features: one launch, the two (B, W) int64 outputs.
  (b) the same two tensors with torch: the rows' (first, n) by index arithmetic on the device window table, a (B, W) index into the
      CSR arrays, advanced indexing of the event column / of the items and then the table, torch.where for pad and [MASK].
      Its outputs are checked equal to (a)'s.
The two take turns; per round `--iters` calls each between two device events; median [min, max] over the rounds after one warm-up
round; both routes' peak extra device memory; then one training step cloze_loss + backward + Adam of a bf16 two-feature model
(items + category, feature_combine='sum', d = 64, 2 layers, tied head) on the Cloze batch.  One JSON line.

    python scratch/batch_features_cost.py"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bert4clickpath_amd import ops, optim  # noqa: E402
from bert4clickpath_amd.cloze_batches import DeviceCloze, Feature  # noqa: E402
from bert4clickpath_amd.input_pipeline import TRAIN  # noqa: E402

ACTIONS, CATS = 7, 50


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
    lens = rng.integers(20, W + 1, size=B)                         # items per Cloze row (the next-item row has one fewer)
    offsets = np.concatenate([[0], np.cumsum(lens + 1)]).astype(np.int64)      # + the held-out item
    ranks = np.arange(1, V + 1, dtype=np.float64)
    cdf = np.cumsum(ranks ** -1.1)
    items = np.searchsorted(cdf / cdf[-1], rng.random(int(offsets[-1]))).astype(np.int32).clip(0, V - 1)
    event = rng.integers(0, ACTIONS, len(items)).astype(np.int32)
    table = rng.integers(0, CATS, V).astype(np.int32)
    dc = DeviceCloze(items, offsets, V=V, holdout=1, features={'action': Feature(event, ACTIONS, per='event', on_mask='keep'),
                                                               'category': Feature(table, CATS, per='item', on_mask='mask')})
    win = rng.permutation(B)
    win_dev = dc._upload(win)
    event_dev, table_dev = dc._feature_sources[0][0], dc._feature_sources[1][0]
    tab = dc.windows_dev
    n_in = dc.next_item_counts(win)

    plain = DeviceCloze(items, offsets, V=V, holdout=1)            # the item rows alone, as the parent commit builds them
    rows = {'cloze': plain._batch((plain.windows, plain.windows_dev), win, win_dev, win_dev, TRAIN, 7, W)['items'],
            'next_item': plain._next_batch(ops.NEXT_TRAIN, win, win_dev, win_dev, n_in, n_in, plain._next_train()[1], 7, W, 0, None, None,
                                           None, 1)['items']}
    layouts = {'cloze': ops.FEAT_CLOZE, 'next_item': ops.FEAT_NEXT_TRAIN}
    cols = torch.arange(W, device='cuda')

    def new(name):
        return ops.batch_features(dc.items_dev, dc.offsets_dev, tab[0], tab[1], tab[2], win_dev, W, layouts[name], rows[name],
                                  dc._feature_sources, holdout=1)

    def composed(name):
        w = win_dev.long()
        g, first, L = tab[0][w].long(), tab[1][w].long(), tab[2][w].long()
        if name == 'cloze':
            n = L.clamp(0, W)
        else:
            T = (dc.offsets_dev[g + 1] - dc.offsets_dev[g] - 1).clamp(min=0)
            n = torch.where(first > 0, L, (L - 1).clamp(min=0))
            first = (first - 1).clamp(min=0)
            n = torch.minimum(n.clamp(max=W), T - first - 1).clamp(min=0)
        real = cols[None, :] < n[:, None]
        idx = torch.where(real, (dc.offsets_dev[g] + first)[:, None] + cols[None, :], 0)
        action = torch.where(real, event_dev[idx].long() + 10, 0)
        cat = table_dev[dc.items_dev[idx].long()].long() + 10
        cat = torch.where(real, torch.where(rows[name] == 1, 1, cat), 0)
        return [action, cat]

    res = {'what': 'ms per call, median [min, max] of %d rounds x %d calls, interleaved' % (a.rounds, a.iters), 'B': B, 'W': W, 'V': V,
           'features': "action: per event, kept; category: per item, masked"}
    for name in ('cloze', 'next_item'):
        x, y = new(name), composed(name)
        torch.cuda.synchronize()
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]), name
        assert bool(((x[1] == 1) == (rows[name] == 1)).all()) and not bool((x[0] == 1).any())
        del x, y
        torch.cuda.synchronize()
        out = {'masked_positions': int((rows[name] == 1).sum()), 'real_positions': int((rows[name] != 0).sum())}
        for k, f in (('batch_features', new), ('composed', composed)):
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            keep = f(name)
            torch.cuda.synchronize()
            out[k + '_peak_extra_MB'] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            del keep
        ms = {'batch_features': [], 'composed': []}
        for r in range(a.rounds + 1):
            for k, f in (('batch_features', new), ('composed', composed)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    f(name)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    ms[k].append(e0.elapsed_time(e1) / a.iters)
        out.update({k: spread(v) for k, v in ms.items()})
        out['composed_over_batch_features'] = round(out['composed'][0] / out['batch_features'][0], 2)
        res[name] = out
    # one training step of a two-feature model beside the gather
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, ClozeMaskedItemPrediction
    torch.manual_seed(1234)
    model = ClickstreamTransformer({'items': ['asin'], 'cats': ['category']},
                                   {'items': ['i%d' % i for i in range(V)], 'cats': ['c%d' % i for i in range(CATS)]},
                                   {'items': 64, 'cats': 64}, ClozeMaskedItemPrediction([], V), value_to_head='[MASK]', num_encoder_layers=2,
                                   num_attention_heads=2, dropout_rate=0.1, compute_dtype=torch.bfloat16, feature_combine='sum').cuda()
    opt = optim.Adam(model.parameters())
    step_ms, build_ms = [], []
    for s in range(a.steps + 2):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        b = dc._batch((dc.windows, dc.windows_dev), win, win_dev, win_dev, TRAIN, 7 + s, W)
        e1.record()
        opt.zero_grad()
        loss = model.cloze_loss(dc.inputs(b, 'asin'), b['labels_padded'], max_masked_per_row=dc.max_masked, n_real_tokens=b['n_real_tokens'])
        loss.backward()
        opt.step()
        e2.record()
        torch.cuda.synchronize()
        if s >= 2:
            build_ms.append(e0.elapsed_time(e1))
            step_ms.append(e1.elapsed_time(e2))
    res['train_step_cloze'] = {'model': 'bf16, items + category summed, d = 64, 2 layers, tied head', 'loss': float(loss.detach()),
                               'step_ms': spread(step_ms), 'batch_with_features_ms_in_loop': spread(build_ms),
                               'batch_features_share_of_step': round(res['cloze']['batch_features'][0] / spread(step_ms)[0], 4)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
