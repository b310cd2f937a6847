"""DeviceCloze.views at the C2 shape (B = 4096, W = 197, two views; the three-op mix and same_target) beside next_item_window_batch
in the same process, and one contrastive_loss step (forward + backward, 4-layer d_model = 128 bf16 causal model) with a device view
on the padding-free layout against the same view with n_real_tokens_b=None, the two alternating.  WINDOWS windows of ITERS calls
each, HIP events around every window and the host clock beside them (the builders' calls are host-bound).
usage: python scratch/views_timing.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, W, V, N_SEQ = 4096, 197, 50000, 16384
WARM, ITERS, WINDOWS = 5, 20, 5


def timed(fn):
    """median / min / max over WINDOWS windows of ITERS calls, device events: ms per call; and the host wall time per call"""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(ITERS):
            fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / ITERS)
        ev.append(a.elapsed_time(b) / ITERS)
    return {'median': float(np.median(ev)), 'min': float(min(ev)), 'max': float(max(ev)), 'wall_median': float(np.median(wall))}


def main():
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    rng = np.random.default_rng(0)
    lengths = rng.integers(22, 201, size=N_SEQ)                  # next-item rows of 20 .. 197 inputs: about 56 % of B W real
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    items = rng.integers(0, V, size=int(offsets[-1])).astype(np.int32)
    dc = DeviceCloze(items, offsets, V=V, max_len=W, holdout=2)
    batch = next(iter(dc.next_item_batches(B, 7, 1, width=W)))
    win = batch['win_idx'].cpu().numpy().astype(np.int64)
    out = {'B': B, 'W': W, 'V': V, 'real_share_of_BW': (batch['n_real_tokens'] - 3 * B) / (B * W), 'warmup': WARM, 'iters': ITERS,
           'windows': WINDOWS, 'device': torch.cuda.get_device_name(0), 'ms': {}}
    ms = out['ms']
    t0 = time.perf_counter()
    dc.target_index()
    out['same_target_index_build_s'] = time.perf_counter() - t0
    ms['next_item_window_batch (no negatives)'] = timed(lambda: dc.next_item_window_batch(win, seed=3, width=W))
    ms['views crop,mask,reorder x2'] = timed(lambda: dc.views(batch, 11, n_views=2))
    ms['views same_target x2'] = timed(lambda: dc.views(batch, 11, ops='same_target', n_views=2))
    ms['views same_target x1'] = timed(lambda: dc.views(batch, 11, ops='same_target', n_views=1))
    ms['next_item_window_batch (no negatives), again'] = timed(lambda: dc.next_item_window_batch(win, seed=3, width=W))
    t0 = time.perf_counter()
    for _ in range(20):
        dc.view_lengths(win, 11, n_views=2, width=W)
    out['host_view_lengths_ms'] = (time.perf_counter() - t0) * 1e3 / 20

    torch.manual_seed(0)
    d = 128
    model = ClickstreamTransformer({'items': ['asin']}, {'items': ['item%d' % i for i in range(V)]}, {'items': d}, SoftMaxHead([64, d], V),
                                   value_to_head='[MASK]', num_encoder_layers=4, num_attention_heads=2, dropout_rate=0.0,
                                   compute_dtype=torch.bfloat16, attention='causal').to('cuda')
    inputs = model._next_item_inputs(batch)
    for kind in ('crop,mask,reorder', 'same_target'):
        view = dc.views(batch, 11, ops=tuple(kind.split(',')), n_views=1)[0]
        vin = {'asin': view['items']}
        out['view_real_share_of_BW ' + kind] = (view['n_real_tokens'] - 3 * B) / (B * W)

        def step(nb):
            model.zero_grad(set_to_none=True)
            loss = model.contrastive_loss(inputs, vin, temperature=0.5, n_real_tokens=batch['n_real_tokens'], n_real_tokens_b=nb)
            loss.backward()
            return loss
        la, lb = float(step(view['n_real_tokens']).detach()), float(step(None).detach())
        out['loss packed / dense ' + kind] = [la, lb]
        res = {}
        for rep in range(2):                                     # alternate the two
            res.setdefault('packed', []).append(timed(lambda: step(view['n_real_tokens'])))
            res.setdefault('dense', []).append(timed(lambda: step(None)))
        ms['contrastive step fwd+bwd, view packed (%s)' % kind] = res['packed']
        ms['contrastive step fwd+bwd, view dense (%s)' % kind] = res['dense']
        out['dense_over_packed ' + kind] = float(np.median([r['median'] for r in res['dense']]) / np.median([r['median'] for r in res['packed']]))
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
