"""What a training batch costs to build: input_pipeline.BeautyCloze.train_batches on the host plus the uploads
examples/beauty_hitrate.py makes (ids, compact labels, flat_idx), against cloze_batches.DeviceCloze.train_batches
(b4c_cloze_batch), and the training step the batch feeds, at the same shape.

Shapes: the committed Beauty file at B = 512 and B = 4096 (the example's model: d 64, 2 layers), and a synthetic CSR with the
C2 lengths (20 .. 197 items per training row, B = 4096, W = 197, V = 50,000; bench.py's model: d 128, 4 layers).
Per round, interleaved: `host_batches` host batches (wall clock, ending in a device synchronise), `dev_batches` device batches
(wall clock around the generator, ending in a synchronise: the permutation slicing and the token-count sum are in it), and the
same number again under ops' launch recorder (device events around the kernel alone).  Then the training step on resident
device batches (device events around windows of `step_iters` steps).  Median [min - max] over the rounds after one warm-up
round; one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bert4clickpath_amd import input_pipeline, ops, optim  # noqa: E402
from bert4clickpath_amd.cloze_batches import DeviceCloze  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return [xs[len(xs) // 2], xs[0], xs[-1]]


def host_pipeline(items, offsets, V):
    h = object.__new__(input_pipeline.BeautyCloze)             # the class reads an .npz; the synthetic CSR is handed over as arrays
    h.items, h.offsets, h.n_seq, h.V = items.astype(np.int64), offsets, len(offsets) - 1, V
    return h


def build_model(V, d, layers):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(1234)
    return ClickstreamTransformer({'items': ['asin']}, {'items': ['item%d' % i for i in range(V)]}, {'items': d},
                                  SoftMaxHead([1024, 512, 256, 128], V), value_to_head='[MASK]', num_encoder_layers=layers,
                                  num_attention_heads=2, dropout_rate=0.1, compute_dtype=torch.bfloat16).cuda()


def measure(name, items, offsets, V, B, width, d, layers, a):
    host, dev = host_pipeline(items, offsets, V), DeviceCloze(items, offsets, V=V)
    steps = 10 ** 9
    hgen, dgen = host.train_batches(B, 1, steps), dev.train_batches(B, 1, steps, width=width)

    def host_batches(n):
        t0 = time.perf_counter()
        for _ in range(n):
            b = next(hgen)
            keep = (torch.from_numpy(b['ids'])[:, 2:-1].contiguous().cuda(), torch.from_numpy(b['labels']).cuda(),
                    torch.from_numpy(b['flat_idx']).cuda())
        torch.cuda.synchronize()
        del keep
        return (time.perf_counter() - t0) * 1e3 / n

    def dev_batches(n):
        t0 = time.perf_counter()
        for _ in range(n):
            keep = next(dgen)
        torch.cuda.synchronize()
        del keep
        return (time.perf_counter() - t0) * 1e3 / n

    def dev_kernel(n):
        ops.start_recording()
        for _ in range(n):
            next(dgen)
        r = ops.stop_recording()['cloze_batch']
        return r['ms'] / r['launches']

    rows = {'host_ms': [], 'device_wall_ms': [], 'device_kernel_ms': []}
    for rnd in range(a.rounds + 1):
        got = (host_batches(a.host_batches), dev_batches(a.dev_batches), dev_kernel(a.dev_batches))
        if rnd:                                                # round 0 warms up
            for k, v in zip(rows, got):
                rows[k].append(v)
    out = {k: spread(v) for k, v in rows.items()}
    # the step these batches feed (this code is not the builder's: it is what the builder must stay below)
    model = build_model(V, d, layers)
    opt = optim.Adam(model.parameters())
    resident = [next(dgen) for _ in range(4)]

    def step(b):
        opt.zero_grad()
        loss = model.cloze_loss({'asin': b['items']}, b['labels_padded'], training=True, max_masked_per_row=b['labels_padded'].shape[1],
                                n_real_tokens=b['n_real_tokens'])
        loss.backward()
        opt.step()

    for i in range(a.step_iters):
        step(resident[i % 4])
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.step_iters):
            step(resident[i % 4])
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / a.step_iters)
    out['train_step_ms'] = spread(ms)
    out.update({'B': B, 'W': resident[0]['items'].shape[1] if width is None else width, 'n_seq': dev.n_seq, 'V': V,
                'mean_row_items': float(np.maximum(dev.lengths - 1, 0).mean()), 'model': 'd %d, %d layers, bf16' % (d, layers)})
    del model, opt, resident
    torch.cuda.empty_cache()
    return name, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--host_batches', type=int, default=4)
    ap.add_argument('--dev_batches', type=int, default=300)
    ap.add_argument('--step_iters', type=int, default=50)
    ap.add_argument('--data', default=os.path.join(ROOT, 'data', 'beauty_sequences.npz'))
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'a measurement: needs the MI355X'
    z = np.load(a.data, allow_pickle=False)
    bi, bo, bV = z['items'], z['offsets'], int(z['vocab'].shape[0])
    rng = np.random.default_rng(0)
    lens = rng.integers(21, 199, 8 * 4096)                     # 20 .. 197 items once the last is held out
    co = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ci = rng.integers(0, 50000, int(co[-1])).astype(np.int32)
    res = dict([measure('beauty_B512', bi, bo, bV, 512, None, 64, 2, a),
                measure('beauty_B4096', bi, bo, bV, 4096, None, 64, 2, a),
                measure('c2_lengths_B4096', ci, co, 50000, 4096, 197, 128, 4, a)])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
