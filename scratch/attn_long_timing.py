"""The streamed attention kernels (ops.attn_long_fwd / attn_long_bwd, include/b4c.h) against what the same shapes ran on
before them: the fp32-math row kernels, reached through ops.attn_fwd / attn_bwd with ops.long_attn off (dense only: the packed layout
was refused past S = 512, so its numbers stand alone).  bf16, H = 2, dh = 64, B * H = 512, S = 1024 and 2048, dense and packed (lengths
uniform in [S / 2, S], one at S), causal and not, forward and forward + backward.  The two sides alternate inside one process, WINDOWS
windows per route, HIP events around every window; median, min and max per window.  The resident forward at S = 512 is timed beside
them for its pairs / s.  FLOPs: 4 pairs d forward, 10 pairs d backward (pairs: the (query, key) pairs the launch works on; causal:
the triangle).
usage (from the repository root): PYTHONPATH=. python scratch/attn_long_timing.py [out.json]"""
import json
import sys

import numpy as np
import torch

from bert4clickpath_amd import ops

H, DH, BH, WINDOWS = 2, 64, 512, 5
ITERS = {'long': 100, 'rows': 4, 'resident': 400}        # windows of 20 ms (the shortest forward) to 0.6 s
BF16 = torch.bfloat16


def _inputs(B, S, packed, seed):
    g = torch.Generator().manual_seed(seed)
    d = H * DH
    lens = np.full(B, S)
    if packed:
        lens = np.random.default_rng(seed).integers(S // 2, S + 1, B)
        lens[0] = S
    T = int(lens.sum())
    qkv = (torch.randn(T, 3 * d, generator=g) * 0.8).to(BF16).cuda()
    do = torch.randn(T, d, generator=g).to(BF16).cuda()
    pad = torch.zeros(T, dtype=torch.uint8, device='cuda')
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device='cuda') if packed else None
    pairs = float((lens.astype(np.float64) ** 2).sum())
    return qkv, do, pad, cu, T, pairs


def main():
    assert BH % H == 0
    B = BH // H
    d = H * DH
    routes = {}                      # name -> (callable, iters, flops per call)
    for S in (1024, 2048):
        for packed in (False, True):
            qkv, do, pad, cu, T, pairs = _inputs(B, S, packed, S + packed)
            for causal in (False, True):
                pr = (pairs + T) / 2 if causal else pairs
                tag = 'S=%d %s%s' % (S, 'packed' if packed else 'dense', ' causal' if causal else '')

                def long_fwd(qkv=qkv, pad=pad, cu=cu, S=S, causal=causal):
                    return ops.attn_long_fwd(qkv, pad, B, S, H, DH, cu=cu, causal=causal)

                def long_both(qkv=qkv, pad=pad, cu=cu, S=S, causal=causal, do=do):
                    o, lse = ops.attn_long_fwd(qkv, pad, B, S, H, DH, cu=cu, causal=causal)
                    return ops.attn_long_bwd(qkv, pad, o, do, lse, B, S, H, DH, cu=cu, causal=causal)
                routes[tag + ' | long fwd'] = (long_fwd, ITERS['long'], 4 * pr * d, pr)
                routes[tag + ' | long fwd+bwd'] = (long_both, ITERS['long'], 14 * pr * d, pr)
                if not packed:          # the parent's route: ops.attn_fwd / attn_bwd with the switch off
                    def rows_fwd(qkv=qkv, pad=pad, S=S, causal=causal):
                        return ops.attn_fwd(qkv, pad, B, S, H, DH, causal=causal)

                    def rows_both(qkv=qkv, pad=pad, S=S, causal=causal, do=do):
                        o, lse = ops.attn_fwd(qkv, pad, B, S, H, DH, causal=causal)
                        return ops.attn_bwd(qkv, pad, o, do, lse, B, S, H, DH, causal=causal)
                    routes[tag + ' | rows fwd'] = (rows_fwd, ITERS['rows'], 4 * pr * d, pr)
                    routes[tag + ' | rows fwd+bwd'] = (rows_both, ITERS['rows'], 14 * pr * d, pr)
    q5, _, pad5, _, T5, pairs5 = _inputs(B, 512, False, 512)
    routes['S=512 dense | resident fwd'] = (lambda: ops.attn_fwd(q5, pad5, B, 512, H, DH), ITERS['resident'], 4 * pairs5 * d, pairs5)
    ops.long_attn = False            # ops.attn_fwd / attn_bwd above are the parent's launches
    for f, _, _, _ in routes.values():          # warm-up: allocator, workspaces, LDS opt-in
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(WINDOWS):
        for name, (f, iters, _, _) in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / iters)
    out = {'H': H, 'dh': DH, 'B': B, 'dtype': 'bf16', 'windows': WINDOWS, 'iters': ITERS, 'device': torch.cuda.get_device_name(0), 'ms': {},
           'tflops': {}, 'pairs_per_s': {}, 'long_over_rows': {}}
    for name, t in times.items():
        t = sorted(t)
        med = t[len(t) // 2]
        out['ms'][name] = {'median': med, 'min': t[0], 'max': t[-1]}
        out['tflops'][name] = routes[name][2] / med * 1e-9
        out['pairs_per_s'][name] = routes[name][3] * H / med * 1e3           # per head
        print('%-44s %9.3f ms  [%9.3f - %9.3f]  %7.1f TFLOP/s' % (name, med, t[0], t[-1], out['tflops'][name]))
    for name in times:
        if '| rows' in name:
            lname = name.replace('| rows', '| long')
            r, l = out['ms'][name], out['ms'][lname]
            spread = max(r['max'] - r['min'], l['max'] - l['min'])
            out['long_over_rows'][name.replace(' | rows', ' |')] = {'speedup': r['median'] / l['median'], 'gain_ms': r['median'] - l['median'],
                                                                   'larger_spread_ms': spread, 'faster_by_more_than_the_spread': r['median'] - l['median'] > spread}
            print('%-44s rows / long = %.2f x (gain %.3f ms, larger spread %.3f ms)' % (lname, r['median'] / l['median'], r['median'] - l['median'], spread))
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
