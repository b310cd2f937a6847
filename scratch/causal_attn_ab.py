"""Causal against bidirectional ops.attn_fwd / ops.attn_bwd ("Causal (left-to-right) self-attention"): same build,
same process, the four launches interleaved, warm.  Device events around N launches, R samples per variant; prints one JSON line per
shape with the median, p10, p90 and minimum of each variant and the causal / bidirectional ratio of the medians.

    python scratch/causal_attn_ab.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bert4clickpath_amd import input_pipeline, ops  # noqa: E402

N, R = 10, 25


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N


def case(name, lens, packed, H, dh):
    g = torch.Generator().manual_seed(1)
    B, S = len(lens), int(max(lens))
    off = np.concatenate([[0], np.cumsum(lens)])
    T, d = int(off[-1]), H * dh
    cu = torch.tensor(off, dtype=torch.int32, device='cuda') if packed else None
    qkv = (torch.randn(T, 3 * d, generator=g) * 0.8).bfloat16().cuda()
    do = torch.randn(T, d, generator=g).bfloat16().cuda()
    pad = torch.zeros(T, dtype=torch.uint8, device='cuda')
    st = {}
    for c in (False, True):
        kw = {'causal': True} if c else {}
        o, lse = ops.attn_fwd(qkv, pad, B, S, H, dh, cu, **kw)
        st[c] = (kw, o, lse)
    fns = {}
    for c in (False, True):
        kw, o, lse = st[c]
        tag = 'causal' if c else 'bidir'
        fns['fwd_' + tag] = (lambda kw=kw: ops.attn_fwd(qkv, pad, B, S, H, dh, cu, **kw))
        fns['bwd_' + tag] = (lambda kw=kw, o=o, lse=lse: ops.attn_bwd(qkv, pad, o, do, lse, B, S, H, dh, cu, **kw))
    for f in fns.values():           # warm every variant
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(R):               # interleaved
        for k, f in fns.items():
            ms[k].append(timed(f))
    out = {'case': name, 'B': B, 'S': S, 'H': H, 'dh': dh, 'tokens': T, 'packed': packed, 'launches_per_sample': N, 'samples': R}
    for k, v in ms.items():
        v = sorted(v)
        out[k] = {'median_ms': v[len(v) // 2], 'p10_ms': v[int(0.1 * (len(v) - 1))], 'p90_ms': v[int(round(0.9 * (len(v) - 1)))], 'min_ms': v[0]}
    for d_ in ('fwd', 'bwd'):
        out[d_ + '_causal_over_bidir'] = out[d_ + '_causal']['median_ms'] / out[d_ + '_bidir']['median_ms']
    print(json.dumps(out), flush=True)
    return out


def main():
    assert torch.cuda.is_available()
    b = input_pipeline.synthetic_cloze_batch(4096, 200, 50000, seed=0)          # bench.py's batch generator: its lengths
    lens = ((b['ids'] != 0).sum(1)).astype(int).tolist()
    for c in [('C2 packed (bench lengths)', lens, True, 2, 64), ('dense S=200', [200] * 4096, False, 2, 64),
              ('config 5 S=512', [512] * 512, False, 4, 64)]:
        case(*c)


if __name__ == '__main__':
    main()
