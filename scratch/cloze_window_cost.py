"""Device time of b4c_cloze_batch_windows against b4c_cloze_batch on the same rows, both in isolation.

Rows: B = 4096 whole-sequence windows of 20 .. 200 training items, W = 200, V = 50,000, TRAIN, last_thr = 0 -- the two entries
write identical bits, which is checked first.  `--other_lib` names a second build of libb4c_hip.so (an earlier commit's) whose
b4c_cloze_batch is timed beside this tree's two entries.  Per round the entries take turns, `--iters` launches each between two
device events; median [min - max] of the per-launch time over the rounds after one warm-up round; one JSON line.

    python scratch/cloze_window_cost.py --other_lib /path/to/other/libb4c_hip.so"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bert4clickpath_amd import _lib  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return [round(x, 5) for x in (xs[len(xs) // 2], xs[0], xs[-1])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--other_lib', default=None)
    ap.add_argument('--B', type=int, default=4096)
    ap.add_argument('--W', type=int, default=200)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=9)
    a = ap.parse_args()
    B, W, M = a.B, a.W, 10
    rng = np.random.default_rng(5)
    lengths = rng.integers(21, W + 2, B)                            # training rows of 20 .. W items
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    items = torch.from_numpy(rng.integers(0, 50000, int(offsets[-1])).astype(np.int32)).cuda()
    offsets_d = torch.from_numpy(offsets).cuda()
    seq = torch.from_numpy(rng.permutation(B).astype(np.int32)).cuda()
    win_seq = torch.arange(B, dtype=torch.int32, device='cuda')
    win_start = torch.zeros(B, dtype=torch.int32, device='cuda')
    win_len = torch.from_numpy((lengths - 1).astype(np.int32)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    new = _lib.lib()
    entries = {}

    def batch_of(lib):
        def run(out, lab, nm):
            return lib.b4c_cloze_batch(items.data_ptr(), offsets_d.data_ptr(), seq.data_ptr(), B, W, 0, 0.4, 10, 77, out.data_ptr(), W,
                                       lab.data_ptr(), M, M, nm.data_ptr(), st)
        return run

    def windows(out, lab, nm):
        return new.b4c_cloze_batch_windows(items.data_ptr(), offsets_d.data_ptr(), win_seq.data_ptr(), win_start.data_ptr(),
                                           win_len.data_ptr(), seq.data_ptr(), B, W, 0, 0.4, 10, 77, 0, out.data_ptr(), W, lab.data_ptr(), M, M,
                                           nm.data_ptr(), st)

    if a.other_lib:
        other = ctypes.CDLL(a.other_lib)
        sig = _lib.signatures()['b4c_cloze_batch']
        other.b4c_cloze_batch.restype, other.b4c_cloze_batch.argtypes = sig
        entries['cloze_batch_other_lib'] = batch_of(other)
    entries['cloze_batch'] = batch_of(new)
    entries['cloze_batch_windows'] = windows
    bufs = {k: (torch.empty(B, W, dtype=torch.int64, device='cuda'), torch.empty(B, M, dtype=torch.float32, device='cuda'),
                torch.empty(B, dtype=torch.int32, device='cuda')) for k in entries}
    for k, f in entries.items():
        assert f(*bufs[k]) == 0, k
    torch.cuda.synchronize()
    first = bufs['cloze_batch_windows']
    same = all(all(torch.equal(x, y) for x, y in zip(first, bufs[k])) for k in entries)
    assert same, 'the entries disagree'
    ms = {k: [] for k in entries}
    for r in range(a.rounds + 1):
        for k, f in entries.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f(*bufs[k])
            e1.record()
            torch.cuda.synchronize()
            if r:                                                  # round 0 warms up
                ms[k].append(e0.elapsed_time(e1) / a.iters)
    res = {'what': 'device ms per launch, median [min, max] of %d rounds x %d launches, interleaved' % (a.rounds, a.iters),
           'B': B, 'W': W, 'tokens': int((lengths - 1).sum()), 'identical_outputs': same, 'ms': {k: spread(v) for k, v in ms.items()}}
    if a.other_lib:
        res['windows_over_other_lib'] = round(res['ms']['cloze_batch_windows'][0] / res['ms']['cloze_batch_other_lib'][0], 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
