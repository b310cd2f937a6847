"""bench.py --dump-outputs: what the last timed step computed goes to DIR/<name>.npy -- the loss (float64), every parameter and
its gradient (float32) -- within 64 MB; larger tensors as a sample whose positions depend on the name and size only, so that
two runs (two builds) with the same arguments write the same elements."""
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _model(vocab):
    argv = sys.argv
    sys.argv = ['bench.py', '--vocab', str(vocab)]
    try:
        a = bench.parse()
    finally:
        sys.argv = argv
    m = bench.build_model(a, 'cpu')
    g = torch.Generator().manual_seed(5)
    for p in m.parameters():
        p.grad = torch.randn(p.shape, generator=g)
    return m


def _files(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_of_the_default_workload_fits_the_budget_and_repeats(tmp_path):
    m = _model(50000)        # parameters + gradients: 107 MB, sampled down
    w1 = bench.dump_outputs(str(tmp_path / 'a'), m, torch.tensor(2.5))
    w2 = bench.dump_outputs(str(tmp_path / 'b'), m, torch.tensor(2.5))
    a, b = _files(str(tmp_path / 'a')), _files(str(tmp_path / 'b'))
    assert w1 == w2 and sorted(a) == sorted(b) and len(a) == 1 + 2 * len(list(m.parameters()))
    assert sum(os.path.getsize(str(tmp_path / 'a' / f)) for f in a) <= bench.DUMP_BUDGET_BYTES
    assert a['loss.npy'].dtype == np.float64 and a['loss.npy'].shape == () and float(a['loss.npy']) == 2.5
    # the per-tensor cap is the largest that fits: one element more per sampled tensor would not
    room = bench.DUMP_BUDGET_BYTES - 128 * len(a)
    numel = {n: p.numel() for n, p in m.named_parameters()}
    sizes = [1 * 8] + [v * 4 for v in numel.values()] * 2
    cap = max(x.size for f, x in a.items() if f != 'loss.npy' and x.size < numel[f.split('.', 1)[1][:-4]])
    assert 8 + 2 * sum(min(v, cap) * 4 for v in numel.values()) <= room < 8 + 2 * sum(min(v, cap + 1) * 4 for v in numel.values())
    assert sum(sizes) > room
    sampled = 0
    for n, p in m.named_parameters():
        for kind, t in (('param.', p.detach()), ('grad.', p.grad)):
            x = a[kind + n + '.npy']
            assert x.dtype == np.float32 and np.array_equal(x, b[kind + n + '.npy'])
            flat = t.reshape(-1).numpy()
            if flat.size <= cap:
                assert np.array_equal(x, flat)
            else:               # the elements at the positions drawn from the name's seed, in order of position
                pos = np.random.default_rng(zlib.crc32((kind + n).encode())).choice(flat.size, cap, replace=False)
                pos.sort()
                assert np.array_equal(x, flat[pos])
                sampled += 1
    assert sampled == 4         # the item table and the vocabulary projection, parameter and gradient


def test_dump_of_a_small_model_is_whole(tmp_path):
    m = _model(1000)
    w = bench.dump_outputs(str(tmp_path), m, torch.tensor(1.0))
    assert all(w['param.' + n] == p.numel() and w['grad.' + n] == p.numel() for n, p in m.named_parameters())
    f = _files(str(tmp_path))
    assert all(np.array_equal(f['param.' + n + '.npy'], p.detach().reshape(-1).numpy()) for n, p in m.named_parameters())
