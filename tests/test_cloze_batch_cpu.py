"""Host side of the device-built Cloze batches (no GPU): the header declares the two entry points and the library exports
them at the pinned ABI version, the masking rule on the host (b4c_cloze_choose -- the kernel's own __host__ __device__ rule) equals its numpy
restatement (tests/cloze_batch_ref.py), the draw is uniform within 4 sigma, argument errors are refused before any launch, and
DeviceCloze's host arithmetic: token counts, the epoch permutation and its rank slices, ValueErrors."""
import numpy as np
import pytest
import torch

import abi_pin
import cloze_batch_ref as ref

SEEDS = (0, 1234, 2 ** 63 + 12345)
GS = (0, 7, 2 ** 31 + 5, 2 ** 54 - 1)
LS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1021)


def test_header_declares_and_library_exports_both_entry_points_at_abi_12():
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    sig = _lib.signatures()
    for name in ('b4c_cloze_batch', 'b4c_cloze_choose'):
        assert name in sig and hasattr(L, name)
    assert len(sig['b4c_cloze_batch'][1]) == 16 and len(sig['b4c_cloze_choose'][1]) == 5
    assert _lib.ABI_VERSION == abi_pin.ABI_VERSION and L.b4c_abi_version() == abi_pin.ABI_VERSION


def test_the_restatements_n_masked_equals_the_pipelines():
    """the header's expression for n, restated in numpy float32 (tests/cloze_batch_ref.py), against input_pipeline.n_masked for
    every L the kernel takes.  This pins the restatement, not the library: the kernel's own n is compared with the restatement
    bit for bit in tests/test_gpu_cloze_batch.py (n_masked and the label columns)."""
    from bert4clickpath_amd import input_pipeline
    for L in range(0, 1100):
        c = min(max(int(np.float32(L) * np.float32(0.4)), 0), 10)
        assert c == input_pipeline.n_masked(L) == ref.n_masked(L)


@pytest.mark.parametrize('L', LS)
def test_choose_host_equals_the_restatement(L):
    from bert4clickpath_amd import ops
    for n in sorted({0, 1, min(L, 10), L}):
        for seed in SEEDS:
            for g in GS:
                got = ops.cloze_choose_host(seed, g, L, n)
                assert got.dtype == np.int32 and got.shape == (n,)
                assert (np.diff(got) > 0).all() and (n == 0 or (got[0] >= 0 and got[-1] < L))      # strictly ascending, in range
                assert np.array_equal(got, ref.choose(seed, g, L, n)), (L, n, seed, g)


def test_choose_host_depends_on_seed_and_sequence():
    from bert4clickpath_amd import ops
    a = ops.cloze_choose_host(5, 3, 200, 10)
    assert np.array_equal(a, ops.cloze_choose_host(5, 3, 200, 10))
    assert not np.array_equal(a, ops.cloze_choose_host(6, 3, 200, 10))
    assert not np.array_equal(a, ops.cloze_choose_host(5, 4, 200, 10))


@pytest.mark.parametrize('L,n,E,g,seed', [(20, 8, 2000, 7, 1234), (5, 2, 2000, 0, 1), (197, 10, 4000, 12345, 99)])
def test_every_position_is_masked_equally_often_within_4_sigma(L, n, E, g, seed):
    """E epochs with the epoch seeds rand64_host(seed, e): position p is masked E n / L times, sigma = sqrt(E (n/L)(1 - n/L)).
    The restatement's own worst deviation at these (fixed) arguments is 1.41, 1.78 and 2.81 sigma."""
    from bert4clickpath_amd import ops
    count = np.zeros(L, np.int64)
    for e in range(E):
        count[ops.cloze_choose_host(int(ops.rand64_host(seed, e)), g, L, n)] += 1
    q = n / L
    dev = np.abs(count - E * q).max() / np.sqrt(E * q * (1 - q))
    print('L = %d n = %d E = %d: worst deviation %.2f sigma' % (L, n, E, dev))
    assert count.sum() == E * n
    assert dev < 4.0, dev


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    EINVAL = -1

    def batch(B=4, W=8, mode=0, pct=0.4, mm=10, ld_items=None, ld_lab=None, M=10):
        return L.b4c_cloze_batch(None, None, None, B, W, mode, pct, mm, 0, None, W if ld_items is None else ld_items, None,
                                 M if ld_lab is None else ld_lab, M, None, None)

    for kw, word in ((dict(W=0), b'W = 0'), (dict(W=1022), b'W = 1022'), (dict(M=9), b'max_masked'), (dict(M=65, mm=65), b'M = 65'),
                     (dict(mode=2), b'mode 2'), (dict(mode=1, M=0), b'M = 0'), (dict(ld_items=7), b'ld_items'), (dict(ld_lab=9), b'ld_lab'),
                     (dict(pct=1.5), b'masked_percentage'), (dict(B=-1), b'B = -1'), (dict(), b'null pointer')):
        assert batch(**kw) == EINVAL, kw
        assert word in L.b4c_last_error(), (kw, L.b4c_last_error())
    assert batch(B=0) == 0                                     # a no-op, pointers not looked at
    pos = np.zeros(4, np.int32)
    for args in ((0, 0, 1022, 0), (0, 0, 3, 4), (0, 0, 3, -1), (0, -1, 3, 1), (0, 2 ** 54, 3, 1)):
        assert L.b4c_cloze_choose(*args, pos.ctypes.data) == EINVAL, args
        assert b'cloze_choose' in L.b4c_last_error()
    assert L.b4c_cloze_choose(0, 0, 0, 0, None) == 0


def test_ops_cloze_batch_checks_its_arguments_before_device_work():
    from bert4clickpath_amd import ops
    from bert4clickpath_amd._lib import B4CError
    items, offsets, seq = torch.zeros(6, dtype=torch.int32), torch.tensor([0, 2, 6]), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(B4CError, match='items'):
        ops.cloze_batch(items.long(), offsets, seq, 4, ops.CLOZE_TRAIN, 0)
    with pytest.raises(B4CError, match='offsets'):
        ops.cloze_batch(items, offsets.int(), seq, 4, ops.CLOZE_TRAIN, 0)
    with pytest.raises(B4CError, match='seq_idx'):
        ops.cloze_batch(items, offsets, seq.long(), 4, ops.CLOZE_TRAIN, 0)
    for W in (0, 1022):
        with pytest.raises(B4CError, match='W = %d' % W):
            ops.cloze_batch(items, offsets, seq, W, ops.CLOZE_TRAIN, 0)
    with pytest.raises(B4CError, match='mode 2'):
        ops.cloze_batch(items, offsets, seq, 4, 2, 0)
    with pytest.raises(B4CError, match='M = 9'):
        ops.cloze_batch(items, offsets, seq, 4, ops.CLOZE_TRAIN, 0, M=9)
    with pytest.raises(B4CError, match='M = 65'):
        ops.cloze_batch(items, offsets, seq, 4, ops.CLOZE_TRAIN, 0, M=65)
    with pytest.raises(B4CError, match='CPU tensor'):
        ops.cloze_batch(items, offsets, seq, 4, ops.CLOZE_TRAIN, 0)


# ---- DeviceCloze, host side ---------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 5, 9, 3, 7, 26, 27, 4, 6, 11, 2, 8, 5, 30, 1, 12, 3, 4, 10, 6, 7]      # 23 sequences


@pytest.fixture(scope='module')
def host_data():
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    items, offsets = ref.synthetic_csr(LENGTHS, 50, seed=2)
    d = DeviceCloze(items, offsets, V=50, device=None)
    d.items_host = items
    return d


def test_n_real_tokens_is_the_row_lengths_plus_three_specials(host_data):
    seq = [3, 0, 7, 7, 1]
    n = np.array([LENGTHS[g] for g in seq])
    assert host_data.n_real_tokens(seq, 'train') == int(np.maximum(n - 1, 0).sum()) + 3 * len(seq) == 4 + 0 + 25 + 25 + 0 + 15
    assert host_data.n_real_tokens(seq, 'eval') == int(n.sum()) + 3 * len(seq)
    assert host_data.n_real_tokens([], 'eval') == 0
    # what the model counts: the non-pad ids of the chained (B, W + 3) batch of the restatement
    out, _, _ = ref.batch(host_data.items_host, host_data.offsets, seq, 25, ref.TRAIN, seed=4)
    assert host_data.n_real_tokens(seq, 'train') == int((out != 0).sum()) + 3 * len(seq)


def test_rank_slices_of_world_2_concatenate_to_the_world_1_batch_of_twice_the_size(host_data):
    d = host_data
    for epoch in (0, 1):
        order = d.epoch_order(9, epoch)
        assert np.array_equal(order, np.random.default_rng([9, epoch]).permutation(d.n_seq))
        o1, one = d.rank_slices(8, 9, epoch)                       # world 1, batch 8: 2 full batches of 23, 7 dropped
        oa, a = d.rank_slices(4, 9, epoch, rank=0, world=2)
        ob, b = d.rank_slices(4, 9, epoch, rank=1, world=2)
        assert np.array_equal(o1, order) and np.array_equal(oa, order) and np.array_equal(ob, order)
        assert one == [(0, 8), (8, 16)] and len(a) == len(b) == 2
        for (lo, hi), (la, ha), (lb, hb) in zip(one, a, b):
            assert np.array_equal(order[lo:hi], np.concatenate([order[la:ha], order[lb:hb]]))
    assert not np.array_equal(d.epoch_order(9, 0), d.epoch_order(9, 1))
    assert d.rank_slices(23, 9, 0)[1] == [(0, 23)] and d.rank_slices(24, 9, 0)[1] == []
    with pytest.raises(ValueError, match='rank'):
        d.rank_slices(4, 9, 0, rank=2, world=2)


def test_value_errors(host_data):
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    with pytest.raises(ValueError, match='2\\*\\*24'):
        DeviceCloze(np.zeros(3, np.int32), np.array([0, 3]), V=2 ** 24 + 1, device=None)
    DeviceCloze(np.zeros(3, np.int32), np.array([0, 3]), V=2 ** 24, device=None)
    with pytest.raises(ValueError, match='shorter than a row'):
        host_data.batch([7, 3], 'train', width=24)                 # sequence 7: 26 items, 25 in TRAIN
    with pytest.raises(ValueError, match='shorter than a row'):
        host_data.batch([7, 3], 'eval', width=25)
    with pytest.raises(ValueError, match='outside'):
        host_data.batch([23], 'train')
    with pytest.raises(ValueError, match='outside'):
        DeviceCloze(np.array([0, 5, 2], np.int32), np.array([0, 3]), V=5, device=None)
    with pytest.raises(ValueError, match='offsets'):
        DeviceCloze(np.zeros(3, np.int32), np.array([0, 2]), device=None)


def test_a_host_only_object_refuses_to_build_batches(host_data):
    for gen in (host_data.train_batches(4, 0, 1), host_data.eval_batches(4)):
        with pytest.raises(ValueError, match='device=None'):
            next(gen)
    with pytest.raises(ValueError, match='device=None'):
        host_data.batch([1, 2], 'train')


def test_from_npz_reads_the_committed_beauty_file():
    import os
    from bert4clickpath_amd import input_pipeline
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'data', 'beauty_sequences.npz')
    d = DeviceCloze.from_npz(path, device=None)
    b = input_pipeline.BeautyCloze(path)
    assert d.n_seq == b.n_seq and d.V == b.V and d.max_masked == 10
    first = next(b.eval_batches(64, 64))
    assert d.n_real_tokens(np.arange(64), 'eval') == int((first['ids'] != 0).sum())
