"""Host side of the candidate lists (no GPU): the sampler's restatement (tests/candidates_ref.py) keeps its promises, the
popularity draw follows the counts, mulhi64 is the exact high half of the product, cloze.item_counts, and argument errors
are raised before any device work."""
import numpy as np
import pytest
import torch

from candidates_ref import sample_rows


def test_mulhi64_host_is_the_high_half_of_the_128_bit_product():
    from bert4clickpath_amd import ops
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.integers(0, 2 ** 64, 2000, dtype=np.uint64),
                        np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1], np.uint64)])
    for v in (1, 2, 7, 50000, 2 ** 31 - 1, 2 ** 32 + 3, 123456789012345678, 2 ** 63 - 1, 2 ** 64 - 1):
        got = ops.mulhi64_host(x, v)
        want = [(int(a) * v) >> 64 for a in x]
        assert [int(g) for g in got] == want, v


def test_host_sampler_distinct_label_free_exclusions_and_zero_counts():
    V, N = 60, 25
    rng = np.random.default_rng(3)
    labels = rng.integers(0, V, 40)
    labels[5] = -1
    labels[9] = V
    exclude = [rng.choice(V, 10, replace=False).tolist() for _ in range(40)]
    counts = rng.integers(0, 5, V)
    counts[::4] = 0
    cdf = np.cumsum(counts).astype(np.int64)
    for mode_cdf in (None, cdf):
        cand, short = sample_rows(labels, V, N, seed=11, row_base=100, exclude=exclude, cdf=mode_cdf)
        assert cand.shape == (40, N + 1)
        for r in range(40):
            if r in (5, 9):
                assert (cand[r] == -1).all()
                continue
            assert cand[r, 0] == labels[r]
            neg = cand[r, 1:][cand[r, 1:] >= 0]
            assert len(set(neg.tolist())) == len(neg)                      # distinct
            assert labels[r] not in neg                                    # never the label
            assert not set(neg.tolist()) & set(exclude[r])                 # exclusions honoured
            assert (cand[r, 1 + len(neg):] == -1).all()                    # -1 only in the tail
            if mode_cdf is not None:
                assert (counts[neg] > 0).all()                             # count 0: never drawn
        if mode_cdf is not None:       # at most 45 items of count > 0, minus 10 excluded and the label: rows may run short
            assert short == sum(1 for r in range(40) if r not in (5, 9) and (cand[r] >= 0).sum() < N + 1)


def test_host_sampler_is_a_function_of_the_global_row():
    V, N = 1000, 30
    labels = np.arange(50) * 7
    one, _ = sample_rows(labels, V, N, seed=5, row_base=0)
    a, _ = sample_rows(labels[:20], V, N, seed=5, row_base=0)
    b, _ = sample_rows(labels[20:], V, N, seed=5, row_base=20)
    assert np.array_equal(one, np.concatenate([a, b]))
    other, _ = sample_rows(labels, V, N, seed=6, row_base=0)
    assert not np.array_equal(one, other)


def test_popularity_draws_follow_the_counts_chi_square():
    """the raw draw of attempt j (before acceptance) is distributed as counts / total: a fixed-seed chi-square"""
    from bert4clickpath_amd import ops
    counts = np.array([50, 0, 1, 7, 300, 0, 25, 25, 80, 3, 0, 120, 60, 9, 2, 18], np.int64)
    cdf = np.cumsum(counts)
    n = 400000
    x = ops.rand64_host(1234, (np.uint64(17) << np.uint64(20)) + np.arange(n, dtype=np.uint64))
    items = np.searchsorted(cdf.astype(np.uint64), ops.mulhi64_host(x, int(cdf[-1])), side='right')
    got = np.bincount(items, minlength=len(counts))
    assert (got[counts == 0] == 0).all()
    nz = counts > 0
    exp = n * counts[nz] / counts.sum()
    chi2 = float(((got[nz] - exp) ** 2 / exp).sum())
    assert chi2 < 32.9, chi2          # 12 degrees of freedom: p = 0.001 at 32.9 (deterministic: fixed seed)


def test_item_counts_of_the_training_split():
    from bert4clickpath_amd import cloze
    ids = torch.tensor([[0, 0, 10, 11, 12, 1], [2, 10, 10, 3, 25, 14]])      # 0..9 reserved / padding; 25 -> item 15 >= V
    c = cloze.item_counts(ids, V=8)
    assert c.dtype == torch.int64 and c.shape == (8,)
    assert c.tolist() == [3, 1, 1, 0, 1, 0, 0, 0]
    assert cloze.item_counts(np.array([5, 6, 7]), V=3, label_offset=5).tolist() == [1, 1, 1]
    with pytest.raises(TypeError):
        cloze.item_counts(torch.zeros(3), V=4)


def test_argument_errors_before_device_work():
    from bert4clickpath_amd import cloze, ops
    from bert4clickpath_amd._lib import B4CError
    lab = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(B4CError, match='num_negatives'):
        ops.sample_candidates(lab, 100, 1024, seed=0)
    with pytest.raises(B4CError, match='int32'):
        ops.sample_candidates(lab.long(), 100, 10, seed=0)
    with pytest.raises(B4CError, match='item_cdf'):
        ops.sample_candidates(lab, 100, 10, seed=0, item_cdf=torch.zeros(99, dtype=torch.int64))
    with pytest.raises(B4CError, match='exclude'):
        ops.sample_candidates(lab, 100, 10, seed=0, exclude=torch.zeros(4, 3, dtype=torch.int64))
    h = torch.zeros(4, 64)
    wt = torch.zeros(104, 64)
    b = torch.zeros(104)
    cand = torch.zeros(4, 5, dtype=torch.int32)
    with pytest.raises(B4CError, match='K = 60'):
        ops.candidate_scores(torch.zeros(4, 60), torch.zeros(104, 60), b, cand, 100)
    with pytest.raises(B4CError, match='1 .. 1024'):
        ops.candidate_scores(h, wt, b, torch.zeros(4, 1025, dtype=torch.int32), 100)
    with pytest.raises(B4CError, match='int32'):
        ops.candidate_scores(h, wt, b, cand.long(), 100)
    with pytest.raises(B4CError, match='rows'):
        ops.candidate_scores(h, wt, b, cand[:3], 100)
    with pytest.raises(B4CError, match='wt'):
        ops.candidate_scores(h, wt.bfloat16(), b, cand, 100)
    with pytest.raises(B4CError, match='k = 17'):
        ops.candidate_scores(h, wt, b, cand, 100, k=17)
    with pytest.raises(B4CError, match='labels'):
        ops.candidate_scores(h, wt, b, cand, 100, labels=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(B4CError, match='scores'):
        ops.candidate_rank_rows(torch.zeros(4, 50), 100, cand)
    with pytest.raises(ValueError, match='num_items'):
        cloze.sample_candidates(torch.zeros(2, 3))
    with pytest.raises(ValueError, match='positive total'):
        cloze.sample_candidates(torch.zeros(2, 3), item_counts=torch.zeros(5, dtype=torch.int64))
    m = cloze.ClozeMaskedRecall(10)
    with pytest.raises(ValueError, match='candidates and exclude'):
        m.update_state(torch.zeros(2, 3), torch.zeros(2, 3, 8), exclude=[[1]], candidates=torch.zeros(6, 4, dtype=torch.int32))


def test_candidate_entry_points_refuse_bad_arguments():
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    for name in ('b4c_sample_candidates', 'b4c_candidate_score', 'b4c_candidate_rank_rows'):
        assert name in _lib.declared_symbols() and hasattr(L, name)
    assert _lib.MAX_CAND == 1024
    # N past B4C_MAX_CAND - 1, C past B4C_MAX_CAND, K not a multiple of 8: refused before any launch
    assert L.b4c_sample_candidates(None, 4, 100, 1024, 0, 0, None, 0, 0, None, None, 1025, None, None) == -1
    assert b'sample_candidates' in L.b4c_last_error()
    assert L.b4c_candidate_score(None, 64, None, 64, None, None, 2000, 4, 2000, 100, 64, 0, None, None, 0, None, 0, None, None) == -1
    assert L.b4c_candidate_score(None, 64, None, 64, None, None, 8, 4, 8, 100, 60, 0, None, None, 0, None, 0, None, None) == -1
    assert b'K = 60' in L.b4c_last_error()
    assert L.b4c_candidate_rank_rows(None, 128, 0, None, 8, 4, 8, 100, None, None, 17, None, None) == -1


def test_a_list_shared_by_every_row_is_laid_out_row_by_row():
    """expand(R, -1) gives stride(0) == 0: the kernels would read row r at r * C past the 101 ids; the helper copies it out"""
    from bert4clickpath_amd import ops
    lst = torch.arange(101, dtype=torch.int32)
    shared = lst.expand(40960, 101)
    t, ld, C = ops._cand_args(shared, 40960, 'x')
    assert C == 101 and ld >= C and t.stride(0) == ld and t.is_contiguous() and torch.equal(t, shared)
    own = torch.arange(4 * 101, dtype=torch.int32).reshape(4, 101)
    t, ld, _ = ops._cand_args(own, 4, 'x')
    assert t is own and ld == 101
    one = lst.expand(1, 101)                                   # a single row reads nothing past its ids
    t, ld, _ = ops._cand_args(one, 1, 'x')
    assert ld >= 101
    wide = torch.zeros(4, 128, dtype=torch.int32)[:, :101]     # a pitch wider than C is kept as it is
    t, ld, _ = ops._cand_args(wide, 4, 'x')
    assert t is wide and ld == 128
