"""Host side of the exclusion lists (no GPU): cloze.seen_items on an evaluation batch, argument checks of ops.exclusions and of
the *_excl entry points of the library."""
import os

import numpy as np
import pytest
import torch


def test_seen_items_of_a_beauty_eval_batch(tmp_path):
    from bert4clickpath_amd import cloze, input_pipeline
    items = np.array([5, 7, 9, 2, 2, 4, 11, 0, 3], np.int64)                 # label-space item indices
    offsets = np.array([0, 3, 6, 9], np.int64)
    path = os.path.join(str(tmp_path), 'beauty.npz')
    np.savez(path, items=items, offsets=offsets, vocab=np.array(['i%d' % i for i in range(12)]))
    data = input_pipeline.BeautyCloze(path)
    batch = next(iter(data.eval_batches(3)))
    ids = batch['ids'] if isinstance(batch, dict) else batch[0]
    ids = torch.as_tensor(np.asarray(ids))
    seen = cloze.seen_items(ids)
    assert seen.shape == ids.shape and seen.dtype == torch.int64
    ids_n, seen_n = ids.numpy(), seen.numpy()
    assert np.array_equal(seen_n[ids_n >= 10], ids_n[ids_n >= 10] - 10)
    assert (seen_n[ids_n < 10] == -1).all()                                   # [PAD], [MASK], [CLS], [SEP] drop out
    for b in range(3):                                                        # the history: the sequence's items but the held-out one
        got = set(seen_n[b][seen_n[b] >= 0].tolist())
        assert got <= set(items[offsets[b]:offsets[b + 1]].tolist()) and got
    with pytest.raises(TypeError):
        cloze.seen_items(torch.zeros(2, 3))


def test_exclusions_checks_its_arguments():
    from bert4clickpath_amd import ops
    from bert4clickpath_amd._lib import B4CError
    with pytest.raises(B4CError, match='shape'):
        ops.exclusions(torch.zeros(4, dtype=torch.int32), 100)
    with pytest.raises(B4CError, match='integer'):
        ops.exclusions(torch.zeros(4, 3), 100)
    with pytest.raises(B4CError, match='at most'):
        ops.exclusions(torch.zeros(2, 1025, dtype=torch.int64), 100)


def test_excl_entry_points_refuse_bad_arguments():
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    assert 'b4c_exclusions_prep' in _lib.declared_symbols() and 'b4c_topk_rows_excl' in _lib.declared_symbols()
    for name in ('b4c_exclusions_prep', 'b4c_vocab_rank_excl', 'b4c_vocab_topk_excl', 'b4c_topk_rows_excl'):
        assert hasattr(L, name)
    # E beyond B4C_MAX_EXCL, and a list without a pointer: refused before any launch
    assert L.b4c_exclusions_prep(None, 2000, 4, 2000, 100, None, None, None) == -1
    assert b'exclusions_prep' in L.b4c_last_error()
    assert L.b4c_topk_rows_excl(None, 8, 1, 8, 1, None, None, None, None, None, 0, None, 8, 4, None) == -1
    assert L.b4c_vocab_rank_excl(None, 64, None, 64, None, None, None, None, 0, 1, 8, 64, None, 0, 4, None) == -1
    assert L.b4c_vocab_topk_excl(None, 64, None, 64, None, 5, None, None, None, None, None, None, 0, 1, 8, 64, None, 0, 2000,
                                 None) == -1
    assert b'vocab_topk_excl' in L.b4c_last_error()
