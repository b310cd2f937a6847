"""The paper's data protocol on the device (include/b4c.h "Cloze batches over windows": b4c_cloze_batch_windows,
b4c_cloze_history; cloze_batches.DeviceCloze(max_len=, stride=, holdout=, last_item_rate=)) against the host restatement of
tests/cloze_window_ref.py, bit for bit: explicit windows, the training epochs and both evaluation splits on data sets whose
lengths sit on every boundary of the window rule and of the kernel, whole-sequence windows against b4c_cloze_batch, independence
of the batch split, the history lists against numpy and against cloze.seen_items in the ranking metrics, and the batches through
a tiny model."""
import numpy as np
import pytest
import torch

import cloze_window_ref as ref

pytestmark = pytest.mark.gpu

V = 500
SENTINEL_I, SENTINEL_F = -77, -55.5
# (W = max_len, stride); 1021: the thread-count edges (256, 257) and the row without a pad column
CONFIGS = [(4, 3), (7, 1), (50, 50), (1021, 1021)]
RATE = 0.25


def _lengths(W, stride, holdout):
    """the training views on every boundary of the window rule, then an empty sequence and one of a single item: too short to
    have the targets"""
    if W == 1021:
        return [n + holdout for n in (0, 1, 256, 257, 1021, 1022)] + [0, 1]
    return [n + holdout for n in (0, 1, 2, 3, W - 1, W, W + 1, W + 2, W + stride, 2 * W, 2 * W + 1, 3 * W + 5)] + [0, 1]


def _host(t):
    return t.cpu().numpy()


_cache = {}


def _data(W, stride, holdout, rate=RATE):
    """(DeviceCloze, items, offsets) of the configuration, built once"""
    key = (W, stride, holdout, rate)
    if key not in _cache:
        from bert4clickpath_amd.cloze_batches import DeviceCloze
        items, offsets = ref.synthetic_csr(_lengths(W, stride, holdout), V, seed=11 + W)
        _cache[key] = (DeviceCloze(items, offsets, V=V, max_len=W, stride=stride, holdout=holdout, last_item_rate=rate), items, offsets)
    return _cache[key]


def _triples(table, rows):
    return [(-1, 0, 0) if w < 0 else (int(table.seq[w]), int(table.start[w]), int(table.len[w])) for w in rows]


def _pick(n, B):
    """B of n indices in a shuffled order, one named twice when B > 1"""
    rng = np.random.default_rng(B)
    if B == 1:
        return np.array([n - 1])
    rows = rng.permutation(n)[:B - 1]
    return np.insert(rows, len(rows) // 2, rows[0])


def _assert_batch(got, want, B, W, M):
    want_items, want_lab, want_n = want
    assert got['items'].dtype == torch.int64 and got['labels_padded'].dtype == torch.float32 and got['n_masked'].dtype == torch.int32
    assert got['items'].shape == (B, W) and got['labels_padded'].shape == (B, M)
    assert np.array_equal(_host(got['items']), want_items)
    assert np.array_equal(_host(got['labels_padded']), want_lab)
    assert np.array_equal(_host(got['n_masked']), want_n)
    assert got['n_real_tokens'] == int((want_items != 0).sum()) + 3 * B


@pytest.mark.parametrize('holdout', [1, 2])
@pytest.mark.parametrize('B', [1, 7, 'all'])
@pytest.mark.parametrize('W,stride', CONFIGS)
def test_window_batches_equal_the_restatement_bit_for_bit(W, stride, B, holdout):
    data, items, offsets = _data(W, stride, holdout)
    seq, start, length = ref.window_table(_lengths(W, stride, holdout), W, stride, holdout)
    assert data.n_windows == len(seq) and all(np.array_equal(a, b) for a, b in zip(data.windows, (seq, start, length)))
    B = min(7, data.n_windows + 1) if B == 7 else (data.n_windows + 1 if B == 'all' else B)
    rows = _pick(data.n_windows, B)
    assert len(rows) == B
    seed = 0x9E3779B97F4A7C15 + B                                  # >= 2^63
    for width in (None, min(W + 13, 1021)):
        got = data.window_batch(rows, seed=seed, width=width)
        Wb = max(int(length[rows].max()), 1) if width is None else width
        want = ref.batch(items, offsets, _triples(data.windows, rows), Wb, ref.TRAIN, seed, last_thr=data.last_thr)
        _assert_batch(got, want, B, Wb, 10)
        assert np.array_equal(_host(got['seq_idx']), seq[rows]) and np.array_equal(_host(got['win_idx']), rows)
    if B > 1:                                                      # the window named twice: identical rows
        vals, count = np.unique(rows, return_counts=True)
        r0, r1 = np.flatnonzero(rows == vals[count == 2][0])
        assert torch.equal(got['items'][r0], got['items'][r1]) and torch.equal(got['labels_padded'][r0], got['labels_padded'][r1])
    if B == data.n_windows + 1 and W != 1021:                      # tens of windows: last-only and ordinary rows are both present
        n = _host(got['n_masked'])
        last = np.array([ref.last_only(seed, *t, data.last_thr) for t in _triples(data.windows, rows)])
        assert last.any() and not last.all() and (n[last] == 1).all()


@pytest.mark.parametrize('holdout', [1, 2])
@pytest.mark.parametrize('W,stride', CONFIGS)
def test_train_batches_equal_the_restatement(W, stride, holdout):
    from bert4clickpath_amd import ops
    data, items, offsets = _data(W, stride, holdout)
    bs = 1 if W == 1021 else 5
    per_epoch = data.n_windows // bs
    seen = []
    for step, b in enumerate(data.train_batches(bs, 21, 2 * per_epoch, width=W)):
        e = step // per_epoch
        order = np.random.default_rng([21, e]).permutation(data.n_windows)
        rows = order[(step % per_epoch) * bs:(step % per_epoch + 1) * bs]
        want = ref.batch(items, offsets, _triples(data.windows, rows), W, ref.TRAIN, int(ops.rand64_host(21, e)), last_thr=data.last_thr)
        _assert_batch(b, want, bs, W, 10)
        assert np.array_equal(_host(b['win_idx']), rows) and np.array_equal(_host(b['seq_idx']), data.windows.seq[rows])
        seen.append(rows)
    assert len(seen) == 2 * per_epoch
    assert len(np.unique(np.concatenate(seen[:per_epoch]))) == per_epoch * bs      # a permutation: no window twice in an epoch


@pytest.mark.parametrize('split', ['test', 'valid'])
@pytest.mark.parametrize('holdout', [1, 2])
@pytest.mark.parametrize('W,stride', CONFIGS)
def test_eval_batches_of_both_splits_equal_the_restatement(W, stride, holdout, split):
    data, items, offsets = _data(W, stride, holdout)
    if split == 'valid' and holdout == 1:
        with pytest.raises(ValueError, match='valid'):
            next(data.eval_batches(4, split='valid'))
        return
    lengths = _lengths(W, stride, holdout)
    wins = [(g,) + ref.eval_window(n, split, W) for g, n in enumerate(lengths)]
    t = np.array(lengths) - (2 if split == 'valid' else 1)
    for bs in (1, 7, len(lengths)):
        got = list(data.eval_batches(bs, width=W, split=split))
        assert len(got) == -(-len(lengths) // bs)
        for i, b in enumerate(got):
            w = wins[i * bs:(i + 1) * bs]
            _assert_batch(b, ref.batch(items, offsets, w, W, ref.EVAL, 0), len(w), W, 1)
            assert np.array_equal(_host(b['seq_idx']), np.arange(i * bs, i * bs + len(w)))
    whole = _host(got[0]['labels_padded'])[:, 0]                   # the label is the split's target; -1 where there is none
    want = np.array([items[offsets[g] + t[g]] if t[g] >= 0 else -1 for g in range(len(lengths))], np.float32)
    assert np.array_equal(whole, want) and np.array_equal(_host(got[0]['n_masked']), (t >= 0).astype(np.int32))
    some = np.array([len(lengths) - 1, 0, 3, 3])                   # batch(): any order, repeats
    b = data.batch(some, 'eval', split=split)
    Wb = max(max(wins[g][2] for g in some), 1)
    _assert_batch(b, ref.batch(items, offsets, [wins[g] for g in some], Wb, ref.EVAL, 0), 4, Wb, 1)


def test_batch_train_takes_the_sequences_of_one_window_and_refuses_the_others():
    data, items, offsets = _data(7, 1, 2)
    lengths = _lengths(7, 1, 2)
    one = [g for g, n in enumerate(lengths) if n - 2 <= 7]
    seq = np.array(one + one[1:2])
    got = data.batch(seq, 'train', seed=5, width=9)
    wins = [(g, 0, lengths[g] - 2) if lengths[g] > 2 else (-1, 0, 0) for g in seq]
    _assert_batch(got, ref.batch(items, offsets, wins, 9, ref.TRAIN, 5, last_thr=data.last_thr), len(seq), 9, 10)
    assert np.array_equal(_host(got['seq_idx']), seq)
    with pytest.raises(ValueError, match='training windows'):
        data.batch([one[0], lengths.index(7 + 1 + 2)], 'train')


@pytest.mark.parametrize('mode', [ref.TRAIN, ref.EVAL])
def test_a_wider_pitch_null_row_win_and_negative_rows(mode):
    """through the library: columns past W and label columns past M keep their sentinel, row_win NULL names window b, a negative
    entry is an empty row, win_len is cut at W, n_masked_out may be NULL"""
    from bert4clickpath_amd import _lib
    data, items, offsets = _data(50, 50, 1)
    n_win, W, M, ld_i, ld_l = data.n_windows, 20, 10 if mode == ref.TRAIN else 1, 27, 13
    ws, wa, wl = data.windows_dev
    st = torch.cuda.current_stream().cuda_stream
    thr = 1 << 22

    def run(row_win, B, nm_out=True):
        out = torch.full((B, ld_i), SENTINEL_I, dtype=torch.int64, device='cuda')
        lab = torch.full((B, ld_l), SENTINEL_F, dtype=torch.float32, device='cuda')
        nm = torch.full((B + 2,), SENTINEL_I, dtype=torch.int32, device='cuda')
        _lib.check(_lib.lib().b4c_cloze_batch_windows(data.items_dev.data_ptr(), data.offsets_dev.data_ptr(), ws.data_ptr(), wa.data_ptr(),
                                                      wl.data_ptr(), None if row_win is None else row_win.data_ptr(), B, W, mode, 0.4, 10,
                                                      77, thr, out.data_ptr(), ld_i, lab.data_ptr(), ld_l, M,
                                                      nm.data_ptr() if nm_out else None, st), 'cloze_batch_windows')
        return _host(out), _host(lab), _host(nm)

    rows = np.concatenate([[-1], np.arange(n_win)[::-1], [-5]])
    for row_win, names in ((None, np.arange(n_win)), (torch.from_numpy(rows.astype(np.int32)).cuda(), rows)):
        B = len(names)
        out, lab, nm = run(row_win, B)
        want_items, want_lab, want_n = ref.batch(items, offsets, _triples(data.windows, names), W, mode, 77, last_thr=thr)
        assert np.array_equal(out[:, :W], want_items) and (out[:, W:] == SENTINEL_I).all()
        assert np.array_equal(lab[:, :M], want_lab) and (lab[:, M:] == SENTINEL_F).all()
        assert np.array_equal(nm[:B], want_n) and (nm[B:] == SENTINEL_I).all()
        out2, _, nm2 = run(row_win, B, nm_out=False)
        assert np.array_equal(out2, out) and (nm2 == SENTINEL_I).all()
    assert (want_items[0] == 0).all() and want_n[0] == 0 and (data.windows.len > W).any()


@pytest.mark.parametrize('mode', [ref.TRAIN, ref.EVAL])
def test_whole_sequence_windows_equal_cloze_batch_bit_for_bit(mode):
    from bert4clickpath_amd import ops
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    lengths = [0, 1, 2, 3, 4, 5, 6, 26, 27, 64, 65, 66, 257, 258, 1021, 7, 30, 129, 200, 513, 1022 if mode == ref.TRAIN else 1000]
    items, offsets = ref.synthetic_csr(lengths, V, seed=3)
    data = DeviceCloze(items, offsets, V=V)
    assert data.n_windows == data.n_seq and data.last_thr == 0
    n = np.array(lengths)
    table = [torch.arange(len(n), dtype=torch.int32, device='cuda'), torch.zeros(len(n), dtype=torch.int32, device='cuda'),
             torch.from_numpy((np.maximum(n - 1, 0) if mode == ref.TRAIN else n).astype(np.int32)).cuda()]
    seq = torch.from_numpy(np.random.default_rng(1).permutation(len(n)).astype(np.int32)).cuda()
    for seed, pct, mm in ((5, 0.4, 10), (2 ** 63 + 9, 1.0, 64), (0, 0.2, 3)):
        old = ops.cloze_batch(data.items_dev, data.offsets_dev, seq, 1021, mode, seed, pct, mm)
        new = ops.cloze_batch_windows(data.items_dev, data.offsets_dev, *table, seq, 1021, mode, seed, pct, mm, last_thr=0)
        assert all(torch.equal(a, b) for a, b in zip(old, new)), (seed, pct, mm)
    # DeviceCloze with the default arguments goes through the windowed entry and gives the same rows
    b = data.batch(_host(seq), mode, seed=5, width=1021)
    old = ops.cloze_batch(data.items_dev, data.offsets_dev, seq, 1021, mode, 5)
    assert torch.equal(b['items'], old[0]) and torch.equal(b['labels_padded'], old[1]) and torch.equal(b['n_masked'], old[2])


def test_a_windows_row_does_not_depend_on_the_batch_its_place_or_the_batch_size():
    data, _, _ = _data(7, 1, 2)
    keys = ('items', 'labels_padded', 'n_masked', 'seq_idx', 'win_idx')
    rows = np.random.default_rng(0).permutation(data.n_windows)
    one = data.window_batch(rows, seed=9, width=7)
    for cut in (5, len(rows) - 1):
        parts = [data.window_batch(rows[:cut], seed=9, width=7), data.window_batch(rows[cut:], seed=9, width=7)]
        for k in keys:
            assert torch.equal(torch.cat([parts[0][k], parts[1][k]]), one[k]), (cut, k)
        assert one['n_real_tokens'] == parts[0]['n_real_tokens'] + parts[1]['n_real_tokens']
    back = data.window_batch(rows[::-1].copy(), seed=9, width=7)
    for k in keys:
        assert torch.equal(back[k].flip(0), one[k]), k
    # the epochs of two ranks of batch 3 are the world-1 epoch of batch 6
    whole = list(data.train_batches(6, 5, 2, width=7))
    ranks = [list(data.train_batches(3, 5, 2, rank=r, world=2, width=7)) for r in (0, 1)]
    for step in range(2):
        for k in keys:
            assert torch.equal(torch.cat([ranks[0][step][k], ranks[1][step][k]]), whole[step][k]), k
    # a narrower width cuts pad columns only
    free = data.window_batch(rows[:4], seed=9)
    Wf = free['items'].shape[1]
    assert torch.equal(free['items'], one['items'][:4, :Wf]) and not bool(one['items'][:4, Wf:].any())


@pytest.mark.parametrize('split,holdout', [('test', 1), ('test', 2), ('valid', 2)])
def test_history_equals_numpy(split, holdout):
    from bert4clickpath_amd import ops
    data, items, offsets = _data(7, 1, holdout)
    lengths = np.array(_lengths(7, 1, holdout))
    drop = 2 if split == 'valid' else 1
    seq = np.concatenate([np.random.default_rng(2).permutation(len(lengths)), [-1, 3, 3]]).astype(np.int32)
    seq_dev = torch.from_numpy(seq).cuda()
    longest = int(lengths.max()) - drop
    for E in (None, longest, longest + 5, 9, 1, 300):              # 9, 1: shorter than the history -> its most recent items
        got = data.history(seq_dev, split=split, width=E)
        Eh = longest if E is None else E
        assert got.dtype == torch.int32 and got.shape == (len(seq), Eh)
        assert np.array_equal(_host(got), ref.history(items, offsets, seq, Eh, drop)), E
    out = torch.full((len(seq), 12), SENTINEL_I, dtype=torch.int32, device='cuda')      # a pitch wider than E
    from bert4clickpath_amd import _lib
    _lib.check(_lib.lib().b4c_cloze_history(data.items_dev.data_ptr(), data.offsets_dev.data_ptr(), seq_dev.data_ptr(), len(seq), drop, 9,
                                            out.data_ptr(), 12, torch.cuda.current_stream().cuda_stream), 'cloze_history')
    assert np.array_equal(_host(out)[:, :9], ref.history(items, offsets, seq, 9, drop)) and (_host(out)[:, 9:] == SENTINEL_I).all()
    short = _host(got)[np.flatnonzero(seq == 0)[0]]                # sequence 0: `holdout` items, holdout - drop in front of the target
    assert (short != -1).sum() == holdout - drop and (_host(got)[len(lengths)] == -1).all()
    assert ops.cloze_history(data.items_dev, data.offsets_dev, seq_dev[:0], 4).shape == (0, 4)
    if split == 'valid':
        with pytest.raises(ValueError, match='valid'):
            _data(7, 1, 1)[0].history(seq_dev, split='valid')


def test_history_excludes_what_seen_items_excludes_when_every_sequence_fits_the_window():
    from bert4clickpath_amd import cloze
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    lengths = [0, 1, 2, 3, 5, 8, 13, 20, 20, 11, 7, 4]
    items, offsets = ref.synthetic_csr(lengths, V, seed=8)
    data = DeviceCloze(items, offsets, V=V, max_len=20, holdout=2)
    gen = torch.Generator().manual_seed(0)
    for split in ('valid', 'test'):
        b = next(data.eval_batches(len(lengths), split=split))
        y_pred = torch.rand(len(lengths), 1, V, generator=gen).cuda()
        # the label's neighbours in the ranking are the sequence's own items: exclusion changes the metric
        for g, n in enumerate(lengths):
            y_pred[g, 0, torch.from_numpy(items[offsets[g]:offsets[g + 1]].astype(np.int64)).cuda()] += 1.0
        res = {}
        for name, ex in (('history', data.history(b['seq_idx'], split=split)), ('seen', cloze.seen_items(b['items'])), ('none', None)):
            rec, nd = cloze.ClozeMaskedRecall(5), cloze.ClozeMaskedNDCG(5)
            rec.update_state(b['labels_padded'], y_pred, exclude=ex)
            nd.update_state(b['labels_padded'], y_pred, exclude=ex)
            res[name] = (float(rec.result()), float(nd.result()))
        assert res['history'] == res['seen']
        assert res['history'] != res['none']


def test_history_reaches_the_items_that_fell_out_of_the_window():
    from bert4clickpath_amd import cloze
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    items = np.arange(100, 110, dtype=np.int32)                    # one sequence of ten distinct items, rows of four
    data = DeviceCloze(items, np.array([0, 10]), V=V, max_len=4)
    b = next(data.eval_batches(1))
    assert _host(b['items']).tolist() == [[116, 117, 118, 1]] and _host(b['labels_padded']).tolist() == [[109.0]]
    y_pred = torch.zeros(1, 1, V)
    y_pred[0, 0, 100], y_pred[0, 0, 109] = 0.9, 0.5                # the best item is the oldest one, outside the window
    y_pred = y_pred.cuda()
    hist = data.history(b['seq_idx'])
    assert _host(hist).tolist() == [list(range(100, 109))]
    hit = {}
    for name, ex in (('history', hist), ('seen', cloze.seen_items(b['items']))):
        rec = cloze.ClozeMaskedRecall(1)
        rec.update_state(b['labels_padded'], y_pred, exclude=ex)
        hit[name] = float(rec.result())
    assert hit == {'history': 1.0, 'seen': 0.0}


# ---- through the model --------------------------------------------------------------------------------------------------------
def _tiny_model(dtype, d):
    """one layer, two heads; the head's last hidden width is the model width, as in the smoke run"""
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(0)
    vocab = ['item%d' % i for i in range(V)]
    return ClickstreamTransformer({'items': ['asin']}, {'items': vocab}, {'items': d}, SoftMaxHead([64, d], V), value_to_head='[MASK]',
                                  num_encoder_layers=1, num_attention_heads=2, dropout_rate=0.0, compute_dtype=dtype).to('cuda')


@pytest.mark.parametrize('dtype,d', [(torch.float32, 32), (torch.bfloat16, 64)], ids=['f32_dense', 'bf16_packed'])
def test_cloze_loss_on_windowed_train_batches_is_finite(dtype, d):
    """a wrong n_real_tokens poisons the loss to NaN: the host's count from the window lengths agrees with the device"""
    data, _, _ = _data(7, 1, 2)
    model = _tiny_model(dtype, d)
    for b in data.train_batches(8, 3, 2):
        M = b['labels_padded'].shape[1]
        loss = model.cloze_loss({'asin': b['items']}, b['labels_padded'], max_masked_per_row=M, n_real_tokens=b['n_real_tokens'])
        assert (model._packed is not None) == (dtype == torch.bfloat16)
        assert np.isfinite(float(loss.detach()))


def test_predict_topk_on_a_valid_batch_returns_one_row_per_non_empty_sequence():
    data, _, _ = _data(7, 1, 2)
    lengths = np.array(_lengths(7, 1, 2))
    model = _tiny_model(torch.float32, 32)
    b = next(data.eval_batches(len(lengths), split='valid'))
    n_rows = int((lengths >= 2).sum())
    assert int(b['n_masked'].sum()) == n_rows < len(lengths)
    labels = b['labels_padded'][b['n_masked'] == 1]
    idx, hit, ndcg = model.predict_topk({'asin': b['items']}, 10, labels)
    assert idx.shape == (n_rows, 10) and hit.shape == (n_rows,) and ndcg.shape == (n_rows,)
    ex = data.history(b['seq_idx'], split='valid')[b['n_masked'] == 1]
    idx_f, _, _ = model.predict_topk({'asin': b['items']}, 10, labels, exclude=ex)
    seen = _host(ex)
    for r in range(n_rows):                                        # nothing of the history is recommended again
        assert not (set(_host(idx_f)[r].tolist()) & (set(seen[r].tolist()) - {-1, int(labels[r, 0])}))
