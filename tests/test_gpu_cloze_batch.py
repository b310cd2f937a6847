"""Cloze batches built on the device (include/b4c.h "Cloze batches": b4c_cloze_batch; cloze_batches.DeviceCloze) against
the host restatement of tests/cloze_batch_ref.py, bit for bit: a synthetic CSR whose lengths sit on every boundary of the rule
and of the kernel, the committed Beauty file against input_pipeline.BeautyCloze (EVAL: equal; TRAIN: the structure, the random
stream being this kernel's own), independence of the batch split, and the batches through a tiny model."""
import os

import numpy as np
import pytest
import torch

import cloze_batch_ref as ref

pytestmark = pytest.mark.gpu

BEAUTY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'data', 'beauty_sequences.npz')
# train L = length - 1: 0 (twice), the first n = 1 (L = 3), n reaching the cap 10 (L = 25 -> 26), one and two waves (63 .. 65),
# the workgroup's 256 threads (256, 257), W = 1021 with no pad column; 1021 is the longest row EVAL takes
EDGES = [0, 1, 2, 3, 4, 5, 6, 26, 27, 64, 65, 66, 257, 258, 1022, 1021]
LENGTHS = EDGES + [7, 9, 12, 15, 18, 21, 24, 30, 33, 40, 48, 50, 70, 90, 100, 128, 129, 150, 197, 200, 255, 256, 300, 513]
V = 500
SENTINEL_I, SENTINEL_F = -77, -55.5


@pytest.fixture(scope='module')
def ops():
    from bert4clickpath_amd import ops as o
    return o


@pytest.fixture(scope='module')
def synth():
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    assert len(LENGTHS) == 40
    items, offsets = ref.synthetic_csr(LENGTHS, V, seed=11)
    return DeviceCloze(items, offsets, V=V), items, offsets


def _order(B, mode):
    """shuffled sequence indices, one sequence named twice.  EVAL leaves out the 1022-item sequence (longer than any row can
    be), TRAIN a filler, so that 39 sequences and the repeat make 40"""
    rng = np.random.default_rng(B)
    if B == 1:
        return np.array([LENGTHS.index(1022 if mode == ref.TRAIN else 1021)])
    if B == 7:
        seq = rng.permutation([0, 3, 7, 9, 12, 28])            # lengths 0, 3, 26, 64, 257, 70
        return np.insert(seq, 4, seq[1])
    left_out = LENGTHS.index(1022) if mode == ref.EVAL else LENGTHS.index(18)
    seq = rng.permutation([g for g in range(40) if g != left_out])
    return np.concatenate([seq, seq[5:6]])


def _host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize('mode', [ref.TRAIN, ref.EVAL])
@pytest.mark.parametrize('fixed_width', [False, True])
@pytest.mark.parametrize('B', [1, 7, 40])
def test_batches_equal_the_restatement_bit_for_bit(ops, synth, B, fixed_width, mode):
    data, items, offsets = synth
    seq = _order(B, mode)
    assert len(seq) == B and (B == 1 or len(set(seq.tolist())) == B - 1)
    longest = max(int(data.row_lengths(seq, mode).max()), 1)
    width = None if not fixed_width else min(longest + 13, 1021)
    seed = 0x9E3779B97F4A7C15 + B                             # >= 2^63
    got = data.batch(seq, mode, seed=seed, width=width)
    W = longest if width is None else width
    want_items, want_lab, want_n = ref.batch(items, offsets, seq, W, mode, seed)
    assert got['items'].dtype == torch.int64 and got['labels_padded'].dtype == torch.float32 and got['n_masked'].dtype == torch.int32
    assert got['items'].shape == (B, W) and got['labels_padded'].shape == (B, 10 if mode == ref.TRAIN else 1)
    assert np.array_equal(_host(got['items']), want_items)
    assert np.array_equal(_host(got['labels_padded']), want_lab)
    assert np.array_equal(_host(got['n_masked']), want_n)
    assert np.array_equal(_host(got['seq_idx']), seq)
    assert got['n_real_tokens'] == int((want_items != 0).sum()) + 3 * B
    if B > 1:                                                  # the sequence named twice: identical rows
        dup = [g for g in np.unique(seq) if (seq == g).sum() == 2][0]
        r0, r1 = np.flatnonzero(seq == dup)
        assert torch.equal(got['items'][r0], got['items'][r1]) and torch.equal(got['labels_padded'][r0], got['labels_padded'][r1])


@pytest.mark.parametrize('mode', [ref.TRAIN, ref.EVAL])
def test_pitches_wider_than_the_rows_leave_the_columns_past_them_untouched(ops, synth, mode):
    from bert4clickpath_amd import _lib
    data, items, offsets = synth
    seq = _order(40, mode)
    B, W, M, ld_i, ld_l = 40, 1021, 10 if mode == ref.TRAIN else 1, 1021 + 6, 13
    out = torch.full((B, ld_i), SENTINEL_I, dtype=torch.int64, device='cuda')
    lab = torch.full((B, ld_l), SENTINEL_F, dtype=torch.float32, device='cuda')
    nm = torch.full((B + 2,), SENTINEL_I, dtype=torch.int32, device='cuda')
    seq_d = torch.from_numpy(seq.astype(np.int32)).cuda()
    _lib.check(_lib.lib().b4c_cloze_batch(data.items_dev.data_ptr(), data.offsets_dev.data_ptr(), seq_d.data_ptr(), B, W, mode, 0.4, 10, 77,
                                          out.data_ptr(), ld_i, lab.data_ptr(), ld_l, M, nm.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), 'cloze_batch')
    want_items, want_lab, want_n = ref.batch(items, offsets, seq, W, mode, 77)
    out, lab, nm = _host(out), _host(lab), _host(nm)
    assert np.array_equal(out[:, :W], want_items) and (out[:, W:] == SENTINEL_I).all()
    assert np.array_equal(lab[:, :M], want_lab) and (lab[:, M:] == SENTINEL_F).all()
    assert np.array_equal(nm[:B], want_n) and (nm[B:] == SENTINEL_I).all()
    # n_masked_out may be NULL; B = 0 is a no-op
    out2 = torch.full((B, ld_i), SENTINEL_I, dtype=torch.int64, device='cuda')
    lab2 = torch.empty(B, ld_l, dtype=torch.float32, device='cuda')
    _lib.check(_lib.lib().b4c_cloze_batch(data.items_dev.data_ptr(), data.offsets_dev.data_ptr(), seq_d.data_ptr(), B, W, mode, 0.4, 10, 77,
                                          out2.data_ptr(), ld_i, lab2.data_ptr(), ld_l, M, None,
                                          torch.cuda.current_stream().cuda_stream), 'cloze_batch')
    assert np.array_equal(_host(out2), out)
    e_items, e_lab, e_n = ops.cloze_batch(data.items_dev, data.offsets_dev, seq_d[:0], 5, mode, 1)
    assert e_items.shape == (0, 5) and e_lab.shape == (0, M) and e_n.shape == (0,)


def test_other_label_widths_and_masking_parameters(ops, synth):
    """M wider than max_masked pads with -1; max_masked and masked_percentage other than the defaults; max_masked = 0"""
    data, items, offsets = synth
    seq = _order(40, ref.TRAIN)
    seq_d = torch.from_numpy(seq.astype(np.int32)).cuda()
    for pct, mm, M in ((0.4, 10, 64), (0.2, 3, 3), (1.0, 64, 64), (0.15, 20, 32), (0.4, 0, 0), (0.0, 10, 10)):
        got = ops.cloze_batch(data.items_dev, data.offsets_dev, seq_d, 1021, ops.CLOZE_TRAIN, 5, masked_percentage=pct, max_masked=mm, M=M)
        want = ref.batch(items, offsets, seq, 1021, ref.TRAIN, 5, masked_percentage=pct, max_masked=mm, M=M)
        for g, w in zip(got, want):
            assert np.array_equal(_host(g), w), (pct, mm, M)


def test_a_row_longer_than_the_width_is_refused_on_the_host(synth):
    data, _, _ = synth
    g = LENGTHS.index(1022)
    with pytest.raises(ValueError, match='at most 1021'):
        data.batch([g], 'eval')
    with pytest.raises(ValueError, match='shorter than a row'):
        data.batch([g, 3], 'train', width=1020)


def test_einval_cases_through_the_library(ops, synth):
    from bert4clickpath_amd import _lib
    data, _, _ = synth
    seq_d = torch.zeros(4, dtype=torch.int32, device='cuda')
    out = torch.zeros(4, 1024, dtype=torch.int64, device='cuda')
    lab = torch.zeros(4, 80, dtype=torch.float32, device='cuda')

    def call(W=8, mode=0, mm=10, M=10):
        return _lib.lib().b4c_cloze_batch(data.items_dev.data_ptr(), data.offsets_dev.data_ptr(), seq_d.data_ptr(), 4, W, mode, 0.4, mm, 0,
                                          out.data_ptr(), 1024, lab.data_ptr(), 80, M, None, torch.cuda.current_stream().cuda_stream)

    for kw in (dict(W=0), dict(W=1022), dict(M=9), dict(M=65, mm=65), dict(mode=2)):
        assert call(**kw) == -1, kw                            # B4C_EINVAL
        assert b'cloze_batch' in _lib.lib().b4c_last_error()
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool(out[:, 8:].any()) and not bool(lab[:, 10:].any())


# ---- the committed Beauty file ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def beauty():
    from bert4clickpath_amd import input_pipeline
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    host = input_pipeline.BeautyCloze(BEAUTY)
    return DeviceCloze.from_npz(BEAUTY), host


def test_beauty_eval_batches_equal_the_host_pipeline(beauty):
    dev, host = beauty
    got, want = list(dev.eval_batches(1024, limit=3000)), list(host.eval_batches(1024, 3000))
    assert len(got) == len(want) == 3 and got[-1]['items'].shape[0] == 3000 - 2048
    for g, w in zip(got, want):
        assert np.array_equal(_host(g['items']), w['ids'][:, 2:-1])
        assert np.array_equal(_host(g['labels_padded']), w['labels_padded'])
        assert g['n_real_tokens'] == int((w['ids'] != 0).sum())
        assert (_host(g['n_masked']) == 1).all()


def test_beauty_train_batches_have_the_structure_of_the_rule(beauty):
    """B = 512, two epochs (78 batches each): every row has exactly n_masked(L) [MASK] ids, the labels are the original items at
    those positions in order, every other column is the original item + 10, or 0 past L; the epochs mask differently; the same
    (seed, epoch) gives the same bits."""
    from bert4clickpath_amd import input_pipeline
    dev, host = beauty
    per_epoch = dev.n_seq // 512
    n_of = np.array([input_pipeline.n_masked(L) for L in range(64)])
    orig = np.zeros((dev.n_seq, 49), np.int64)                 # the TRAIN rows unmasked: item + 10, 0 past L
    Ls = np.maximum(dev.lengths - 1, 0)
    live = np.arange(49)[None, :] < Ls[:, None]
    orig[live] = np.concatenate([host.seq(g)[:-1] for g in range(dev.n_seq)]) + 10
    masks = np.zeros((2, dev.n_seq, 49), bool)
    seen = np.zeros((2, dev.n_seq), bool)
    first = []
    for step, b in enumerate(dev.train_batches(512, 21, 2 * per_epoch, width=49)):
        e = step // per_epoch
        seq, items, lab, nm = _host(b['seq_idx']), _host(b['items']), _host(b['labels_padded']), _host(b['n_masked'])
        assert not seen[e, seq].any()                          # a permutation: no sequence twice in an epoch
        seen[e, seq] = True
        m = items == 1
        assert np.array_equal(nm, n_of[Ls[seq]]) and np.array_equal(m.sum(1), nm)
        assert np.array_equal(np.where(m, orig[seq], items), orig[seq])       # unmasked columns: the original; masks inside L
        assert not (m & ~live[seq]).any()
        want_lab = np.full((512, 10), -1.0, np.float32)
        r, c = np.nonzero(m)                                   # row-major: ascending position within a row
        slot = np.arange(len(r)) - np.concatenate([[0], np.cumsum(nm)])[r]
        want_lab[r, slot] = orig[seq][r, c] - 10
        assert np.array_equal(lab, want_lab)
        assert b['n_real_tokens'] == int(Ls[seq].sum()) + 3 * 512
        masks[e, seq] = m
        if step < 3:
            first.append(b)
    assert seen.sum() == 2 * per_epoch * 512
    both = seen[0] & seen[1] & (n_of[Ls] >= 1)
    differ = (masks[0] != masks[1]).any(1)[both].mean()        # a sequence repeats its mask with probability <= 1/3 (L = 3, n = 1)
    assert differ > 0.5, differ
    for b, again in zip(first, dev.train_batches(512, 21, 3, width=49)):
        assert all(torch.equal(b[k], again[k]) for k in ('items', 'labels_padded', 'n_masked', 'seq_idx'))
    other = next(dev.train_batches(512, 22, 1, width=49))
    assert not torch.equal(other['seq_idx'], first[0]['seq_idx'])


def test_rows_do_not_depend_on_the_batch_split(beauty):
    dev, _ = beauty
    keys = ('items', 'labels_padded', 'n_masked', 'seq_idx')
    one = next(dev.train_batches(64, 5, 1, width=49))
    halves = list(dev.train_batches(32, 5, 2, width=49))
    ranks = [next(dev.train_batches(32, 5, 1, rank=r, world=2, width=49)) for r in (0, 1)]
    for pair in (halves, ranks):
        for k in keys:
            assert torch.equal(torch.cat([pair[0][k], pair[1][k]]), one[k]), k
    assert one['n_real_tokens'] == halves[0]['n_real_tokens'] + halves[1]['n_real_tokens']
    # batch-derived widths: the same rows, cut at the batch's longest
    free = next(dev.train_batches(64, 5, 1))
    W = free['items'].shape[1]
    assert W == int(dev.row_lengths(_host(one['seq_idx']), 'train').max())
    assert torch.equal(free['items'], one['items'][:, :W]) and not bool(one['items'][:, W:].any())


# ---- through the model --------------------------------------------------------------------------------------------------------
def _tiny_model(V, dtype, d):
    """one layer, two heads; the head's last hidden width is the model width, as in the smoke run"""
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(0)
    vocab = ['item%d' % i for i in range(V)]
    return ClickstreamTransformer({'items': ['asin']}, {'items': vocab}, {'items': d}, SoftMaxHead([64, d], V), value_to_head='[MASK]',
                                  num_encoder_layers=1, num_attention_heads=2, dropout_rate=0.0, compute_dtype=dtype).to('cuda')


@pytest.mark.parametrize('dtype,d', [(torch.float32, 32), (torch.bfloat16, 64)], ids=['f32_dense', 'bf16_packed'])
def test_cloze_loss_on_a_device_batch_equals_the_loss_on_the_uploaded_restatement(synth, dtype, d):
    data, items, offsets = synth
    seq = np.array([4, 7, 9, 6, 18, 27, 7, 5])                # lengths 4, 26, 64, 6, 12, 50, 26, 5
    model = _tiny_model(V, dtype, d)
    b = data.batch(seq, 'train', seed=31)
    M = b['labels_padded'].shape[1]
    loss = model.cloze_loss({'asin': b['items']}, b['labels_padded'], max_masked_per_row=M, n_real_tokens=b['n_real_tokens'])
    assert (model._packed is not None) == (dtype == torch.bfloat16)
    loss = float(loss.detach())
    assert np.isfinite(loss)                                   # neither poison flag fired: the host's token count and M hold
    w_items, w_lab, _ = ref.batch(items, offsets, seq, b['items'].shape[1], ref.TRAIN, 31)
    want = model.cloze_loss({'asin': torch.from_numpy(w_items).cuda()}, torch.from_numpy(w_lab).cuda(), max_masked_per_row=M,
                            n_real_tokens=int((w_items != 0).sum()) + 3 * len(seq))
    assert loss == float(want.detach())


def test_predict_topk_on_a_device_eval_batch_equals_the_host_batch(beauty):
    dev, host = beauty
    model = _tiny_model(dev.V, torch.float32, 32)
    g = next(dev.eval_batches(64, limit=64))
    w = next(host.eval_batches(64, 64))
    assert g['labels_padded'].shape == (64, 1)
    idx, hit, ndcg = model.predict_topk({'asin': g['items']}, 10, g['labels_padded'])
    w_items = torch.from_numpy(w['ids'])[:, 2:-1].contiguous().cuda()
    widx, whit, wndcg = model.predict_topk({'asin': w_items}, 10, torch.from_numpy(w['labels']).cuda(),
                                           flat_idx=torch.from_numpy(w['flat_idx']).cuda())
    assert idx.shape == (64, 10) and torch.equal(idx, widx) and torch.equal(hit, whit) and torch.equal(ndcg, wndcg)
