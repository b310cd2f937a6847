"""Exclusion lists in the ranking (include/b4c.h: b4c_exclusions_prep, b4c_vocab_rank_excl, b4c_vocab_topk_excl,
b4c_topk_rows_excl) against a numpy oracle on the materialised scores: an excluded item is absent from its row's ranking
(never an id, never before the label), every other item keeps its order (score descending, ties -> lower index), the label
is never excluded, ids -1 past the items that remain."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from bert4clickpath_amd import ops as o
    return o


def _operands(R, V, K, integer, seed):
    g = torch.Generator().manual_seed(seed)
    if integer:        # exact products: mass ties
        h = torch.randint(0, 3, (R, K), generator=g).float()
        W = torch.randint(-1, 2, (V, K), generator=g).float()
        b = torch.randint(0, 2, (V,), generator=g).float()
    else:
        h = (torch.randn(R, K, generator=g) * 0.5).bfloat16().float()
        W = (torch.randn(V, K, generator=g) * 0.3).bfloat16().float()
        b = torch.randn(V, generator=g) * 0.5
    y = torch.randint(0, V, (R,), generator=g).int()
    return h, W, b, y


def _device(h, W, b, V):
    Vp = (V + 7) // 8 * 8
    hd = h.cuda().bfloat16()
    wt = torch.zeros(Vp, h.shape[1], device='cuda', dtype=torch.bfloat16)
    wt[:V] = W.cuda().bfloat16()
    bd = torch.zeros(Vp, device='cuda')
    bd[:V] = b.cuda()
    return hd, wt, bd


def _mask(ex, V, y):
    """[R, V] bool: the row's eligible excluded items (in range, not the label)"""
    R = ex.shape[0]
    m = np.zeros((R, V), bool)
    rr, cc = np.nonzero((ex >= 0) & (ex < V))
    m[rr, ex[rr, cc]] = True
    if y is not None:
        ok = (y >= 0) & (y < V)
        m[np.arange(R)[ok], y[ok]] = False
    return m


def _oracle_topk(x, m, k):
    order = np.argsort(-x, axis=1, kind='stable')                 # score descending, ties -> lower index
    keep = ~np.take_along_axis(m, order, axis=1)
    pos = np.cumsum(keep, axis=1) - 1
    idx = np.full((x.shape[0], k), -1, np.int64)
    rr, cc = np.nonzero(keep & (pos < k))
    idx[rr, pos[rr, cc]] = order[rr, cc]
    return idx


def _oracle_rank(x, m, y):
    R, V = x.shape
    xy = x[np.arange(R), np.clip(y, 0, V - 1)][:, None]
    j = np.arange(V)[None, :]
    r = (((x > xy) | ((x == xy) & (j < y[:, None]))) & ~m).sum(1)
    return np.where((y >= 0) & (y < V), r, -1)


def _lists(x, y, E, seed, adversarial_rows=0, k=10):
    """[R, E] raw lists: random ids with duplicates, out-of-range / negative ids, the label in some rows, empty rows; the
    first `adversarial_rows` rows exclude their own true top 2k items"""
    R, V = x.shape
    rng = np.random.default_rng(seed)
    ex = rng.integers(0, V, (R, E))
    ex[:, E // 2:E // 2 + max(1, E // 8)] = ex[:, :max(1, E // 8)]          # duplicates
    ex[::3, -1] = V + 5
    ex[1::3, -1] = -3
    ex[::4, 0] = y[::4]                                                      # the label: never excluded
    ex[5::7] = -1                                                            # empty lists
    if adversarial_rows:
        top = np.argsort(-x[:adversarial_rows], axis=1, kind='stable')[:, :2 * k]
        n = min(2 * k, E)
        ex[:adversarial_rows, :n] = rng.permuted(top[:, :n], axis=1)
        ex[:adversarial_rows, n:] = -1
    return ex


CASES = [(300, 1000, 128, False, 40), (300, 1000, 128, True, 40), (77, 50, 64, True, 60), (130, 129, 64, False, 1024),
         (1000, 50000, 128, False, 200), (257, 5000, 128, True, 20), (16500, 3000, 64, False, 24), (16500, 1031, 128, True, 16)]


@pytest.mark.parametrize('R,V,K,integer,E', CASES)
def test_sweeps_and_materialised_ranking_with_exclusions_equal_the_oracle(ops, R, V, K, integer, E):
    h, W, b, y = _operands(R, V, K, integer, seed=R + V + E)
    y[:2] = -1                                           # pads
    hd, wt, bd = _device(h, W, b, V)
    yd = y.cuda()
    logits = ops.gemm_nt(hd, wt, wt.shape[0], bd, out_dtype=torch.float32)
    x = logits[:, :V].cpu().numpy()
    yn = y.numpy()
    k = min(10, V)
    raw = _lists(x, yn, E, seed=E, adversarial_rows=min(64, R), k=k)
    if E >= V:                                           # rows that exclude every item: the label alone remains (ids -1 after it)
        raw[10::5, :V] = np.arange(V)
        raw[10::5, V:] = -1
    ex = ops.exclusions(torch.from_numpy(raw).cuda(), V, yd)
    # canonical form
    exn = ex.cpu().numpy()
    m = _mask(raw, V, yn)
    for r in range(0, R, max(1, R // 50)):
        want = np.nonzero(m[r])[0]
        assert np.array_equal(exn[r, :len(want)], want) and (exn[r, len(want):] == -1).all()
    want_idx = _oracle_topk(x, m, k)
    want_rank = _oracle_rank(x, m, yn)
    # materialised fp32 logits, never written
    before = logits.clone()
    idx_m, hit_m, ndcg_m = ops.topk_rows(logits, V, k, yd, exclude=ex)
    assert torch.equal(logits, before)
    assert np.array_equal(idx_m.cpu().numpy(), want_idx)
    # the rank sweep
    rank = ops.vocab_rank(hd, wt, bd, yd, V, exclude=ex).cpu().numpy()
    assert np.array_equal(np.where(rank < 0, -1, rank), want_rank)
    hit_r, ndcg_r = ops.rank_metrics(torch.from_numpy(rank).cuda(), k)
    ok = want_rank >= 0
    hit_ref = (ok & (want_rank < k)).astype(np.float32)
    assert np.array_equal(hit_r.cpu().numpy(), hit_ref)
    assert np.allclose(ndcg_r.cpu().numpy(), hit_ref / np.log2(np.maximum(want_rank, 0) + 2.0), atol=1e-6)
    assert np.array_equal(hit_m.cpu().numpy()[ok], hit_ref[ok])
    assert np.allclose(ndcg_m.cpu().numpy()[ok], hit_ref[ok] / np.log2(want_rank[ok] + 2.0), atol=1e-6)
    # the top-k sweeps: every row that does not overflow
    idx, hit, ndcg, overflow = ops.vocab_topk(hd, wt, bd, V, k, yd, exclude=ex)
    idx = idx.cpu().numpy()
    over = (idx[:, 0] < 0) & (want_idx[:, 0] >= 0)
    assert int(over.sum()) == int(overflow)
    if not integer:
        assert int(overflow) == 0                        # the adversarial rows included: tau is that of the items left
    assert np.array_equal(idx[~over], want_idx[~over])
    v = ok & ~over
    assert np.array_equal(hit.cpu().numpy()[v], hit_ref[v])
    assert np.allclose(ndcg.cpu().numpy()[v], ndcg_m.cpu().numpy()[v], atol=1e-6)
    if E >= V:
        assert (want_idx[:, 1] < 0).sum() >= R // 5 - 2    # rows with fewer than k items are part of the case


def test_empty_lists_change_nothing(ops):
    R, V, K = 700, 3001, 128
    h, W, b, y = _operands(R, V, K, False, seed=5)
    hd, wt, bd = _device(h, W, b, V)
    yd = y.cuda()
    logits = ops.gemm_nt(hd, wt, wt.shape[0], bd, out_dtype=torch.float32)
    for E in (0, 7):
        ex = ops.exclusions(torch.full((R, E), -1, dtype=torch.int64, device='cuda'), V, yd)
        assert tuple(ex.shape) == (R, E)
        assert torch.equal(ops.vocab_rank(hd, wt, bd, yd, V, exclude=ex), ops.vocab_rank(hd, wt, bd, yd, V))
        a, b_ = ops.vocab_topk(hd, wt, bd, V, 10, yd, exclude=ex), ops.vocab_topk(hd, wt, bd, V, 10, yd)
        assert all(torch.equal(p, q) for p, q in zip(a, b_))
        for s in (logits, logits.bfloat16()):
            a, b_ = ops.topk_rows(s, V, 10, yd, exclude=ex), ops.topk_rows(s, V, 10, yd)
            assert all(torch.equal(p, q) for p, q in zip(a, b_))


@pytest.mark.parametrize('R,V', [(64, 3000), (4, 2000011)])
def test_materialised_probabilities_and_bf16_scores(ops, R, V):
    g = torch.Generator().manual_seed(V)
    ld = (V + 7) // 8 * 8
    logits = torch.zeros(R, ld)
    logits[:, :V] = torch.randn(R, V, generator=g) * 3
    logits = logits.cuda()
    probs = ops.softmax_rows(logits, V)
    y = torch.randint(0, V, (R,), generator=g).int()
    rng = np.random.default_rng(V)
    for scores in (probs, logits.bfloat16()):
        x = scores[:, :V].float().cpu().numpy()
        raw = rng.integers(0, V, (R, 300))
        raw[:, :20] = np.argsort(-x, axis=1, kind='stable')[:, :20]        # the row's own best items
        raw[::2, 20] = y.numpy()[::2]
        ex = ops.exclusions(torch.from_numpy(raw).cuda(), V, y.cuda())
        m = _mask(raw, V, y.numpy())
        before = scores.clone()
        idx, hit, ndcg = ops.topk_rows(scores, V, 10, y.cuda(), exclude=ex)
        assert torch.equal(scores, before)
        assert np.array_equal(idx.cpu().numpy(), _oracle_topk(x, m, 10))
        rk = _oracle_rank(x, m, y.numpy())
        assert np.array_equal(hit.cpu().numpy(), (rk < 10).astype(np.float32))
        # the list kernel (rows handed back by the threshold kernel) applies the lists too
        prev = ops.topk_threshold
        ops.topk_threshold = False
        try:
            idx2, _, _ = ops.topk_rows(scores, V, 10, y.cuda(), exclude=ex)
        finally:
            ops.topk_threshold = prev
        assert torch.equal(idx, idx2)


def _model(V, dtype, tied=False):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, ClozeMaskedItemPrediction, SoftMaxHead
    torch.manual_seed(0)
    head = ClozeMaskedItemPrediction([64], V) if tied else SoftMaxHead([64, 128], V)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': 128}, head,
                               value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, dropout_rate=0.0,
                               compute_dtype=dtype)
    if tied:
        head.tie(m.transformer.embedding_layers['items'].weight)
    return m.to('cuda')


@pytest.mark.parametrize('dtype,tied', [(torch.bfloat16, False), (torch.bfloat16, True), (torch.float32, False)])
def test_model_predict_topk_and_metrics_with_exclusions(ops, dtype, tied):
    from bert4clickpath_amd import cloze, input_pipeline
    from bert4clickpath_amd.cloze import ClozeMaskedNDCG, ClozeMaskedRecall
    V, B, S, k = 3000, 32, 40, 10
    m = _model(V, dtype, tied)
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=4, min_len=6)
    ids = torch.from_numpy(b['ids'])
    items = ids[:, 2:S - 1].contiguous().cuda()
    labels = torch.from_numpy(b['labels_padded']).cuda()
    seen = cloze.seen_items(items)                                            # (B, S') label-space history, -1 elsewhere
    with torch.no_grad():
        for packed in ((False, True) if dtype == torch.bfloat16 else (False,)):      # (the padding-free layout is bf16 only)
            # the oracle ranks the model's own materialised scores of the same layout (dense / padding-free)
            rows, _ = m._masked_rows({'asin': items}, False, pack=m._use_packed({'asin': items}, packed, None))
            R = rows.shape[0]
            lab = labels[labels != -1.0].to(torch.int32)
            scores = m.head.logits(rows, out_fp32=True)
            if dtype == torch.float32:
                scores = ops.softmax_rows(scores, V)                          # the parity path ranks probabilities
            x = scores[:, :V].float().cpu().numpy()
            offsets = m._row_offsets.cpu().numpy()
            seq = np.searchsorted(offsets[1:], np.arange(R), side='right')
            hist = seen.cpu().numpy()[seq]
            # the row's own best items too, so that the ids change
            per_row = np.concatenate([hist, np.argsort(-x, axis=1, kind='stable')[:, :5]], axis=1)
            labn = lab.cpu().numpy()
            for ex, w in ((torch.from_numpy(per_row).cuda(), _oracle_topk(x, _mask(per_row, V, labn), k)),
                          (seen, _oracle_topk(x, _mask(hist, V, labn), k))):     # (B, E): each sequence's history, per row
                idx, hit, ndcg = m.predict_topk({'asin': items}, k, labels, packed=packed, exclude=ex)
                assert np.array_equal(idx.cpu().numpy(), w), (packed, tuple(ex.shape))
                assert np.array_equal(hit.cpu().numpy(), (w == labn[:, None]).any(1).astype(np.float32))
        # metrics: the filtered rank of every row, materialised and lazy
        recs = []
        for y_pred in (m({'asin': items}, training=False, max_matches=10), m({'asin': items}, training=False, max_matches=10,
                                                                            scores='lazy')):
            rec, nd = ClozeMaskedRecall(k), ClozeMaskedNDCG(k)
            rec.update_state(labels, y_pred, exclude=seen)
            nd.update_state(labels, y_pred, exclude=seen)
            recs.append((float(rec.result()), float(nd.result())))
            rec0 = ClozeMaskedRecall(k)
            rec0.update_state(labels, y_pred)
            assert float(rec.result()) >= float(rec0.result())      # leaving items out never pushes the label down
        # bf16: the materialised bf16 probabilities tie where the logits do not -> compared as loosely as test_gpu_rank
        tol = 1e-6 if dtype == torch.float32 else 0.05
        assert abs(recs[0][0] - recs[1][0]) <= tol and abs(recs[0][1] - recs[1][1]) <= tol
        lazy = m({'asin': items}, training=False, max_matches=10, scores='lazy')
        if hasattr(lazy, 'rank_of'):
            yl = labels.reshape(-1)
            lab_l = torch.where(yl != -1.0, yl, torch.full_like(yl, -1)).to(torch.int32).contiguous()
            ex_l = ops.exclusions(seen.repeat_interleave(labels.shape[1], 0), V, lab_l)
            r0 = lazy.rank_of(lab_l).cpu().numpy()
            r1 = lazy.rank_of(lab_l, exclude=ex_l).cpu().numpy()
            # filtered rank = unfiltered rank - #{excluded items ranked before the label}
            wt, bl = lazy._operands()                  # the logits the sweep ranks, materialised (b4c_gemm_nt)
            xl = ops.gemm_nt(lazy.h2d, wt, wt.shape[0], bl, out_dtype=torch.float32)[:, :V].cpu().numpy()
            yn = lab_l.cpu().numpy()
            ml = _mask(seen.repeat_interleave(labels.shape[1], 0).cpu().numpy(), V, yn)
            xy = xl[np.arange(len(yn)), np.clip(yn, 0, V - 1)][:, None]
            before = (((xl > xy) | ((xl == xy) & (np.arange(V)[None] < yn[:, None]))) & ml).sum(1)
            v = yn >= 0
            assert np.array_equal(r1[v], r0[v] - before[v])
