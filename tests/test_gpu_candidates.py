"""Candidate lists on the device (include/b4c.h "candidate lists": b4c_sample_candidates, b4c_candidate_score,
b4c_candidate_rank_rows) against the host restatements of tests/candidates_ref.py: the sampler bit for bit, the scores
against float64, rank / top-k exactly (integer-exact scores: equal to the full-vocabulary kernels with the list 0 .. V-1),
the heads, the model and the metrics with candidates=, and an evaluation batch at C2 scoring size."""
import numpy as np
import pytest
import torch

from candidates_ref import rank_rows, sample_rows, topk_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from bert4clickpath_amd import ops as o
    return o


def _canonical_host(ex_dev):
    return [[int(v) for v in row if v >= 0] for row in ex_dev.cpu().numpy()]


# ---- 1. the sampler, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 100, 1023])
@pytest.mark.parametrize('popularity', [False, True])
@pytest.mark.parametrize('with_excl', [False, True])
def test_sampler_is_bit_exact_against_the_restatement(ops, N, popularity, with_excl):
    V = 5000
    R = 6 if N == 1023 else 70
    rng = np.random.default_rng(N + 10 * popularity + 100 * with_excl)
    y = rng.integers(0, V, R)
    y[2], y[4] = -1, V + 3                                     # rows without a valid label
    lab = torch.from_numpy(y.astype(np.int32)).cuda()
    counts = rng.integers(0, 20, V)
    counts[::3] = 0
    cdf = np.cumsum(counts).astype(np.int64)
    ex = ex_host = None
    if with_excl:
        raw = rng.integers(-3, V + 3, (R, 300))
        raw[:, :5] = y[:, None]                                # the label in the raw list: removed by ops.exclusions
        ex = ops.exclusions(torch.from_numpy(raw).cuda(), V, lab)
        ex_host = _canonical_host(ex)
    cdf_d = torch.from_numpy(cdf).cuda() if popularity else None
    cand, short = ops.sample_candidates(lab, V, N, seed=0xC0FFEE, row_base=1000, exclude=ex, item_cdf=cdf_d)
    want, wshort = sample_rows(y, V, N, 0xC0FFEE, 1000, ex_host, cdf if popularity else None)
    assert np.array_equal(cand.cpu().numpy(), want)
    assert int(short) == wshort
    again, short2 = ops.sample_candidates(lab, V, N, seed=0xC0FFEE, row_base=1000, exclude=ex, item_cdf=cdf_d)
    assert torch.equal(cand, again) and int(short2) == wshort
    # two row_base chunks = one call
    cut = R // 3
    a, _ = ops.sample_candidates(lab[:cut].contiguous(), V, N, 0xC0FFEE, 1000, None if ex is None else ex[:cut].contiguous(), cdf_d)
    b, _ = ops.sample_candidates(lab[cut:].contiguous(), V, N, 0xC0FFEE, 1000 + cut, None if ex is None else ex[cut:].contiguous(),
                                 cdf_d)
    assert torch.equal(torch.cat([a, b]), cand)


def test_sampler_runs_dry_on_a_tiny_vocabulary(ops):
    V, N, R = 6, 10, 9
    y = np.array([0, 1, 2, 3, 4, 5, -1, 2, 5])
    lab = torch.from_numpy(y.astype(np.int32)).cuda()
    counts = np.array([3, 0, 1, 1, 0, 9], np.int64)
    for cdf in (None, np.cumsum(counts)):
        cand, short = ops.sample_candidates(lab, V, N, seed=3, item_cdf=None if cdf is None else torch.from_numpy(cdf).cuda())
        want, wshort = sample_rows(y, V, N, 3, 0, None, cdf)
        c = cand.cpu().numpy()
        assert np.array_equal(c, want)
        assert int(short) == wshort == 8                      # every valid row is short
        for r in range(R):
            if y[r] < 0:
                assert (c[r] == -1).all()
                continue
            pool = {i for i in range(V) if i != y[r] and (cdf is None or counts[i] > 0)}
            assert set(c[r, 1:1 + len(pool)].tolist()) == pool      # 64 N attempts find the whole pool here
            assert (c[r, 1 + len(pool):] == -1).all()


# ---- 2. scores against float64 --------------------------------------------------------------------------------------------
def _table(V, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    Vp = (V + 7) // 8 * 8
    W = (torch.randn(V, K, generator=g) * 0.3).to(dtype)
    wt = torch.zeros(Vp, K, dtype=dtype)
    wt[:V] = W
    b = torch.zeros(Vp)
    b[:V] = torch.randn(V, generator=g) * 0.5
    return wt.cuda(), b.cuda()


def _lists(R, C, V, rng, y=None):
    cand = rng.integers(0, V, (R, C))
    if C >= 4:
        cand[:, C - 1] = cand[:, 0]                            # duplicates
        cand[::2, 1] = -5                                      # absent
        cand[1::2, 2] = V + 7
        if y is not None:
            cand[::3, 3] = y[::3]                              # the label listed in some rows
    return cand.astype(np.int32)


SCORE_CASES = ([(dt, K, 101, 257) for dt in (torch.float32, torch.bfloat16) for K in (8, 64, 128, 256, 1000)]
               + [(dt, 128, C, 33) for dt in (torch.float32, torch.bfloat16) for C in (1, 7, 1024)]
               + [(torch.float32, 64, 7, 0), (torch.bfloat16, 64, 7, 1), (torch.float32, 64, 7, 4097),
                  (torch.bfloat16, 128, 101, 4097)])


@pytest.mark.parametrize('dtype,K,C,R', SCORE_CASES)
def test_scores_rank_and_topk_against_float64(ops, dtype, K, C, R):
    V = 3001
    rng = np.random.default_rng(K * 7 + C + R)
    wt, b = _table(V, K, dtype, seed=K + C)
    big = (torch.randn(R, K + 24, generator=torch.Generator().manual_seed(R + K)) * 0.5).to(dtype).cuda()
    h = big[:, 8:8 + K]                                        # strided rows (pitch K + 24), offset start
    y = rng.integers(0, V, R)
    if R:
        y[0] = -1
    cand = _lists(R, C, V, rng, y)
    cd = torch.from_numpy(cand).cuda()
    yd = torch.from_numpy(y.astype(np.int32)).cuda()
    k = min(10, C)
    scores, rank, idx = ops.candidate_scores(h, wt, b, cd, V, labels=yd, k=k)
    assert scores.shape == (R, C) and rank.shape == (R,) and idx.shape == (R, k)
    if R == 0:
        return
    hn, Wn, bn = h.double().cpu().numpy(), wt.double().cpu().numpy(), b.double().cpu().numpy()
    present = (cand >= 0) & (cand < V)
    cc = np.where(present, cand, 0)
    prod = hn[:, None, :] * Wn[cc]                             # [R, C, K] float64
    ref = prod.sum(-1) + bn[cc]
    bound = K * 2.0 ** -24 * (np.abs(prod).sum(-1) + np.abs(bn[cc])) + 1e-30     # fp32 summation of K + 1 terms
    s = scores.cpu().numpy()
    assert np.isnan(s[~present]).all()
    assert (np.abs(s[present] - ref[present]) <= bound[present]).all(), np.abs(s - ref)[present].max()
    # duplicates score alike; rank / top-k follow the definition on the device's own scores (exact where the label is listed)
    if C >= 4:
        assert np.array_equal(s[:, C - 1][present[:, 0]], s[:, 0][present[:, 0]])
    assert np.array_equal(idx.cpu().numpy(), topk_rows(s, cand, V, k))
    listed = np.array([0 <= y[r] < V and y[r] in cand[r] for r in range(R)])
    if listed.any():
        p = np.array([int(np.nonzero(cand[r] == y[r])[0][0]) if listed[r] else 0 for r in range(R)])
        s_lab = s[np.arange(R), p]
        want = rank_rows(s, cand, s_lab, y, V)
        assert np.array_equal(rank.cpu().numpy()[listed], want[listed])
    assert int(rank[0]) < 0
    # the scores are optional and change nothing else
    s2, rank2, idx2 = ops.candidate_scores(h, wt, b, cd, V, labels=yd, k=k, want_scores=False)
    assert s2 is None and torch.equal(rank2, rank) and torch.equal(idx2, idx)


# ---- 3. integer-exact ties: equal to the full-vocabulary kernels ----------------------------------------------------------
@pytest.mark.parametrize('V', [64, 1000, 1024])
def test_the_whole_vocabulary_as_a_list_equals_the_full_rank(ops, V):
    R, K, k = 300, 128, 10
    g = torch.Generator().manual_seed(V)
    h = torch.randint(0, 3, (R, K), generator=g).bfloat16().cuda()
    Vp = (V + 7) // 8 * 8
    wt = torch.zeros(Vp, K, dtype=torch.bfloat16)
    wt[:V] = torch.randint(-1, 2, (V, K), generator=g).bfloat16()
    wt = wt.cuda()
    b = torch.zeros(Vp)
    b[:V] = torch.randint(0, 2, (V,), generator=g).float()
    b = b.cuda()
    y = torch.randint(0, V, (R,), generator=g).int()
    y[:3] = -1
    yd = y.cuda()
    full = torch.arange(V, dtype=torch.int32).repeat(R, 1).cuda()
    scores, rank, idx = ops.candidate_scores(h, wt, b, full, V, labels=yd, k=k)
    want_rank = ops.vocab_rank(h, wt, b, yd, V)
    assert torch.equal(torch.where(want_rank < 0, -1, want_rank), torch.where(rank < 0, -1, rank))
    assert (rank[:3] < 0).all()
    logits = ops.gemm_nt(h, wt, wt.shape[0], b, out_dtype=torch.float32)
    assert torch.equal(scores, logits[:, :V])                  # integer-exact: every summation order agrees
    vi, _, _, _ = ops.vocab_topk(h, wt, b, V, k, yd)
    ok = vi[:, 0] >= 0                                         # (rows with mass ties at the threshold hand back -1)
    assert torch.equal(idx[ok], vi[ok])
    ti, _, _ = ops.topk_rows(logits, V, k)
    assert torch.equal(idx, ti)
    # the same on the materialised logits, fp32 and bf16 (exact small integers)
    for x in (logits, logits.bfloat16()):
        before = x.clone()
        r2, i2 = ops.candidate_rank_rows(x, V, full, yd, k)
        assert torch.equal(x, before)
        assert torch.equal(r2, rank) and torch.equal(i2, ti)
    # shuffled lists, with duplicates and absent entries: the same rank; the top-k is the full top-k
    rng = np.random.default_rng(V)
    perm = np.stack([rng.permutation(V) for _ in range(R)])
    extra = np.concatenate([perm, perm[:, :min(V, 1024 - V)]], axis=1).astype(np.int32)     # duplicates where C allows
    cd = torch.from_numpy(extra).cuda()
    _, r3, i3 = ops.candidate_scores(h, wt, b, cd, V, labels=yd, k=k, want_scores=False)
    assert torch.equal(r3, rank) and torch.equal(i3, idx)
    r4, i4 = ops.candidate_rank_rows(logits, V, cd, yd, k)
    assert torch.equal(r4, rank) and torch.equal(i4, idx)
    # a short list: against the restatement with the exact scores
    short = np.concatenate([perm[:, :37], perm[:, :5], np.full((R, 3), -1)], axis=1).astype(np.int32)
    sd = torch.from_numpy(short).cuda()
    s5, r5, i5 = ops.candidate_scores(h, wt, b, sd, V, labels=yd, k=k)
    x = logits[:, :V].cpu().numpy()
    yn = y.numpy()
    want = rank_rows(np.where(short >= 0, x[np.arange(R)[:, None], np.maximum(short, 0)], np.nan), short,
                     x[np.arange(R), np.clip(yn, 0, V - 1)], yn, V)
    assert np.array_equal(r5.cpu().numpy(), want)
    assert np.array_equal(i5.cpu().numpy(), topk_rows(s5.cpu().numpy(), short, V, k))
    hit, ndcg = ops.rank_metrics(r5, k)
    assert np.array_equal(hit.cpu().numpy(), ((want >= 0) & (want < k)).astype(np.float32))


# ---- 4. heads, model and metrics ------------------------------------------------------------------------------------------
def _model(V, dtype, kind):
    from bert4clickpath_amd.clickstream_transformer import (ClickstreamTransformer, ClozeMaskedItemPrediction, SampledSoftmaxHead,
                                                             SoftMaxHead)
    torch.manual_seed(0)
    head = {'softmax': lambda: SoftMaxHead([64, 128], V), 'tied': lambda: ClozeMaskedItemPrediction([64], V),
            'sampled': lambda: SampledSoftmaxHead([96], V, num_sampled=512)}[kind]()
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': 128}, head,
                               value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, dropout_rate=0.0,
                               compute_dtype=dtype)
    if kind == 'tied':
        head.tie(m.transformer.embedding_layers['items'].weight)
    return m.to('cuda')


@pytest.mark.parametrize('kind', ['softmax', 'tied', 'sampled'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_model_scores_topk_and_metrics_with_candidates(ops, kind, dtype):
    from bert4clickpath_amd import cloze, input_pipeline
    from bert4clickpath_amd.clickstream_transformer.head import ClozeScores
    V, B, S, k = 3000, 24, 40, 10
    m = _model(V, dtype, kind)
    m.eval()
    bt = input_pipeline.synthetic_cloze_batch(B, S, V, seed=9, min_len=6)
    items = torch.from_numpy(bt['ids'])[:, 2:S - 1].contiguous().cuda()
    labels = torch.from_numpy(bt['labels_padded']).cuda()
    inp = {'asin': items}
    counts = cloze.item_counts(items, V)
    counts += 1                                                # every item drawable
    cand_all = cloze.sample_candidates(labels, 100, exclude=cloze.seen_items(items), item_counts=counts, seed=1)
    valid = (labels.reshape(-1) != -1.0)
    cand = cand_all[valid]                                     # (R, 101): one list per [MASK] row, label first
    lab = labels.reshape(-1)[valid].to(torch.int32)
    R = cand.shape[0]
    with torch.no_grad():
        scores = m.score_candidates(inp, cand)
        assert scores.shape == (R, 101) and scores.dtype == torch.float32
        # float64 restatement of the head's logits at the list
        rows, _ = m._masked_rows(inp, False)
        hh = m.head.trunk(rows)
        K, _, _ = m.head._proj()
        wt, _, bb = m.head._packs[-1].get(hh.dtype, K, False)
        hn, Wn, bn = hh.double().cpu().numpy(), wt.double().cpu().numpy(), bb.double().cpu().numpy()
        cn = cand.cpu().numpy()
        prod = hn[:, None, :] * Wn[cn]
        ref = prod.sum(-1) + bn[cn]
        bound = K * 2.0 ** -24 * (np.abs(prod).sum(-1) + np.abs(bn[cn])) + 1e-30
        s = scores.cpu().numpy()
        assert (np.abs(s - ref) <= bound).all()
        # the logits of the full projection agree at the listed columns (the same model, the full-vocabulary route)
        full = m.head.logits(rows, out_fp32=True)[:, :V].double().cpu().numpy()
        assert np.allclose(full[np.arange(R)[:, None], cn], ref, rtol=1e-4, atol=1e-4 if dtype == torch.float32 else 2e-2)
        # predict_topk(candidates=): ids from the list, in order; hit / ndcg of the rank among the list
        idx, hit, ndcg = m.predict_topk(inp, k, labels, candidates=cand)
        labn = lab.cpu().numpy()
        want_idx = topk_rows(s, cn, V, k)
        assert np.array_equal(idx.cpu().numpy(), want_idx)
        assert all(set(r[r >= 0].tolist()) <= set(c.tolist()) for r, c in zip(idx.cpu().numpy(), cn))
        want_rank = rank_rows(s, cn, s[:, 0], labn, V)         # the label is listed first: its own score
        assert np.array_equal(hit.cpu().numpy(), (want_rank < k).astype(np.float32))
        assert np.allclose(ndcg.cpu().numpy(), (want_rank < k) / np.log2(want_rank + 2.0), atol=1e-6)
        # (B, C) lists: one per sequence, for each of its rows
        per_seq = torch.from_numpy(np.stack([cn[0]] * B)).cuda()
        i2, _, _ = m.predict_topk(inp, k, candidates=per_seq)
        assert (np.isin(i2.cpu().numpy(), cn[0]) | (i2.cpu().numpy() < 0)).all()
        assert np.array_equal(i2.cpu().numpy()[0], want_idx[0])           # row 0 keeps its own list
        # metrics: the lazy scores (through the head's candidate scores) and the materialised probabilities
        preds = []
        lazy = m(inp, training=False, max_matches=10, scores='lazy')
        if hasattr(lazy, 'rank_of'):                           # (fp32 / other widths: the model materialises instead)
            preds.append(('lazy', lazy))
        probs = m(inp, training=False, max_matches=10)
        preds.append(('materialised', probs))
        yt = labels.reshape(-1)
        labf = torch.where(yt != -1.0, yt, torch.full_like(yt, -1)).to(torch.int32)
        for name, y_pred in preds:
            rec, nd = cloze.ClozeMaskedRecall(k), cloze.ClozeMaskedNDCG(k)
            rec.update_state(labels, y_pred, candidates=cand_all)
            nd.update_state(labels, y_pred, candidates=cand_all)
            if name == 'lazy':
                sc, _, _ = m.head.score_candidates(y_pred.h2d, cand_all, trunk_done=True)
                sl = sc.cpu().numpy()
            else:
                pn = y_pred.reshape(-1, V).float().cpu().numpy()
                ca = cand_all.cpu().numpy()
                sl = np.where(ca >= 0, pn[np.arange(ca.shape[0])[:, None], np.maximum(ca, 0)], np.nan)
            ca = cand_all.cpu().numpy()
            yl = labf.cpu().numpy()
            wr = rank_rows(sl, ca, sl[:, 0], yl, V)
            v = yl >= 0
            want_hit = ((wr >= 0) & (wr < k))[v].mean()
            want_nd = np.where((wr >= 0) & (wr < k), 1.0 / np.log2(np.maximum(wr, 0) + 2.0), 0.0)[v].mean()
            assert abs(float(rec.result()) - want_hit) < 1e-6, name
            assert abs(float(nd.result()) - want_nd) < 1e-5, name
        # a ClozeScores of any dtype ranks through the candidate kernel (fp32 too)
        h2d = m.head.trunk(m._masked_rows(inp, False)[0])
        cs = ClozeScores(m.head, h2d, (R,))
        r_cs = cs.rank_of(lab, candidates=cand).cpu().numpy()
        assert np.array_equal(r_cs, want_rank)
        assert cs.rank_of(lab, candidates=cand) is cs.rank_of(lab, candidates=cand)      # cached per (labels, candidates)
        i_cs, h_cs, _ = cs.topk(k, lab, candidates=cand)
        assert np.array_equal(i_cs.cpu().numpy(), want_idx) and torch.equal(h_cs, hit)


def test_packed_layout_with_a_contradicted_token_count_poisons_the_rows(ops):
    from bert4clickpath_amd import input_pipeline
    V, B, S, k = 3000, 16, 40, 10
    m = _model(V, torch.bfloat16, 'softmax')
    m.eval()
    bt = input_pipeline.synthetic_cloze_batch(B, S, V, seed=2, min_len=6)
    ids = torch.from_numpy(bt['ids'])
    items = ids[:, 2:S - 1].contiguous().cuda()
    labels = torch.from_numpy(bt['labels_padded']).cuda()
    n_real = int((ids != 0).sum())
    inp = {'asin': items}
    R = int((labels != -1.0).sum())
    cand = torch.randint(0, V, (R, 33), dtype=torch.int32, device='cuda')
    with torch.no_grad():
        good = m.score_candidates(inp, cand, packed=True, n_real_tokens=n_real)
        assert torch.isfinite(good).all()
        idx, hit, ndcg = m.predict_topk(inp, k, labels, packed=True, n_real_tokens=n_real, candidates=cand)
        assert (idx >= 0).all() and torch.isfinite(hit).all()
        bad = m.score_candidates(inp, cand, packed=True, n_real_tokens=n_real + 3)
        assert torch.isnan(bad).all()
        idx, hit, ndcg = m.predict_topk(inp, k, labels, packed=True, n_real_tokens=n_real + 3, candidates=cand)
        assert (idx == -1).all() and torch.isnan(hit).all() and torch.isnan(ndcg).all()


# ---- 5. an evaluation batch at C2 scoring size ----------------------------------------------------------------------------
def test_c2_scoring_batch_popularity_with_seen_items(ops):
    from bert4clickpath_amd import cloze
    R, V, K, N, B = 40960, 50000, 128, 100, 2048
    g = torch.Generator().manual_seed(11)
    seqs = torch.randint(10, V + 10, (B, 200), generator=g)            # input ids: histories of 200 items
    seqs[:, 150:] = 0                                                  # padding
    counts = cloze.item_counts(seqs, V)
    counts[counts == 0] = 1
    y = torch.randint(0, V, (R,), generator=g).to(torch.int32)
    yt = y.float().reshape(B, R // B)                                  # (B, M): 20 [MASK] rows per sequence
    seen = cloze.seen_items(seqs).cuda()
    cand = cloze.sample_candidates(yt, N, exclude=seen, item_counts=counts, seed=7, row_base=0)
    assert cand.shape == (R, N + 1)
    assert torch.equal(cand[:, 0].cpu(), y)
    neg = cand[:, 1:].long()
    assert (neg >= 0).all()                                            # no row short at this size
    srt, _ = torch.sort(neg, dim=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()                           # distinct
    assert (neg != cand[:, :1].long()).all()                           # never the label
    hist = torch.sort(seen.repeat_interleave(R // B, 0), dim=1)[0]     # the row's sequence history
    pos = torch.searchsorted(hist, srt).clamp(max=hist.shape[1] - 1)
    assert (torch.gather(hist, 1, pos) != srt).all()                   # no seen item among the negatives
    again = cloze.sample_candidates(yt, N, exclude=seen, item_counts=counts, seed=7, row_base=0)
    assert torch.equal(cand, again)
    h = (torch.randn(R, K, generator=g) * 0.5).bfloat16().cuda()
    wt, b = _table(V, K, torch.bfloat16, seed=3)
    yd = y.cuda()
    _, r1, i1 = ops.candidate_scores(h, wt, b, cand, V, labels=yd, k=10, want_scores=False)
    _, r2, i2 = ops.candidate_scores(h, wt, b, cand, V, labels=yd, k=10, want_scores=False)
    assert torch.equal(r1, r2) and torch.equal(i1, i2)
    assert (r1 >= 0).all() and (r1 <= N).all()
    s, r3, _ = ops.candidate_scores(h, wt, b, cand, V, labels=yd)
    assert torch.equal(r3, r1) and torch.isfinite(s).all()


# ---- argument layouts and caching -----------------------------------------------------------------------------------------
def test_expanded_lists_equal_repeated_lists_and_overlapping_exclusions_are_refused(ops):
    from bert4clickpath_amd._lib import B4CError
    R, V, K, C = 5000, 3001, 128, 101
    wt, b = _table(V, K, torch.bfloat16, seed=1)
    h = (torch.randn(R, K, generator=torch.Generator().manual_seed(2)) * 0.5).bfloat16().cuda()
    y = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(3)).to(torch.int32).cuda()
    lst = torch.randperm(V, generator=torch.Generator().manual_seed(4))[:C].to(torch.int32).cuda()
    shared, rep = lst.expand(R, -1), lst.repeat(R, 1)
    assert shared.stride(0) == 0
    s1, r1, i1 = ops.candidate_scores(h, wt, b, shared, V, labels=y, k=10)
    s2, r2, i2 = ops.candidate_scores(h, wt, b, rep, V, labels=y, k=10)
    assert torch.equal(s1, s2) and torch.equal(r1, r2) and torch.equal(i1, i2)
    logits = ops.gemm_nt(h, wt, wt.shape[0], b, out_dtype=torch.float32)
    a1 = ops.candidate_rank_rows(logits, V, shared, y, 10)
    a2 = ops.candidate_rank_rows(logits, V, rep, y, 10)
    assert all(torch.equal(p, q) for p, q in zip(a1, a2))
    ex = ops.exclusions(torch.arange(50, dtype=torch.int64, device='cuda').reshape(1, 50), V).expand(R, -1)
    with pytest.raises(B4CError, match='overlap'):
        ops.sample_candidates(y, V, 20, seed=0, exclude=ex)


def test_a_cdf_without_mass_draws_nothing(ops):
    y = torch.tensor([3, -1, 0, 7], dtype=torch.int32, device='cuda')
    cand, short = ops.sample_candidates(y, 8, 5, seed=1, item_cdf=torch.zeros(8, dtype=torch.int64, device='cuda'))
    c = cand.cpu().numpy()
    assert int(short) == 3 and np.array_equal(c[:, 0], [3, -1, 0, 7]) and (c[:, 1:] == -1).all()


def test_metric_cache_does_not_answer_a_new_list_with_an_old_rank(ops):
    """the same probabilities ranked against freshly sampled lists, inline: each call gets its own list's rank"""
    from bert4clickpath_amd import cloze
    B, M, V, k = 64, 4, 2000, 10
    g = torch.Generator().manual_seed(8)
    probs = torch.softmax(torch.randn(B, M, V, generator=g), -1).cuda()
    labels = torch.randint(0, V, (B, M), generator=g).float().cuda()
    labels[::5, -1] = -1.0
    got = []
    for seed in (1, 2, 1):
        nd = cloze.ClozeMaskedNDCG(k)
        nd.update_state(labels, probs, candidates=cloze.sample_candidates(labels, 20, seed=seed, num_items=V))
        got.append(float(nd.result()))
    want = []
    for seed in (1, 2):
        cand = cloze.sample_candidates(labels, 20, seed=seed, num_items=V).cpu().numpy()
        pn = probs.reshape(-1, V).cpu().numpy()
        yl = labels.reshape(-1).cpu().numpy().astype(np.int64)
        sl = np.where(cand >= 0, pn[np.arange(cand.shape[0])[:, None], np.maximum(cand, 0)], np.nan)
        wr = rank_rows(sl, cand, sl[:, 0], yl, V)
        want.append(float(np.where((wr >= 0) & (wr < k), 1.0 / np.log2(np.maximum(wr, 0) + 2.0), 0.0)[yl >= 0].mean()))
    assert abs(got[0] - want[0]) < 1e-5 and abs(got[1] - want[1]) < 1e-5 and got[2] == got[0]
    assert want[0] != want[1]                                   # (the two lists do rank differently here)
