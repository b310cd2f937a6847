"""Next-item batches built on the device (include/b4c.h; NO REFERENCE ORACLE: an extension -- the restatement is
tests/next_item_ref.py): every output of the kernel bit for bit on the case list, every list against the existing sampler (an
independent kernel), purity, and the model entry next_item_loss against cloze_loss / candidate_loss on host-built inputs.
Everything about the batches is integer-exact: no tolerance.  Gradients of two routes through the same kernels differ only by the
order of the candidate backward's float atomics: the two-route gates of tests/test_gpu_candidate_loss.py."""
import numpy as np
import pytest
import torch

import next_item_ref as ref

pytestmark = pytest.mark.gpu

SENT = -777
MAX_LEN = 5


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops as o
    return o


@pytest.fixture(scope='module')
def data(ops):
    items, offsets, V = ref.case_data()
    return items, offsets, V, torch.from_numpy(items).cuda(), torch.from_numpy(offsets).cuda()


def _cdfs(V):
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 5, V)
    counts[::3] = 0                                               # zero-mass items
    return {'uniform': None, 'popularity': np.cumsum(counts).astype(np.int64), 'no_mass': np.zeros(V, np.int64)}


def _table(offsets, holdout):
    """window_table's windows at max_len = stride = 5, and one window of no items (L = 0) of sequence 1 at the end"""
    from bert4clickpath_amd.cloze_batches import window_table
    w = window_table(np.diff(offsets), MAX_LEN, MAX_LEN, holdout)
    return tuple(np.concatenate([x, np.array([v], np.int32)]) for x, v in zip(w, (1, 0, 0)))


def _case_rows(table):
    """<= 16 rows: every short sequence's windows, the repeated-item sequence, the long sequence's window at 0 (in front of the
    1024 most recent items), one inside them and its last, an empty row (negative index), the L = 0 window"""
    seq, start, _ = table
    pick = [int(w) for w in np.flatnonzero(np.isin(seq[:-1], [2, 3, 5, 6, 10]))]
    long_w = np.flatnonzero(seq[:-1] == 7)
    four = np.flatnonzero(seq[:-1] == 4)
    pick += [int(long_w[np.argmin(start[long_w])]), int(long_w[len(long_w) // 2]), int(long_w[0]), int(four[0]), int(four[-1]), -1,
             len(seq) - 1]
    assert len(pick) <= 16
    return np.array(pick, np.int64)


def _launch(data, mode, row_idx, table, W, N, seed, excl, cdf, holdout, rows_extra=0, max_len=MAX_LEN, want=None):
    """b4c_next_item_batch into sentinel-filled buffers with two spare rows / columns -> numpy outputs cut to the written extent
    (the spare cells are checked here)"""
    from bert4clickpath_amd import _lib
    items, offsets, V, items_d, offsets_d = data
    B = len(row_idx)
    R = want['n_targets']
    rows = R + rows_extra
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    tab = [dev(t, np.int32) for t in table] if table is not None else [None] * 3
    row_d, off_d = dev(row_idx, np.int32), dev(want['row_off'], np.int32)
    cdf_d = None if cdf is None else dev(cdf, np.int64)
    out = torch.full((B + 2, W + 2), SENT, dtype=torch.int64, device='cuda')
    flat = torch.full((rows + 2,), SENT, dtype=torch.int32, device='cuda')
    lab = torch.full((rows + 2,), SENT, dtype=torch.int32, device='cuda')
    cand = torch.full((rows + 2, N + 3), SENT, dtype=torch.int32, device='cuda') if N else None
    short = torch.full((3,), SENT, dtype=torch.int32, device='cuda')
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.lib().b4c_next_item_batch(p(items_d), p(offsets_d), p(tab[0]), p(tab[1]), p(tab[2]), p(row_d), p(off_d), B, W, mode, holdout,
                                              max_len, V, N, seed, excl, p(cdf_d), p(out), W + 2, p(flat), p(lab), p(cand), N + 3, rows,
                                              p(short) if N else None, torch.cuda.current_stream().cuda_stream), 'next_item_batch')
    torch.cuda.synchronize()
    out, flat, lab, short = out.cpu().numpy(), flat.cpu().numpy(), lab.cpu().numpy(), short.cpu().numpy()
    assert (out[B:] == SENT).all() and (out[:, W:] == SENT).all() and (flat[rows:] == SENT).all() and (lab[rows:] == SENT).all()
    got = {'items': out[:B, :W], 'flat_idx': flat[:rows], 'labels': lab[:rows], 'candidates': None, 'short': 0}
    if N:
        cand = cand.cpu().numpy()
        assert (cand[rows:] == SENT).all() and (cand[:, N + 1:] == SENT).all() and (short[1:] == SENT).all()
        got['candidates'], got['short'] = cand[:rows, :N + 1], int(short[0])
    else:
        assert (short == SENT).all()
    return got


def _same(got, want):
    for k in ('items', 'flat_idx', 'labels', 'candidates'):
        assert (got[k] is None and want[k] is None) or np.array_equal(got[k], want[k]), k
    assert got['short'] == want['short']


def _check_lists(want, V):
    """no negative is the label or an item of X_g, and a row's negatives are distinct"""
    R = want['n_targets']
    for r in range(R):
        neg = want['candidates'][r, 1:]
        neg = neg[neg >= 0].tolist()
        assert len(set(neg)) == len(neg) and int(want['labels'][r]) not in neg and not (set(neg) & want['X'][r]), r


# ---- the kernel against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('holdout', [1, 2])
@pytest.mark.parametrize('N, cdf, exclude', [(0, 'uniform', 'history'), (1, 'uniform', 'history'), (20, 'uniform', 'history'),
                                             (20, 'uniform', None), (3, 'popularity', 'history'), (2, 'no_mass', 'history')])
def test_train_rows_equal_the_restatement(ops, data, holdout, N, cdf, exclude):
    """the case list's TRAIN rows: L = 0, 1, 2, a window at a > 0 (the prepended input), a window of exactly max_len, an empty row,
    repeated items, the 1100-item sequence (the cap of X_g), rows = R + 7, W wider than the longest row."""
    items, offsets, V = data[:3]
    table = _table(offsets, holdout)
    rows = _case_rows(table)
    cdf = _cdfs(V)[cdf]
    want = ref.batch(items, offsets, ref.TRAIN, rows, V, table, holdout, MAX_LEN, W=8, N=N, seed=99, exclude=exclude, cdf=cdf,
                     rows=None)
    R = want['n_targets']
    Ls = set(int(table[2][w]) for w in rows if w >= 0)
    assert {0, 1, 2, MAX_LEN} <= Ls and R > 30
    padded = ref.batch(items, offsets, ref.TRAIN, rows, V, table, holdout, MAX_LEN, W=8, N=N, seed=99, exclude=exclude, cdf=cdf, rows=R + 7)
    got = _launch(data, ops.NEXT_TRAIN, rows, table, 8, N, 99, ops.NEXT_EXCLUDE[exclude], cdf, holdout, rows_extra=7, want=want)
    _same(got, padded)
    assert (got['flat_idx'][R:] == -1).all() and (got['labels'][R:] == -1).all()
    if N:
        assert (got['candidates'][R:] == -1).all()
        if exclude == 'history':
            _check_lists(want, V)
        if cdf is not None and int(cdf[-1]) == 0:
            assert got['short'] == R and (got['candidates'][:R, 1:] == -1).all()


def test_short_rows_are_counted(ops):
    """V = 12, ten distinct items in the view, N = 3: two items are left, every row is short"""
    seq = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 3, 11], np.int32)
    offsets = np.array([0, 12], np.int64)
    d = (seq, offsets, 12, torch.from_numpy(seq).cuda(), torch.from_numpy(offsets).cuda())
    table = (np.array([0], np.int32), np.array([0], np.int32), np.array([11], np.int32))
    want = ref.batch(seq, offsets, ref.TRAIN, [0], 12, table, 1, None, W=12, N=3, seed=5)
    assert want['short'] == want['n_targets'] == 10
    got = _launch(d, ops.NEXT_TRAIN, np.array([0]), table, 12, 3, 5, 1, None, 1, want=want)
    _same(got, want)


@pytest.mark.parametrize('drop', [1, 2])
def test_eval_rows_equal_the_restatement(ops, data, drop):
    """EVAL rows of every sequence (t = -1, 0, 1, .., max_len + 5, 1098) and an empty row; with negatives, which the batch builders
    do not ask for but the entry point defines"""
    items, offsets, V = data[:3]
    rows = np.array(list(range(len(offsets) - 1)) + [-1], np.int64)
    ts = set((np.diff(offsets) - drop).tolist())
    assert {0, 1, MAX_LEN + 5} <= ts
    for N in (0, 4):
        want = ref.batch(items, offsets, ref.EVAL, rows, V, None, drop, MAX_LEN, W=7, N=N, seed=8)
        got = _launch(data, ops.NEXT_EVAL, rows, None, 7, N, 8, 1, None, drop, want=want)
        _same(got, want)
    assert want['n_targets'] == int(((np.diff(offsets) - drop) >= 1).sum())


# ---- against the existing sampler -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N, cdf', [(20, 'uniform'), (3, 'popularity')])
def test_every_list_is_what_sample_candidates_draws_for_that_target(ops, data, N, cdf):
    items, offsets, V = data[:3]
    table = _table(offsets, 1)
    rows = _case_rows(table)
    cdf = _cdfs(V)[cdf]
    want = ref.batch(items, offsets, ref.TRAIN, rows, V, table, 1, MAX_LEN, W=8, N=N, seed=31, cdf=cdf)
    got = _launch(data, ops.NEXT_TRAIN, rows, table, 8, N, 31, 1, cdf, 1, want=want)
    cdf_d = None if cdf is None else torch.from_numpy(cdf).cuda()
    short = 0
    for r in range(want['n_targets']):
        y = torch.tensor([int(want['labels'][r])], dtype=torch.int32, device='cuda')
        ex = ops.exclusions([sorted(want['X'][r])], V, labels=y)
        c, s = ops.sample_candidates(y, V, N, 31, row_base=want['csr'][r], exclude=ex, item_cdf=cdf_d)
        assert np.array_equal(c.cpu().numpy()[0], got['candidates'][r]), r
        short += int(s.item())
    assert short == got['short']


# ---- purity -----------------------------------------------------------------------------------------------------------------------
def _dc(data, **kw):
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    items, offsets, V = data[:3]
    return DeviceCloze(items, offsets, V=V, **kw)


def test_a_row_does_not_depend_on_its_batch(ops, data):
    dc = _dc(data, max_len=MAX_LEN)
    rows = _case_rows((dc.windows.seq, dc.windows.start, dc.windows.len))[:-2]         # (the L = 0 window is not in dc's table)
    rows = np.concatenate([rows, rows])[:16]
    big = dc.next_item_window_batch(rows, seed=4, width=9, num_negatives=6)
    off = big['row_offsets'].cpu().numpy()
    assert off[-1] == big['n_targets'] and big['flat_idx'].shape[0] == big['n_targets']
    where = {}
    for b, w in enumerate(rows.tolist()):
        one = dc.next_item_window_batch([w], seed=4, width=9, num_negatives=6)
        lo, hi = off[b], off[b + 1]
        assert torch.equal(one['items'][0], big['items'][b]) and torch.equal(one['labels'], big['labels'][lo:hi])
        assert torch.equal(one['candidates'], big['candidates'][lo:hi])
        assert torch.equal(one['flat_idx'] - 2, big['flat_idx'][lo:hi] - 2 - b * 12)
        where.setdefault(w, []).append(b)
    assert max(len(v) for v in where.values()) == 2               # the same window at two places of one batch
    other = dc.next_item_window_batch(rows, seed=5, width=9, num_negatives=6)
    assert torch.equal(other['labels'], big['labels']) and not torch.equal(other['candidates'], big['candidates'])


def test_two_ranks_build_what_one_builds(ops, data):
    dc = _dc(data, max_len=MAX_LEN, holdout=2)
    kw = dict(width=6, num_negatives=3)
    one = list(dc.next_item_batches(8, 21, 3, **kw))
    two = [list(dc.next_item_batches(4, 21, 3, rank=r, world=2, **kw)) for r in (0, 1)]
    for step, b in enumerate(one):
        halves = [two[0][step], two[1][step]]
        assert torch.equal(b['items'], torch.cat([h['items'] for h in halves]))
        assert torch.equal(b['win_idx'], torch.cat([h['win_idx'] for h in halves]))
        assert torch.equal(b['seq_idx'], torch.cat([h['seq_idx'] for h in halves]))
        assert torch.equal(b['labels'], torch.cat([h['labels'] for h in halves]))
        assert torch.equal(b['candidates'], torch.cat([h['candidates'] for h in halves]))
        assert b['n_targets'] == sum(h['n_targets'] for h in halves) and b['n_real_tokens'] == sum(h['n_real_tokens'] for h in halves)
        want = ref.batch(data[0], data[1], ref.TRAIN, b['win_idx'].cpu().numpy(), data[2], dc.windows, 2, MAX_LEN, W=6, N=3,
                         seed=int(ops.rand64_host(21, 0)))
        assert np.array_equal(b['flat_idx'].cpu().numpy(), want['flat_idx']) and np.array_equal(b['candidates'].cpu().numpy(), want['candidates'])
        assert np.array_equal(b['row_offsets'].cpu().numpy(), want['row_off']) and int(b['short'].item()) == want['short']


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _model(V, d, dtype, seed=0):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, ClozeMaskedItemPrediction
    torch.manual_seed(seed)
    hd = ClozeMaskedItemPrediction([], V)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': d}, hd, value_to_head='[MASK]',
                               num_encoder_layers=2, num_attention_heads=2, dropout_rate=0.0, compute_dtype=dtype, attention='causal')
    hd.tie(m.transformer.embedding_layers['items'].weight)
    m = m.to('cuda')
    with torch.no_grad():
        m.head.output_bias.normal_(0, 0.3)
    return m


def _model_batch(data, holdout=1):
    """12 windows of up to 20 items (the long sequence's, the repeated-item sequence's, short ones), W = 24"""
    dc = _dc(data, max_len=20, holdout=holdout)
    seq = dc.windows.seq
    rows = np.concatenate([np.flatnonzero(seq == 7)[:6], np.flatnonzero(np.isin(seq, [3, 4, 6, 8, 9, 10]))])[:12]
    return dc, rows


def _grads(model, loss):
    model.zero_grad(set_to_none=True)
    loss.backward()
    return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16_packed'])
@pytest.mark.parametrize('loss', ['full', 'bce', 'softmax'])
def test_next_item_loss_equals_the_losses_on_host_built_inputs(ops, data, dtype, loss):
    """next_item_loss(device batch) against cloze_loss / candidate_loss called with the restatement's items, flat_idx, labels and
    candidates: the loss bit for bit; gradients inside the two-route gates of tests/test_gpu_candidate_loss.py (fp32: 2 x 2e-4 of a
    gradient's largest entry, 2 x 1e-5 where it is identically zero; bf16: 2 x BF16_GRAD_BOUND in relative L2).  A rows=-padded
    batch gives the same loss; on the packed layout a contradicted n_real_tokens gives NaN."""
    from bf16_gates import BF16_GRAD_BOUND, grad_errors
    items, offsets, V = data[:3]
    bf16 = dtype == torch.bfloat16
    model = _model(V, 128 if bf16 else 64, dtype, seed=2)
    dc, rows = _model_batch(data)
    N = 0 if loss == 'full' else 7
    b = dc.next_item_window_batch(rows, seed=13, width=24, num_negatives=N)
    want = ref.batch(items, offsets, ref.TRAIN, rows, V, dc.windows, 1, 20, W=24, N=N, seed=13)
    assert b['n_targets'] == want['n_targets'] > 100 and b['n_real_tokens'] == want['n_real_tokens']
    got = model.next_item_loss(b, loss=loss)
    g_got = _grads(model, got)
    assert (model._packed is not None) == bf16
    feats = {'asin': torch.from_numpy(want['items']).cuda()}
    flat, lab = torch.from_numpy(want['flat_idx']).cuda(), torch.from_numpy(want['labels']).cuda()
    if loss == 'full':
        host = model.cloze_loss(feats, lab, flat_idx=flat, n_real_tokens=want['n_real_tokens'])
    else:
        host = model.candidate_loss(feats, lab, candidates=torch.from_numpy(want['candidates']).cuda(), loss=loss, flat_idx=flat,
                                    n_real_tokens=want['n_real_tokens'])
    g_ref = _grads(model, host)
    print('next_item_loss %s: %.9g, host-built %.9g' % (loss, float(got.detach()), float(host.detach())))
    assert float(got.detach()) == float(host.detach()) and np.isfinite(float(got.detach()))
    assert set(g_got) == set(g_ref)
    if bf16:
        for n, p in model.named_parameters():                     # (grad_errors reads p.grad: give it the device route's)
            if n in g_got:
                p.grad = g_got[n].to(p.grad.dtype).cuda()
        errs = grad_errors(model.named_parameters(), g_ref)
        assert len(errs) >= len(g_ref) - 2 and max(errs.values()) <= 2 * BF16_GRAD_BOUND, errs
    else:
        for n, gr in g_ref.items():
            if float(gr.abs().max()) < 1e-9:
                assert float(g_got[n].abs().max()) < 2 * 1e-5, n
            else:
                assert float((g_got[n] - gr).abs().max()) <= 2 * 2e-4 * float(gr.abs().max()), n
    with torch.no_grad():
        padded = dc.next_item_window_batch(rows, seed=13, width=24, num_negatives=N, rows=b['n_targets'] + 9)
        assert padded['flat_idx'].shape[0] == b['n_targets'] + 9 and int(padded['flat_idx'][-1]) == -1
        lp = model.next_item_loss(padded, loss=loss, training=False)
        l0 = model.next_item_loss(b, loss=loss, training=False)
        print('next_item_loss %s: padded %.9g, unpadded %.9g' % (loss, float(lp), float(l0)))
        assert float(lp) == float(l0)
        if bf16:
            wrong = dict(b, n_real_tokens=b['n_real_tokens'] + 3)
            assert torch.isnan(model.next_item_loss(wrong, loss=loss, training=False))
    if loss != 'full':
        with pytest.raises(ops.B4CError, match='num_negatives > 0'):
            model.next_item_loss(dict(b, candidates=None), loss=loss)


def test_predict_topk_on_an_eval_batch(ops, data):
    """EVAL batches at holdout = 2: sequences without a target have no compact row, so hit / ndcg count the others only; the
    device batch ranks as the restatement's host-built inputs do, with the history as the exclusion list"""
    items, offsets, V = data[:3]
    model = _model(V, 64, torch.float32, seed=4)
    dc = _dc(data, max_len=MAX_LEN, holdout=2)
    n, fewer = 0, False
    for split, drop in (('valid', 2), ('test', 1)):
        for b in dc.next_item_eval_batches(6, width=7, split=split):
            seqs = b['seq_idx'].cpu().numpy()
            want = ref.batch(items, offsets, ref.EVAL, seqs, V, None, drop, MAX_LEN, W=7)
            with_target = seqs[(np.diff(offsets)[seqs] - drop) >= 1]
            assert np.array_equal(b['items'].cpu().numpy(), want['items']) and np.array_equal(b['flat_idx'].cpu().numpy(), want['flat_idx'])
            assert np.array_equal(b['labels'].cpu().numpy(), want['labels']) and b['n_real_tokens'] == want['n_real_tokens']
            assert np.array_equal(b['target_seq_idx'].cpu().numpy(), with_target) and b['n_targets'] == len(with_target)
            if b['n_targets'] == 0:
                continue
            seen = dc.history(b['target_seq_idx'], split)
            idx, hit, ndcg = model.predict_topk({'asin': b['items']}, 10, labels=b['labels'], flat_idx=b['flat_idx'],
                                                n_real_tokens=b['n_real_tokens'], exclude=seen)
            idx2, hit2, ndcg2 = model.predict_topk({'asin': torch.from_numpy(want['items']).cuda()}, 10,
                                                   labels=torch.from_numpy(want['labels']).cuda(),
                                                   flat_idx=torch.from_numpy(want['flat_idx']).cuda(), exclude=seen)
            assert hit.shape[0] == ndcg.shape[0] == idx.shape[0] == len(with_target)
            fewer |= len(with_target) < len(seqs)
            assert torch.equal(idx, idx2) and torch.equal(hit, hit2) and torch.equal(ndcg, ndcg2) and bool(torch.isfinite(ndcg).all())
            for r, g in enumerate(with_target.tolist()):             # nothing of the history comes back
                end = int(offsets[g + 1]) - drop                   # (history() keeps the most recent B4C_MAX_EXCL items)
                hist = set(items[max(int(offsets[g]), end - 1024):end].tolist()) - {int(want['labels'][r])}
                assert not (set(idx[r].cpu().tolist()) & hist)
            n += len(with_target)
    assert fewer and n == int((np.diff(offsets) >= 3).sum()) + int((np.diff(offsets) >= 2).sum())


def test_three_steps_of_the_example_loop_reduce_the_loss(ops, data):
    """the loop of examples/beauty_hitrate.py --objective next_item at toy size: a smoke run of the plumbing, not a quality claim"""
    from bert4clickpath_amd import optim
    model = _model(data[2], 64, torch.float32, seed=6)
    dc, rows = _model_batch(data, holdout=2)
    opt = optim.Adam(model.parameters(), learning_rate=1e-2)
    losses = []
    for step in range(4):
        b = dc.next_item_window_batch(rows[:8], seed=1, width=20, num_negatives=4)       # one batch, seen again: the loss must fall
        opt.zero_grad()
        loss = model.next_item_loss(b, loss='bce')
        if step < 3:
            loss.backward()
            opt.step()
        losses.append(float(loss.detach()))
    print('next-item bce loss over three steps:', losses)
    assert np.isfinite(losses).all() and losses[3] < losses[0]
    assert len(list(dc.next_item_batches(4, 3, 2, num_negatives=1))) == 2
