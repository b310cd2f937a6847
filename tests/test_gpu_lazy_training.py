"""The row-lazy Adam (optim.LazyRows over b4c_adam_rows) as a user trains with it, and both Adam kernels against float64.

A. b4c_adam_step and b4c_adam_rows over ~300 irregular steps against a float64 restatement of Keras' Adam
   (oracle/numpy_ref.adam_step, lr_t recomputed per step in float64): gaps between a row's touches around `max_staleness`,
   an lr change inside a gap, grad_mul != 1, rows that never receive a gradient, gradients near the fp32 extremes.
B. Lazy against dense THROUGH THE MODEL, bit for bit (ops.deterministic is on by default): the bench order, the
   `forward -> zero_grad -> backward -> step` order, accumulated micro-batches, evaluation forwards between steps, a mid-run lr
   change, a checkpoint round trip, two lazy tables, and a tied-weight head over a lazy table.
C. The sampled-softmax head (config 5, reduced): its row scatter uses float atomics, so lazy and dense agree to a stated
   tolerance, and the table state (zero gradient rows, every stamp current) is checked exactly.
D. Two ranks with a lazy table under the row-sparse exchange and under its dense fallback.
And the lr_t table of the lazy optimizer over ~3000 steps: its entries and how often it is reallocated."""
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-9


def _lr_t(lr, t):
    return lr * math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)


def _tolerance(p64, p32, lr_sum, T):
    """|p - p64| <= 256 * sum_s lr_s * 2^-23 + T * ulp(p): see test_adam_kernels_match_float64_over_long_histories"""
    mag = np.maximum(np.abs(p64), np.abs(p32.astype(np.float64))).astype(np.float32)
    return 256.0 * lr_sum * 2.0 ** -23 + T * np.spacing(mag).astype(np.float64)


def _grad_schedule(rows, T, staleness, seed):
    """(steps x rows) bool: which rows receive a gradient at each step.  Row classes (by row % 8): 0 never; 1 every step;
    2..5 every (staleness - 1, staleness, staleness + 1, 2.5 x staleness) steps; 6, 7 at random (p = 0.3)"""
    rng = np.random.default_rng(seed)
    on = np.zeros((T + 1, rows), dtype=bool)
    r = np.arange(rows)
    cls = r % 8
    on[1:, cls == 1] = True
    for c, gap in ((2, staleness - 1), (3, staleness), (4, staleness + 1), (5, int(2.5 * staleness))):
        sel = r[cls == c]
        for j, row in enumerate(sel):
            on[1 + j % gap::gap, row] = True
    sel = (cls == 6) | (cls == 7)
    on[1:, sel] = rng.random((T, int(sel.sum()))) < 0.3
    return on


def _magnitudes(rows):
    """per-row gradient scale: most rows O(1), some 1e-20 (g^2 underflows below the fp32 normal range), some 1e15"""
    s = np.ones(rows)
    s[np.arange(rows) % 11 == 3] = 1e-20
    s[np.arange(rows) % 13 == 5] = 1e15
    return s


@pytest.mark.parametrize('rows,width', [(1003, 4), (517, 8), (301, 128), (97, 256)])
def test_adam_kernels_match_float64_over_long_histories(rows, width):
    """The dense kernel (ops.adam_step_ over the arena) and the row-lazy one (optim.Adam(lazy_rows=[table]), max_staleness 16)
    against float64 Keras Adam, 300 steps.  Row counts are not multiples of the 4-row blocks of b4c_adam_rows nor of the
    dense kernel's 4-element vectors.

    Tolerance.  One fp32 step p <- p - lr_t * m / (sqrt(v) + eps) rounds m, v (one fma each), g (1 - b), g^2, lr_t * m, the
    sqrt, the sum, the quotient and the difference.  The ratio m / (sqrt(v) + eps) is bounded by (1 - b1) / sqrt(1 - b2) ~ 3.2
    and reaches the update with a relative error of a few 2^-24 from its own operations, plus the absolute error m carries:
    every step multiplies the old error by b1 and adds ~ulp(m), so it stays below ~10 ulp(max |m|) -- relative to sqrt(v)
    that is up to ~50 x 2^-23 where the gradient changes sign and m cancels (an fp32 restatement of these steps on the host
    reaches 55).  The subtraction from p rounds once per step: half an ulp of p.  So after T steps
        |p - p64| <= c * sum_s lr_s * 2^-23 + T * ulp(p),     c = 256 (about 5 x the worst case seen).
    A lost or repeated update is lr_t * O(0.1 .. 3) ~ 1e-5 .. 1e-3 and a replay with a neighbouring step's lr_t ~1e-6 per
    replayed step; the bound here is ~2e-6 (|p| <= ~1).  Rows that never receive a gradient keep m = v = 0 and must keep p
    exactly (0 / (0 + eps) = 0): asserted bit for bit, as is lazy == dense."""
    from bert4clickpath_amd import optim
    from oracle import numpy_ref as nr
    T, staleness = 300, 16
    on = _grad_schedule(rows, T, staleness, seed=rows)
    scale = _magnitudes(rows)
    g0 = torch.Generator().manual_seed(rows + width)
    p0 = (torch.randn(rows, width, generator=g0) * 0.05)
    dense_p = torch.nn.Parameter(p0.clone().cuda())
    lazy_p = torch.nn.Parameter(p0.clone().cuda())
    od = optim.Adam([dense_p])
    ol = optim.Adam([lazy_p], lazy_rows=[lazy_p], max_staleness=staleness)
    lz = lazy_p._b4c_lazy
    P, M, V = p0.double().numpy(), np.zeros((rows, width)), np.zeros((rows, width))
    rng = np.random.default_rng(width)
    lr, lr_sum = 1e-3, 0.0
    for t in range(1, T + 1):
        if t == 150:                     # inside the gaps of classes 3..5: the replay of a missed step must use its own lr_t
            od.lr = ol.lr = lr = 3.17e-4
        mul = 0.5 if t % 4 == 0 else (3.0 if t % 7 == 0 else 1.0)
        g = (rng.standard_normal((rows, width)) * scale[:, None] * on[t][:, None]).astype(np.float32)
        ids = np.nonzero(on[t])[0]
        gt = torch.from_numpy(g).cuda()
        od.zero_grad()
        ol.zero_grad()
        if ids.size:
            lz.catch_up(torch.from_numpy(ids).cuda())
        dense_p.grad.copy_(gt)
        lazy_p.grad.copy_(gt)
        od.step(mul)
        ol.step(mul)
        P, M, V = nr.adam_step(P, g.astype(np.float64) * mul, M, V, t, lr=lr, beta1=B1, beta2=B2, eps=EPS)
        lr_sum += _lr_t(lr, t)
        assert float(lazy_p.grad.abs().max()) == 0.0, t
    ol.sync_rows()
    torch.cuda.synchronize()
    pd, pl = dense_p.detach().cpu().numpy(), lazy_p.detach().cpu().numpy()
    assert np.array_equal(pd, pl), 'lazy != dense in %d elements' % int((pd != pl).sum())
    assert torch.equal(od.m, ol.m) and torch.equal(od.v, ol.v)
    stamp = lz.stamp.cpu().numpy()
    # every row current; a row that never had a gradient keeps stamp 0 (all moments zero: nothing to replay)
    assert np.array_equal(stamp == 0, ~on.any(axis=0)) and (stamp[on.any(axis=0)] == T).all()
    assert np.isfinite(pd).all()
    never = ~on.any(axis=0)
    assert np.array_equal(pd[never], p0.numpy()[never]), 'rows without a gradient moved'
    assert float(od.v[:rows * width].view(rows, width)[torch.from_numpy(never).cuda()].abs().max()) == 0.0
    err = np.abs(pd.astype(np.float64) - P)
    tol = _tolerance(P, pd, lr_sum, T)
    bad = err > tol
    assert not bad.any(), 'fp32 Adam off float64 in %d elements: worst %g (tolerance %g) at row %d' % (
        int(bad.sum()), float(err.max()), float(tol.reshape(-1)[err.argmax()]), int(err.argmax()) // width)
    # the moments too: m to the same absolute form, v relative
    m32 = od.m[:rows * width].view(rows, width).cpu().numpy().astype(np.float64)
    v32 = od.v[:rows * width].view(rows, width).cpu().numpy().astype(np.float64)
    big = np.sqrt(V) + 1e-30
    assert float((np.abs(m32 - M) / big).max()) < 1e-4
    assert float((np.abs(v32 - V) / np.maximum(V, 1e-300)).max(where=V > 1e-30, initial=0.0)) < 1e-4


def test_dense_kernel_directly_on_a_ragged_flat_buffer():
    """ops.adam_step_ on n = 1001 elements (the dense kernel's scalar tail), 300 steps, against float64; zero-gradient elements
    bit-still; gradients 1e-20 and 1e15; grad_mul 0.25"""
    from bert4clickpath_amd import ops
    from oracle import numpy_ref as nr
    n, T = 1001, 300
    rng = np.random.default_rng(3)
    p0 = (rng.standard_normal(n) * 0.05).astype(np.float32)
    p, m, v = torch.from_numpy(p0.copy()).cuda(), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    P, M, V = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    scale = np.ones(n)
    scale[::7] = 1e-20
    scale[3::11] = 1e15
    scale[5::13] = 0.0                    # never a gradient
    lr, lr_sum = 1e-3, 0.0
    for t in range(1, T + 1):
        if t == 200:
            lr = 1e-4
        g = (rng.standard_normal(n) * scale * (rng.random(n) < 0.5)).astype(np.float32)
        lr_t = _lr_t(lr, t)
        ops.adam_step_(p, torch.from_numpy(g).cuda(), m, v, lr_t, B1, B2, EPS, 0.25)
        P, M, V = nr.adam_step(P, g.astype(np.float64) * 0.25, M, V, t, lr=lr, beta1=B1, beta2=B2, eps=EPS)
        lr_sum += lr_t
    pc = p.cpu().numpy()
    assert np.isfinite(pc).all()
    assert np.array_equal(pc[5::13], p0[5::13])
    err = np.abs(pc.astype(np.float64) - P)
    assert (err <= _tolerance(P, pc, lr_sum, T)).all(), float(err.max())


def test_lr_table_is_written_per_step_and_rarely_reallocated():
    """optim.Adam.lr_hist over 3000 lazy steps: at most ceil(log2(3000 / 1024)) + 1 allocations of the device table; every
    entry equals fp32(lr_t) computed in float64 from the lr in force at that step, also across an lr change and after
    load_state_dict (which restates the history from the loaded lr)"""
    from bert4clickpath_amd import optim
    table = torch.nn.Parameter(torch.randn(64, 8).cuda() * 0.05)
    opt = optim.Adam([table], lazy_rows=[table], max_staleness=8)
    lz = table._b4c_lazy
    ids = torch.tensor([1, 5, 9], device='cuda')
    lrs, allocs, last, last_ptr = [None], 0, None, None
    for t in range(1, 3001):
        if t == 1700:
            opt.lr = 2.5e-4
        opt.zero_grad()
        lz.catch_up(ids)
        table.grad[1] = 0.5
        opt.step()
        lrs.append(opt.lr)
        if opt._lr_dev is not last or opt._lr_dev.data_ptr() != last_ptr:      # a new device table
            allocs, last, last_ptr = allocs + 1, opt._lr_dev, opt._lr_dev.data_ptr()
    limit = math.ceil(math.log2(3000 / 1024)) + 1
    assert allocs <= limit, 'the lr_t table was allocated %d times in 3000 steps' % allocs
    want = np.array([0.0] + [_lr_t(lrs[s], s) for s in range(1, 3001)], dtype=np.float64).astype(np.float32)
    got = opt.lr_hist(3000)[:3001].cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    sd['lr'] = 1e-4
    opt.load_state_dict(sd)
    got = opt.lr_hist(3000)[:3001].cpu().numpy()
    want = np.array([0.0] + [_lr_t(1e-4, s) for s in range(1, 3001)], dtype=np.float64).astype(np.float32)
    assert np.array_equal(got, want)
    opt.zero_grad()
    lz.catch_up(ids)
    opt.step()
    assert float(opt.lr_hist(3001)[3001].cpu()) == np.float32(_lr_t(1e-4, 3001))
    assert opt._lr_dev is last, 'load_state_dict / the next step reallocated a table that had room'


def test_zero_grad_keeps_the_forward_pass_row_notes():
    """zero_grad() between the forward pass and backward: the rows the forward read still take this step"""
    from bert4clickpath_amd import optim
    table = torch.nn.Parameter(torch.randn(200, 16).cuda() * 0.05)
    ref = torch.nn.Parameter(table.detach().clone())
    ol, od = optim.Adam([table], lazy_rows=[table], max_staleness=1000), optim.Adam([ref])
    lz = table._b4c_lazy
    for t in range(3):
        ids = torch.tensor([3 + t, 50], device='cuda')
        lz.catch_up(ids)                    # forward
        ol.zero_grad()
        od.zero_grad()
        assert len(lz.touched) == 1
        for p in (table, ref):
            p.grad[ids] = 1.0 + t           # backward
        ol.step()
        od.step()
        assert float(table.grad.abs().max()) == 0.0 and not lz.touched
    ol.sync_rows()
    assert torch.equal(table.detach(), ref.detach()) and torch.equal(ol.m, od.m) and torch.equal(ol.v, od.v)


# ---- B. lazy against dense through the model, bit for bit ------------------------------------------------------------
V, B, S = 3000, 48, 48


def _model(head='softmax', two_features=False, seed=5, vocab=V):
    from bert4clickpath_amd.clickstream_transformer import (ClickstreamTransformer, ClozeMaskedItemPrediction,
                                                            SampledSoftmaxHead, SoftMaxHead)
    torch.manual_seed(seed)
    chains, vocabs, dims = {'items': ['asin']}, {'items': ['i%d' % i for i in range(vocab)]}, {'items': 128}
    if two_features:
        chains['actions'], vocabs['actions'], dims = ['act'], ['a%d' % i for i in range(20)], {'items': 96, 'actions': 32}
    hd = {'softmax': lambda: SoftMaxHead([64, 128], vocab), 'tied': lambda: ClozeMaskedItemPrediction([64], vocab),
          'sampled': lambda: SampledSoftmaxHead([64, 128], vocab, num_sampled=512)}[head]()
    m = ClickstreamTransformer(chains, vocabs, dims, hd, value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2,
                               dropout_rate=0.1, compute_dtype=torch.bfloat16)
    if head == 'tied':
        hd.tie(m.transformer.embedding_layers['items'].weight)
    return m.to('cuda')


def _optimizer(model, lazy):
    """as bench.py builds it: the arena in backward order, the embedding tables and a sampled projection row-lazy"""
    import bench
    from bert4clickpath_amd import optim
    rows = [p for n, p in model.named_parameters() if 'embedding_layers' in n or n == 'head.output_embedding'] if lazy else []
    return optim.Adam(model.parameters(), order=bench.backward_order(model), lazy_rows=rows)


def _batches(n, two_features=False, vocab=V):
    from bert4clickpath_amd import input_pipeline
    out = []
    for i in range(n):
        b = input_pipeline.synthetic_cloze_batch(B, S, vocab, seed=300 + i, min_len=10, n_extra_features=1 if two_features else 0,
                                                 extra_vocab=20)
        feats = {'asin': torch.from_numpy(b['ids'])[:, 2:S - 1].contiguous().cuda()}
        if two_features:
            feats['act'] = torch.from_numpy(b['extra'][0])[:, 2:S - 1].contiguous().cuda()
        out.append((feats, torch.from_numpy(b['labels_padded']).cuda(), int((b['ids'] != 0).sum())))
    return out


def _loss(model, batch):
    feats, labels, n_real = batch
    return model.cloze_loss(feats, labels, training=True, max_masked_per_row=10, n_real_tokens=n_real)


def _evaluate(model, batch):
    from bert4clickpath_amd.cloze import ClozeMaskedNDCG, ClozeMaskedRecall
    feats, labels, n_real = batch
    out = []
    with torch.no_grad():
        for scores in (None, 'lazy'):
            y = model(feats, training=False, max_matches=10, n_real_tokens=n_real, scores=scores)
            rec, nd = ClozeMaskedRecall(10), ClozeMaskedNDCG(10)
            rec.update_state(labels, y)
            nd.update_state(labels, y)
            out += [float(rec.result()), float(nd.result())]
    return out


def _train(loop, lazy, steps=4, head='softmax', two_features=False, tmp=None, vocab=V, check=None):
    """-> (losses, evaluation numbers, flat, m, v) after sync_rows"""
    from bert4clickpath_amd import checkpoint
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    model = _model(head, two_features, vocab=vocab)
    opt = _optimizer(model, lazy)
    T.set_dropout_seed(777)
    data = _batches(steps + 1, two_features, vocab)
    plateau = checkpoint.ReduceLROnPlateau(opt, patience=1)
    losses, evals = [], []
    for i in range(steps):
        if loop == 'checkpoint' and i == 2 and tmp is not None:
            path = checkpoint.save_checkpoint(os.path.join(tmp, 'ckpt-lazy'), model, opt, epoch=i)
            model = _model(head, two_features, seed=99, vocab=vocab)          # fresh model and optimizer, other weights
            opt = _optimizer(model, lazy)
            T.set_dropout_seed(5)
            checkpoint.load_checkpoint(path, model, opt)
        if loop == 'forward_first':
            loss = _loss(model, data[i])
            opt.zero_grad()
            loss.backward()
        elif loop == 'accumulate':
            opt.zero_grad()
            loss = _loss(model, data[i])
            loss.backward()
            loss2 = _loss(model, data[i + 1])
            loss2.backward()
            losses.append(float(loss2.detach()))
        else:
            opt.zero_grad()
            loss = _loss(model, data[i])
            loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if loop == 'evaluate':
            evals += _evaluate(model, data[steps])
        if loop == 'lr':
            r = plateau.on_epoch_end(i, 1.0)          # no improvement after the first: lr * 0.317 after step 2
            if r is not None:
                evals.append(r)
        if check is not None:
            check(model, opt)
    opt.sync_rows()
    torch.cuda.synchronize()
    return losses, evals, opt.arena.flat.clone(), opt.m.clone(), opt.v.clone()


def _assert_same(d, l):
    assert d[0] == l[0], ('losses', d[0], l[0])
    assert d[1] == l[1], ('evaluation', d[1], l[1])
    for what, x, y in zip(('parameters', 'first moments', 'second moments'), d[2:], l[2:]):
        assert torch.equal(x, y), '%s differ in %d of %d elements (max %g)' % (what, int((x != y).sum()), x.numel(),
                                                                             float((x - y).abs().max()))


@pytest.mark.parametrize('loop,head,two', [
    ('bench_order', 'softmax', False),
    ('forward_first', 'softmax', False),
    ('accumulate', 'softmax', False),
    ('evaluate', 'softmax', False),
    ('lr', 'softmax', False),
    ('bench_order', 'softmax', True),
    ('bench_order', 'tied', False),
])
def test_lazy_equals_dense_through_the_model(loop, head, two):
    """the same model, batches and dropout stream under optim.Adam(model.parameters()) and under the row-lazy optimizer
    (embedding tables in lazy_rows, arena in bench.py's order): every loss, the arena and both moments bit for bit"""
    d = _train(loop, False, head=head, two_features=two)
    l = _train(loop, True, head=head, two_features=two)
    if loop == 'lr':
        assert d[1] and d[1] == l[1], 'the lr never changed'
    _assert_same(d, l)


def test_lazy_checkpoint_round_trip_equals_the_uninterrupted_run(tmp_path):
    """save_checkpoint after step 2, load into a fresh model and a fresh lazy optimizer, continue: equal to the run never
    interrupted (which equals the dense run)"""
    d = _train('bench_order', False)
    l = _train('checkpoint', True, tmp=str(tmp_path))
    _assert_same(d, l)


# ---- C. the sampled head (config 5 shape, reduced) --------------------------------------------------------------------
VS = 20011


def _check_every_row_current(model, opt):
    """after a step: both lazy tables' gradients all zero; after sync_rows() every row current -- stamp == iterations, or
    stamp 0 for a row that never had a gradient (its moments all zero: nothing to replay)"""
    assert len(opt.lazy) == 2
    for lz in opt.lazy:
        assert float(lz.p.grad.abs().max()) == 0.0, 'a lazy table kept gradient rows after the step'
    opt.sync_rows()
    for lz in opt.lazy:
        _, _, m, v = lz._slices()
        live = (m.view(lz.rows, lz.width) != 0).any(1) | (v.view(lz.rows, lz.width) != 0).any(1)
        ok = (lz.stamp == opt.iterations) | ((lz.stamp == 0) & ~live)
        assert bool(ok.all()), 'rows not current after sync_rows: %d' % int((~ok).sum())
        assert bool((lz.stamp[live] == opt.iterations).all())


@pytest.mark.parametrize('loop', ['bench_order', 'forward_first', 'checkpoint'])
def test_sampled_head_lazy_against_dense(loop, tmp_path):
    """SampledSoftmaxHead, V = 20,011, output_embedding and the item table row-lazy as in bench.py.  The head's row scatter
    adds with float atomics, so the two runs differ by rounding: |dense - lazy| <= 2e-5 over the arena (the bound of
    test_gpu_parallel's two-rank check; elements whose gradient is identically zero in exact arithmetic -- the key
    projections' biases -- are left out: Adam's 1e-9 epsilon turns their rounding noise into full steps).  One lost row
    update is lr_t * m / sqrt(v) ~ 1e-4 .. 1e-3 at these steps: 5x to 50x the bound.  After every step: both tables'
    gradients all zero, every row's stamp == iterations once sync_rows() ran."""
    d = _train('bench_order' if loop != 'forward_first' else loop, False, steps=3, head='sampled', vocab=VS)
    l = _train(loop, True, steps=3, head='sampled', vocab=VS, tmp=str(tmp_path), check=_check_every_row_current)
    assert np.allclose(d[0], l[0], rtol=1e-3, atol=1e-3), (d[0], l[0])
    model = _model('sampled', vocab=VS)
    opt = _optimizer(model, False)
    diff = (d[2] - l[2]).abs()
    for n, p in model.named_parameters():
        if n.endswith('mha.wk.bias'):
            lo, hi = opt.arena.slice_of(p)
            diff[lo:hi] = 0
    assert float(diff.max()) <= 2e-5, 'max |dense - lazy| %g at %d' % (float(diff.max()), int(diff.argmax()))


# ---- D. two ranks with the lazy optimizer -------------------------------------------------------------------------------
def _worker(rank, world, port, out_dir, fill):
    from test_gpu_parallel import _batch, _model as _pmodel
    multi = torch.cuda.device_count() >= world
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank if multi else 0), B4C_DIST_BACKEND='nccl' if multi else 'gloo',
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    from bert4clickpath_amd import optim, parallel
    parallel.init_distributed()
    torch.cuda.set_device(rank if multi else 0)
    model = _pmodel()
    table = model.transformer.embedding_layers['items'].weight
    opt = optim.Adam(model.parameters(), lazy_rows=[table], max_staleness=4)
    head_end = max(opt.arena.slice_of(p)[1] for n, p in model.named_parameters() if n.startswith('head.'))
    red = parallel.GradReducer(opt.arena, bucket_bounds=[head_end], reduce='sum', sparse_params=[table], sparse_max_fill=fill)
    items, labels, flat = _batch(rank)
    kinds = []
    for step in range(3):
        opt.zero_grad()
        red.begin_backward()
        loss = model.cloze_loss({'asin': items}, labels, training=True, flat_idx=flat)
        loss.backward()
        ids = torch.cat([torch.full((items.shape[0], 2), 3, device=items.device), items,
                         torch.full((items.shape[0], 1), 4, device=items.device)], dim=1)
        ids[:, 1] = 4
        red.set_touched_rows(table, ids)
        red.finish()
        kinds.append(red.last_exchange[id(table)])
        opt.step(red.grad_mul)
        assert float(table.grad.abs().max()) == 0.0
    opt.sync_rows()
    torch.cuda.synchronize()
    np.save(os.path.join(out_dir, 'rank%d.npy' % rank), opt.arena.flat.cpu().numpy())
    with open(os.path.join(out_dir, 'kind%d.txt' % rank), 'w') as f:
        f.write(','.join(kinds))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize('fill,kind', [(8.0, 'sparse'), (1e-6, 'dense')])
def test_two_ranks_with_a_lazy_table(tmp_path, fill, kind):
    """2 ranks, 3 steps, the item table row-lazy under parallel.GradReducer's exchange: sparse (the other rank's rows reach
    the optimizer through LazyRows.note) and its dense fallback (LazyRows.all_rows).  Replicas bit-identical, and equal to
    one process with the dense optimizer on both shards to test_gpu_parallel's 2e-5."""
    from test_gpu_parallel import _batch, _free_port, _model as _pmodel
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path), fill)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
        assert p.exitcode == 0
    for r in range(world):
        assert (tmp_path / ('kind%d.txt' % r)).read_text() == ','.join([kind] * 3)
    w0, w1 = np.load(tmp_path / 'rank0.npy'), np.load(tmp_path / 'rank1.npy')
    assert np.array_equal(w0, w1), 'replicas diverged in %d elements' % int((w0 != w1).sum())
    from bert4clickpath_amd import optim
    model = _pmodel()
    opt = optim.Adam(model.parameters())
    shards = [_batch(r) for r in range(world)]
    for step in range(3):
        opt.zero_grad()
        for items, labels, flat in shards:
            model.cloze_loss({'asin': items}, labels, training=True, flat_idx=flat).backward()
        opt.step()
    ref = opt.arena.flat.cpu().numpy()
    diff = np.abs(ref - w0)
    for n, p in model.named_parameters():
        if n.endswith('mha.wk.bias'):
            lo, hi = opt.arena.slice_of(p)
            diff[lo:hi] = 0
    assert float(diff.max()) < 2e-5, float(diff.max())
