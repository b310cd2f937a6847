"""Global-norm gradient clipping (optim.Adam(global_clipnorm=...), csrc/gradnorm.hip) and learning-rate schedules on the device.

A. The norm kernels against float64, and the row form against the dense form bit for bit.
B. Adam with clipping / with a schedule over long irregular histories against float64 Keras Adam, dense and row-lazy side by
   side (the loop of test_gpu_lazy_training.test_adam_kernels_match_float64_over_long_histories); a clip that never bites.
C. Through the model: last_grad_norm, lazy == dense, a checkpoint round trip of a scheduled, clipped run; no host sync in step().
D. Two ranks.

The float64 clip restated here (oracle/numpy_ref.adam_step takes the gradient it is given):  g <- g mul min(1, clip / ||g mul||)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_lazy_training import B1, B2, EPS, _grad_schedule, _lr_t, _magnitudes, _tolerance

pytestmark = pytest.mark.gpu

CHUNK, GROUP = 1024, 4096


# ---- A. the norm kernels ------------------------------------------------------------------------------------------------
def _norm(grad, lo, hi, clip, mul=1.0, ids=None, table=None):
    """-> (partial, total, norm, coef) on the host.  ids / table = (table_lo, rows, width): the row form instead of [lo, hi)"""
    from bert4clickpath_amd import ops
    n_chunks = ops.grad_chunks(grad.numel())
    partial = torch.zeros(n_chunks, dtype=torch.float64, device='cuda')
    groups = torch.full(((n_chunks + GROUP - 1) // GROUP,), 7.0, dtype=torch.float64, device='cuda')
    total = torch.full((1,), -1.0, dtype=torch.float64, device='cuda')
    nc = torch.full((2,), -1.0, dtype=torch.float32, device='cuda')
    if ids is None:
        ops.grad_sumsq_(grad, lo, hi, partial)
    else:
        for i in ids:
            ops.grad_sumsq_rows_(grad, table[0], table[1], table[2], i, partial)
    ops.grad_clip_coef_(partial, groups, clip, mul, total, nc)
    torch.cuda.synchronize()
    return partial.cpu(), total.cpu(), nc[:1].cpu().numpy()[0], nc[1:].cpu().numpy()[0]


def _ulps(got, want64):
    want = np.float32(want64)
    return abs(float(got) - float(want)) / float(np.spacing(want)) if want != 0 else abs(float(got))


def _arena(n, seed, offset=64):
    """fp32 arena of n elements that starts `offset` elements into its allocation, magnitudes 1e-20 / 1 / 1e15 by position"""
    rng = np.random.default_rng(seed)
    scale = _magnitudes(n)
    host = (rng.standard_normal(n) * scale).astype(np.float32)
    buf = torch.zeros(n + offset + 64, device='cuda')
    buf[offset:offset + n].copy_(torch.from_numpy(host))
    return buf[offset:offset + n], host


@pytest.mark.parametrize('n,lo,hi', [
    (5 * CHUNK + 3 * 64 + 1, 0, 5 * CHUNK + 3 * 64 + 1),          # the whole arena: a last chunk of 193 elements
    (5 * CHUNK + 3 * 64 + 1, 192, 4099),                           # 64-aligned start inside chunk 0, ragged end inside chunk 4
    (7 * CHUNK + 2, 3 * CHUNK + 64, 7 * CHUNK + 2),               # up to the arena's ragged end
    (3 * CHUNK, 2 * CHUNK - 64, 2 * CHUNK + 3),                    # two chunks, one element past a chunk boundary... and 3
    (GROUP * CHUNK + 3 * CHUNK + 77, 0, GROUP * CHUNK + 3 * CHUNK + 77),      # more than one group of partials
])
def test_norm_kernel_matches_float64(n, lo, hi):
    """partial[c] covers the WHOLE chunk for every chunk that overlaps [lo, hi): the float64 reference is the sum over that
    extent.  norm within 2 ulp(fp32) of the float64 value, the coefficient within 1 ulp; two launches: identical bits."""
    grad, host = _arena(n, seed=n + lo)
    e_lo, e_hi = lo // CHUNK * CHUNK, min(-(-hi // CHUNK) * CHUNK, n)
    ref_total = float(np.sum(host[e_lo:e_hi].astype(np.float64) ** 2))
    for mul in (1.0, 0.5, -3.0):
        ref_norm = math.sqrt(ref_total) * abs(mul)
        for clip, bites in ((0.37 * ref_norm, True), (3.0 * ref_norm, False)):
            clip = float(np.float32(clip))
            partial, total, norm, coef = _norm(grad, lo, hi, clip, mul)
            assert abs(float(total) - ref_total) <= 1e-12 * ref_total
            assert _ulps(norm, ref_norm) <= 2, (norm, ref_norm)
            ref_coef = clip / ref_norm if bites else 1.0
            assert _ulps(coef, ref_coef) <= 1, (coef, ref_coef)
            assert bites or coef == np.float32(1.0)
            # chunks outside the range were not written
            c_lo, c_hi = lo // CHUNK, -(-hi // CHUNK)
            assert float(partial[:c_lo].abs().sum()) == 0.0 and float(partial[c_hi:].abs().sum()) == 0.0
            again = _norm(grad, lo, hi, clip, mul)
            assert torch.equal(partial, again[0]) and torch.equal(total, again[1])
            assert np.float32(norm).tobytes() == np.float32(again[2]).tobytes() and np.float32(coef).tobytes() == np.float32(again[3]).tobytes()


def test_norm_kernel_zero_and_non_finite_gradients():
    n = 3 * CHUNK + 5
    zero = torch.zeros(n, device='cuda')
    _, total, norm, coef = _norm(zero, 0, n, 1.0)
    assert float(total) == 0.0 and norm == 0.0 and coef == np.float32(1.0)
    for bad in (float('inf'), float('-inf'), float('nan')):
        grad, _ = _arena(n, seed=1)
        grad[2 * CHUNK + 7] = bad
        _, total, norm, coef = _norm(grad, 0, n, 1.0)
        assert np.isnan(coef) and not np.isfinite(norm)


@pytest.mark.parametrize('width', [4, 8, 100, 128, 256])
def test_row_form_equals_dense_form_bit_for_bit(width):
    """a (rows, width) table inside an arena at a 64-aligned, not chunk-aligned offset; several id lists per step with
    repeats and out-of-range ids (clamped as the Adam row kernel clamps them); the gradient non-zero on exactly the named
    rows.  Width 100: rows straddle chunks; width 4: 256 rows share one."""
    rows, table_lo = 1531, 192
    n = table_lo + rows * width + 64 + 3
    rng = np.random.default_rng(width)
    lists = [rng.integers(0, rows, 40), np.array([5, 5, 5, rows - 2, -7, rows + 100, 2 ** 40]), rng.integers(0, rows, 9).repeat(3),
             np.array([rows // 2])]
    named = np.unique(np.clip(np.concatenate(lists), 0, rows - 1))
    assert 0 in named and rows - 1 in named
    host = np.zeros(n, dtype=np.float32)
    table = host[table_lo:table_lo + rows * width].reshape(rows, width)
    table[named] = (rng.standard_normal((named.size, width)) * _magnitudes(named.size)[:, None]).astype(np.float32)
    host[5] = 2.5                                                   # a dense neighbour in the table's first chunk
    grad = torch.from_numpy(host).cuda()
    ids = [torch.from_numpy(np.asarray(l, dtype=np.int64)).cuda() for l in lists]
    dense = _norm(grad, 0, n, 1.0)
    lazy = _norm(grad, 0, 0, 1.0, ids=ids, table=(table_lo, rows, width))
    assert float(dense[1]) > 0
    assert torch.equal(dense[0], lazy[0]), int((dense[0] != lazy[0]).sum())
    assert torch.equal(dense[1], lazy[1])
    assert np.float32(dense[2]).tobytes() == np.float32(lazy[2]).tobytes() and np.float32(dense[3]).tobytes() == np.float32(lazy[3]).tobytes()
    assert abs(float(dense[1]) - float(np.sum(host.astype(np.float64) ** 2))) <= 1e-12 * float(dense[1])


# ---- B. Adam with clipping / a schedule over long histories ----------------------------------------------------------------
def _mul(t):
    return 0.5 if t % 4 == 0 else (3.0 if t % 7 == 0 else 1.0)


def _history(rows, width, T, staleness, clip=None, schedule=None, lr_change=None, oracle=True):
    """T steps of the dense and of the row-lazy optimizer on the same gradients; float64 Keras Adam beside them.
    -> dict(pd, pl, od, ol, P, lr_sum, on, p0, norms)"""
    from bert4clickpath_amd import optim
    from oracle import numpy_ref as nr
    on = _grad_schedule(rows, T, staleness, seed=rows)
    scale = _magnitudes(rows)
    rng = np.random.default_rng(width)
    grads = [None] + [(rng.standard_normal((rows, width)) * scale[:, None] * on[t][:, None]).astype(np.float32) for t in range(1, T + 1)]
    norms = np.array([0.0] + [math.sqrt(float(np.sum((grads[t].astype(np.float64) * _mul(t)) ** 2))) for t in range(1, T + 1)])
    if clip == 'median':
        # a condition on the INPUTS, checked from the float64 side before anything runs on the device
        clip = float(np.float32(np.median(norms[1:])))
        clipped = norms[1:] > clip
        assert clipped.sum() >= T / 3 and (~clipped).sum() >= T / 3, (int(clipped.sum()), T)
        assert (np.abs(norms[1:] - clip) > 1e-6 * clip).all(), 'a step ties with the clip: fp32 and float64 may branch differently'
    g0 = torch.Generator().manual_seed(rows + width)
    p0 = torch.randn(rows, width, generator=g0) * 0.05
    dense_p, lazy_p = torch.nn.Parameter(p0.clone().cuda()), torch.nn.Parameter(p0.clone().cuda())
    lr0 = schedule if schedule is not None else 1e-3
    od = optim.Adam([dense_p], learning_rate=lr0, global_clipnorm=clip)
    ol = optim.Adam([lazy_p], learning_rate=lr0, lazy_rows=[lazy_p], max_staleness=staleness, global_clipnorm=clip)
    lz = lazy_p._b4c_lazy
    P, M, V = p0.double().numpy(), np.zeros((rows, width)), np.zeros((rows, width))
    lr, lr_sum = 1e-3, 0.0
    for t in range(1, T + 1):
        if lr_change is not None and t == lr_change[0]:
            od.lr = ol.lr = lr = lr_change[1]
        if schedule is not None:
            lr = schedule(t - 1)
            assert od.lr == lr and ol.lr == lr
        mul, g = _mul(t), grads[t]
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
        if oracle:
            g64 = g.astype(np.float64) * mul
            if clip is not None and norms[t] > clip:
                g64 = g64 * (clip / norms[t])
            P, M, V = nr.adam_step(P, g64, M, V, t, lr=lr, beta1=B1, beta2=B2, eps=EPS)
            lr_sum += _lr_t(lr, t)
        assert float(lazy_p.grad.abs().max()) == 0.0, t
    ol.sync_rows()
    torch.cuda.synchronize()
    return dict(pd=dense_p.detach().cpu().numpy(), pl=lazy_p.detach().cpu().numpy(), od=od, ol=ol, P=P, lr_sum=lr_sum, on=on,
                p0=p0.numpy(), norms=norms, clip=clip)


def _assert_lazy_equals_dense(h):
    pd, pl = h['pd'], h['pl']
    assert np.array_equal(pd, pl), 'lazy != dense in %d elements' % int((pd != pl).sum())
    assert torch.equal(h['od'].m, h['ol'].m) and torch.equal(h['od'].v, h['ol'].v)
    assert np.isfinite(pd).all()
    never = ~h['on'].any(axis=0)
    assert np.array_equal(pd[never], h['p0'][never]), 'rows without a gradient moved'


def _assert_within_tolerance(h, T, what):
    err = np.abs(h['pd'].astype(np.float64) - h['P'])
    tol = _tolerance(h['P'], h['pd'], h['lr_sum'], T)
    ratio = float((err / tol).max())
    print('%s: worst |p - p64| / bound = %.4f (worst error %.3g)' % (what, ratio, float(err.max())))
    assert ratio <= 1.0, '%s: fp32 Adam off float64: worst error / bound = %g' % (what, ratio)


@pytest.mark.parametrize('rows,width', [(1003, 4), (517, 8), (301, 128), (97, 256)])
def test_clipped_adam_matches_float64_over_long_histories(rows, width):
    """300 steps, lr change at 150, grad_mul in {0.5, 1, 3}, max_staleness 16, gradients 1e-20 .. 1e15, clip = the median of
    the float64 norms of the sequence (at least a third of the steps clip, a third do not, none ties within 1e-6).  The bound
    is the project's own (test_gpu_lazy_training._tolerance, c = 256): Adam's update is invariant to first order under a
    common scale of g, and the clip adds two roundings to g (the coefficient's, and mul * coef).
    Worst error / bound observed on an MI355X: 0.117 (1003x4), 0.124 (517x8), 0.139 (301x128), 0.141 (97x256) -- the unclipped
    loop of test_gpu_lazy_training sits in the same place, so c = 256 stands."""
    T = 300
    h = _history(rows, width, T, 16, clip='median', lr_change=(150, 3.17e-4))
    _assert_lazy_equals_dense(h)
    _assert_within_tolerance(h, T, 'clipped %dx%d' % (rows, width))
    # the logged norm of the last step is the float64 one
    assert _ulps(float(h['od'].last_grad_norm), h['norms'][T]) <= 2
    assert h['od'].last_grad_norm.dim() == 0 and torch.equal(h['od'].last_grad_norm, h['ol'].last_grad_norm)


@pytest.mark.parametrize('rows,width', [(1003, 4), (301, 128)])
def test_a_clip_that_never_bites_changes_no_bit(rows, width):
    """global_clipnorm=1e30 (coefficient exactly 1.0f every step) against global_clipnorm=None, dense and lazy, 50 steps"""
    a = _history(rows, width, 50, 16, clip=None, oracle=False)
    b = _history(rows, width, 50, 16, clip=1e30, oracle=False)
    assert a['od'].last_grad_norm is None and b['od'].last_grad_norm is not None
    for x, y in ((a['pd'], b['pd']), (a['pl'], b['pl'])):
        assert np.array_equal(x, y)
    for k in ('od', 'ol'):
        assert torch.equal(a[k].m, b[k].m) and torch.equal(a[k].v, b[k].v)
    _assert_lazy_equals_dense(b)


def test_clipnorm_can_be_switched_between_steps():
    """a plain attribute: None launches nothing new and leaves last_grad_norm alone; a value clips from the next step on"""
    from bert4clickpath_amd import optim
    p = torch.nn.Parameter(torch.zeros(8, 8).cuda())
    o = optim.Adam([p])
    p.grad.fill_(2.0)
    o.step()
    assert o.last_grad_norm is None
    o.global_clipnorm = 4.0
    p.grad.fill_(2.0)
    o.step()
    assert float(o.last_grad_norm) == 16.0          # 64 elements of 2.0
    with pytest.raises(ValueError):
        o.global_clipnorm = 0.0


@pytest.mark.parametrize('rows,width', [(517, 8), (301, 128)])
def test_schedule_composes_with_lazy_rows(rows, width):
    """CustomLRSchedule(d, warmup_steps=20) over 60 steps, rows touched every ~max_staleness steps: every replayed step uses
    its own lr_t out of the schedule.  lazy == dense bit for bit, both within the bound of float64 with lr_sum accumulated from
    the schedule."""
    from clickstream_transformer.training_utils import CustomLRSchedule
    T = 60
    h = _history(rows, width, T, 16, schedule=CustomLRSchedule(width, warmup_steps=20))
    _assert_lazy_equals_dense(h)
    assert not np.array_equal(h['pd'], h['p0'])
    _assert_within_tolerance(h, T, 'scheduled %dx%d' % (rows, width))
    h = _history(rows, width, T, 16, schedule=CustomLRSchedule(width, warmup_steps=20), clip='median')
    _assert_lazy_equals_dense(h)
    _assert_within_tolerance(h, T, 'scheduled, clipped %dx%d' % (rows, width))


# ---- C. through the model --------------------------------------------------------------------------------------------------
V, B, S = 3000, 48, 48


def _model(dtype, seed=5):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(seed)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': 128}, SoftMaxHead([64, 128], V),
                               value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, dropout_rate=0.1,
                               compute_dtype=dtype)
    return m.to('cuda')


def _optimizer(model, lazy, **kw):
    import bench
    from bert4clickpath_amd import optim
    rows = [p for n, p in model.named_parameters() if 'embedding_layers' in n] if lazy else []
    return optim.Adam(model.parameters(), order=bench.backward_order(model), lazy_rows=rows, **kw)


def _batches(n):
    from bert4clickpath_amd import input_pipeline
    out = []
    for i in range(n):
        b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=300 + i, min_len=10)
        out.append(({'asin': torch.from_numpy(b['ids'])[:, 2:S - 1].contiguous().cuda()}, torch.from_numpy(b['labels_padded']).cuda(),
                    int((b['ids'] != 0).sum())))
    return out


def _loss(model, batch):
    feats, labels, n_real = batch
    return model.cloze_loss(feats, labels, training=True, max_masked_per_row=10, n_real_tokens=n_real)


CLIP = 0.05          # below the norm of the first steps' gradient (asserted from the float64 norm)


def _train(dtype, lazy, steps=10, schedule=False, tmp=None, sync_debug=False):
    """steps 0..: bench order; 3..5 forward -> zero_grad -> backward -> step; 6.. two accumulated micro-batches.
    -> (losses, norms (device), float64 norms of the arena's gradient, flat, m, v)"""
    from bert4clickpath_amd import checkpoint
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    from clickstream_transformer.training_utils import WarmupLinearDecay
    kw = dict(global_clipnorm=CLIP)
    if schedule:
        kw['learning_rate'] = WarmupLinearDecay(2e-3, 3, 40)
    model = _model(dtype)
    opt = _optimizer(model, lazy, **kw)
    T.set_dropout_seed(777)
    data = _batches(steps + 1)
    losses, norms, norms64 = [], [], []
    for i in range(steps):
        if tmp is not None and i == steps // 2:
            path = checkpoint.save_checkpoint(os.path.join(tmp, 'ckpt-clip'), model, opt, epoch=i)
            model = _model(dtype, seed=99)
            if schedule:
                kw['learning_rate'] = WarmupLinearDecay(2e-3, 3, 40)       # the schedule is the caller's to construct again
            opt = _optimizer(model, lazy, **kw)
            T.set_dropout_seed(5)
            checkpoint.load_checkpoint(path, model, opt)
            assert opt.iterations == i
        if 3 <= i < 6:
            loss = _loss(model, data[i])
            opt.zero_grad()
            loss.backward()
        else:
            opt.zero_grad()
            loss = _loss(model, data[i])
            loss.backward()
            if i >= 6:
                _loss(model, data[i + 1]).backward()
        from bert4clickpath_amd import ops
        ops.flush_pending_dw(opt.arena.ctx)
        ops.join_side_work(opt.arena.ctx)
        norms64.append(math.sqrt(float((opt.arena.grad.double() ** 2).sum())))
        if sync_debug and i >= 1:
            torch.cuda.set_sync_debug_mode('error')
            try:
                opt.step()
            finally:
                torch.cuda.set_sync_debug_mode('default')
        else:
            opt.step()
        norms.append(float(opt.last_grad_norm))
        losses.append(float(loss.detach()))
    opt.sync_rows()
    torch.cuda.synchronize()
    return losses, norms, norms64, opt.arena.flat.clone(), opt.m.clone(), opt.v.clone()


def _assert_same_run(d, l):
    assert d[0] == l[0], ('losses', d[0], l[0])
    assert d[1] == l[1], ('norms', d[1], l[1])
    for what, x, y in zip(('parameters', 'first moments', 'second moments'), d[3:], l[3:]):
        assert torch.equal(x, y), '%s differ in %d of %d elements' % (what, int((x != y).sum()), x.numel())


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_clipping_through_the_model(dtype):
    """cloze_loss -> backward -> step with a clip below the first steps' norm: last_grad_norm is the float64 norm of the arena's
    gradient (copied out before the step) rounded to fp32; the row-lazy optimizer and the dense one bit-identical after 10
    steps that include the forward -> zero_grad -> backward -> step order and two accumulated micro-batches."""
    d = _train(dtype, False)
    assert all(n64 > CLIP * 1.001 for n64 in d[2][:3]), ('the first steps do not clip', d[2][:3])
    for got, want in zip(d[1], d[2]):
        assert _ulps(got, want) <= 2, (got, want)
    l = _train(dtype, True)
    _assert_same_run(d, l)
    assert np.isfinite(d[0]).all() and bool(torch.isfinite(d[3]).all())


def test_scheduled_clipped_checkpoint_round_trip(tmp_path):
    """save in the middle of a scheduled, clipped, row-lazy run; load into a fresh model and optimizer built with the same
    schedule; continue: equal to the run never interrupted, bit for bit"""
    a = _train(torch.bfloat16, True, steps=6, schedule=True)
    b = _train(torch.bfloat16, True, steps=6, schedule=True, tmp=str(tmp_path))
    _assert_same_run(a, b)


def test_step_makes_no_host_sync():
    """steps 2.. under torch.cuda.set_sync_debug_mode('error'), dense and lazy, clipped and scheduled.  The mode sees
    torch-side synchronisation only (the library's own calls are launches and hipMemsetAsync: csrc/gradnorm.hip, rowops.hip)."""
    probe = torch.ones(1, device='cuda')
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
    finally:
        torch.cuda.set_sync_debug_mode('default')
    if not honoured:
        pytest.skip('this torch build does not raise on a synchronising call under set_sync_debug_mode("error")')
    for lazy in (False, True):
        _train(torch.bfloat16, lazy, steps=4, schedule=True, sync_debug=True)


# ---- D. two ranks ------------------------------------------------------------------------------------------------------------
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
    opt = optim.Adam(model.parameters(), lazy_rows=[table], max_staleness=4, global_clipnorm=0.05)
    head_end = max(opt.arena.slice_of(p)[1] for n, p in model.named_parameters() if n.startswith('head.'))
    red = parallel.GradReducer(opt.arena, bucket_bounds=[head_end], reduce='mean', sparse_params=[table], sparse_max_fill=fill)
    items, labels, flat = _batch(rank)
    kinds, norms = [], []
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
        norms.append(opt.last_grad_norm.cpu().numpy().copy())
        assert float(table.grad.abs().max()) == 0.0
    opt.sync_rows()
    torch.cuda.synchronize()
    np.save(os.path.join(out_dir, 'rank%d.npy' % rank), opt.arena.flat.cpu().numpy())
    np.save(os.path.join(out_dir, 'norm%d.npy' % rank), np.asarray(norms, dtype=np.float32))
    with open(os.path.join(out_dir, 'kind%d.txt' % rank), 'w') as f:
        f.write(','.join(kinds))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize('fill,kind', [(8.0, 'sparse'), (1e-6, 'dense')])
def test_two_ranks_clip_identically(tmp_path, fill, kind):
    """2 ranks, 3 steps, clipping on, reduce='mean' (the clip applies to the mean gradient), the item table row-lazy under the
    row-sparse exchange and under its dense fallback: replicas and their logged norms bit-identical, every step clipped"""
    from test_gpu_parallel import _free_port
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
    n0, n1 = np.load(tmp_path / 'norm0.npy'), np.load(tmp_path / 'norm1.npy')
    assert n0.tobytes() == n1.tobytes(), (n0, n1)
    assert (n0 > 0.05).all() and np.isfinite(n0).all(), n0
