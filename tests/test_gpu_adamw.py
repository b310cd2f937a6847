"""Decoupled weight decay (optim.Adam(weight_decay=...), Keras AdamW; b4c_adamw_step / b4c_adamw_rows) on the device.

1. Row-lazy == dense, bit for bit, with never-touched rows that move every step (the harness of test_gpu_lazy_adam).
2. An excluded parameter / a whole excluded lazy table takes exactly the update it takes without decay.
3. weight_decay=0.0 changes no bit against None; None never reaches the new entry points.
4. Both kernels, clipped and unclipped, against float64 over 300 steps.
5. Through the model (clip 5, WarmupLinearDecay, weight_decay 0.01, no_decay_params): lazy == dense, a checkpoint round trip,
   no host sync in step().
6. Two ranks.

The float64 AdamW restated here (the reference never decays, so oracle/numpy_ref has none):
    P <- P - (lr * wd) * P;   P, M, V <- numpy_ref.adam_step(P, g, M, V, t, lr)        with lr the plain rate of step t."""
import contextlib
import inspect
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_clipnorm import _assert_same_run, _batches, _loss, _model, _mul, _optimizer
from test_gpu_lazy_training import B1, B2, EPS, _grad_schedule, _lr_t, _magnitudes, _tolerance

pytestmark = pytest.mark.gpu

WD = 0.01


@contextlib.contextmanager
def _adamw_calls():
    """-> a dict that counts, while the block runs, the calls of ops.adam_step_ / ops.adam_rows_ that carry a decay ('step',
    'rows') and the calls that reach the C entry points b4c_adamw_step / b4c_adamw_rows: a decayed call that the wrapper
    routed to b4c_adam_step / b4c_adam_rows (or their clipped forms) would leave the C count behind"""
    from bert4clickpath_amd import _lib, ops
    lib = _lib.lib()
    n = {'step': 0, 'rows': 0, 'b4c_adamw_step': 0, 'b4c_adamw_rows': 0}
    prev = [(ops, 'adam_step_', 'step', 'decay'), (ops, 'adam_rows_', 'rows', 'decay_hist'),
            (lib, 'b4c_adamw_step', 'b4c_adamw_step', None), (lib, 'b4c_adamw_rows', 'b4c_adamw_rows', None)]
    prev = [(obj, name, key, arg, getattr(obj, name)) for obj, name, key, arg in prev]

    def counted(fn, key, arg):
        def f(*a, **k):
            if arg is None or inspect.signature(fn).bind(*a, **k).arguments.get(arg) is not None:
                n[key] += 1
            return fn(*a, **k)
        return f
    for obj, name, key, arg, fn in prev:
        setattr(obj, name, counted(fn, key, arg))
    try:
        yield n
    finally:
        for obj, name, key, arg, fn in prev:
            setattr(obj, name, fn)


# ---- 1. lazy == dense ------------------------------------------------------------------------------------------------------
def _pair(rows, width, n_dense, staleness, seed, **kw):
    from bert4clickpath_amd import optim
    g = torch.Generator().manual_seed(seed)
    out = []
    for lazy in (False, True):
        g.manual_seed(seed)
        dense = torch.nn.Parameter(torch.randn(n_dense, generator=g).cuda())
        table = torch.nn.Parameter((torch.randn(rows, width, generator=g) * 0.05).cuda())
        tail = torch.nn.Parameter(torch.randn(37, generator=g).cuda())
        opt = optim.Adam([dense, table, tail], lazy_rows=[table] if lazy else (), max_staleness=staleness, **kw)
        out.append((opt, dense, table, tail))
    return out


def _lazy_against_dense(rows, width, staleness, wd0, changes):
    """test_gpu_lazy_adam's loop (hot ids, repeats, out-of-range ids, an lr change, grad_mul, rotation slices), 25 steps, with
    weight_decay = wd0 and `changes` {step: value} applied before that step.  The last tenth of the table (short of its last
    row, which the clamped out-of-range ids name) is never read and never receives a gradient: those rows move by the decay
    alone, step by step, and must carry the dense run's bits."""
    (od, dd, td, ld), (ol, dl, tl, ll) = _pair(rows, width, 1000, staleness, seed=rows, weight_decay=wd0)
    change = bool(changes)
    rng = np.random.default_rng(rows + width)
    live = rows - max(3, rows // 10)                      # rows [live, rows - 1) are never named
    never = np.arange(live, rows - 1)
    hot = rng.integers(0, live, 5)
    t0 = td.detach().clone()
    for step in range(1, 26):
        if step == 12:
            od.lr = ol.lr = 3.17e-4
        if step in changes:
            was_off = ol.weight_decay is None and not ol._decay_seen
            od.weight_decay = ol.weight_decay = changes[step]
            if was_off and changes[step] is not None:
                # switched on in mid-run: every row is current and stamped, so max_staleness bounds the replays from here on
                assert int((tl._b4c_lazy.stamp != step - 1).sum()) == 0
                assert torch.equal(tl.detach(), td.detach())
        n = int(rng.integers(1, 400))
        ids = np.concatenate([rng.integers(0, live, n), np.repeat(hot, 50)])
        if step % 5 == 0:
            ids = np.concatenate([ids, [-3, rows + 9]])
        if step in (7, 8, 9):
            ids = hot[:1].copy()
        ids_t = torch.from_numpy(ids).cuda()
        od.zero_grad()
        ol.zero_grad()
        tl._b4c_lazy.catch_up(ids_t.view(1, -1))
        uniq = np.unique(np.clip(ids, 0, rows - 1))
        assert not np.intersect1d(uniq, never).size
        assert torch.equal(tl.detach()[uniq], td.detach()[uniq]), step
        got = uniq[rng.random(uniq.size) < 0.8]
        grad_rows = torch.from_numpy(rng.standard_normal((got.size, width)).astype(np.float32)).cuda()
        gd = torch.from_numpy(rng.standard_normal(1000).astype(np.float32)).cuda()
        for opt, d, t, l in ((od, dd, td, ld), (ol, dl, tl, ll)):
            t.grad[torch.from_numpy(got).cuda()] = grad_rows
            d.grad.copy_(gd)
            l.grad.fill_(0.25)
        mul = 0.125 if step % 4 == 0 else 1.0
        od.step(mul)
        ol.step(mul)
        assert torch.equal(dl.detach(), dd.detach()) and torch.equal(ll.detach(), ld.detach())
        assert float(tl.grad.abs().max()) == 0.0
    lz = tl._b4c_lazy
    stale = int((lz.stamp != ol.iterations).sum())
    assert stale > 0 or staleness <= 25, 'every row is current already: the catch-up in front of state_dict is not exercised'
    sd = ol.state_dict()
    torch.cuda.synchronize()
    # the never-touched rows: they exist, they moved, they carry the dense bits; their moments are still zero
    assert never.size >= 2
    nv = torch.from_numpy(never).cuda()
    assert bool((td.detach()[nv] != t0[nv]).any(dim=1).all()), 'a never-touched row of a decayed table did not move'
    assert torch.equal(tl.detach()[nv], td.detach()[nv])
    lo, hi = ol.arena.slice_of(tl)
    lo_d, hi_d = od.arena.slice_of(td)
    assert float(od.m[lo_d:hi_d].view(rows, width)[nv].abs().max()) == 0.0
    assert torch.equal(tl.detach(), td.detach())
    assert torch.equal(sd['m'][lo:hi], od.m[lo_d:hi_d]) and torch.equal(sd['v'][lo:hi], od.v[lo_d:hi_d])
    assert torch.equal(ol.arena.flat, od.arena.flat)
    assert torch.equal(ol.m, od.m) and torch.equal(ol.v, od.v)
    assert int((lz.stamp != ol.iterations).sum()) == 0    # sync() visited the never-touched rows too
    # the decay is 25 small steps: (1 - d)^25 of the start, to a relative 1e-5
    if not change:
        want = t0[nv].double() * (1 - 1e-3 * WD) ** 11 * (1 - 3.17e-4 * WD) ** 14
        assert float(((td.detach()[nv].double() - want).abs() / want.abs().clamp_min(1e-30)).max()) < 1e-5


@pytest.mark.parametrize('rows,width,staleness,change', [(5000, 256, 7, False), (300, 64, 256, False), (70000, 128, 1000, False),
                                                         (64, 8, 3, False), (5000, 256, 7, True), (300, 64, 256, True)])
def test_lazy_rows_equal_the_dense_update_bit_for_bit_under_decay(rows, width, staleness, change):
    """weight_decay = 0.01 -- change: 0.05 from step 9, off (None) for steps 15..17, 0.01 again after"""
    _lazy_against_dense(rows, width, staleness, WD, {9: 0.05, 15: None, 18: WD} if change else {})


@pytest.mark.parametrize('rows,width,staleness', [(5000, 256, 7), (300, 64, 256)])
def test_decay_switched_on_in_mid_run(rows, width, staleness):
    """an optimizer built without weight decay, 0.01 from step 10: the plain kernel left the never-touched rows at stamp 0; the
    switch brings every row up to date and stamps it, then the run is as any decayed one"""
    _lazy_against_dense(rows, width, staleness, None, {10: WD})


# ---- 2., 3. exclusions, zero decay, None ----------------------------------------------------------------------------------------
def _mixed_run(steps=12, clip=None, count=None, **kw):
    """two dense vectors, two lazy tables and a ragged tail in one arena, fixed gradients -> {name: final values}, m, v"""
    from bert4clickpath_amd import optim
    g = torch.Generator().manual_seed(11)
    shapes = dict(a=(1000,), b=(130,), t1=(400, 16), t2=(300, 8), c=(77,), tail=(37,))
    P = {k: torch.nn.Parameter((torch.randn(*s, generator=g) * 0.5).cuda()) for k, s in shapes.items()}
    excl = [P[k] for k in kw.pop('exclude', ())]
    opt = optim.Adam(list(P.values()), lazy_rows=[P['t1'], P['t2']], max_staleness=5, global_clipnorm=clip,
                     exclude_from_weight_decay=excl, **kw)
    with _adamw_calls() as calls:
        rng = np.random.default_rng(5)
        for step in range(1, steps + 1):
            opt.zero_grad()
            for k in ('t1', 't2'):
                rows = shapes[k][0]
                ids = np.unique(rng.integers(0, rows // 2, 20))                       # the upper half is never touched
                grad = torch.from_numpy(rng.standard_normal((ids.size, shapes[k][1])).astype(np.float32)).cuda()
                ids = torch.from_numpy(ids).cuda()
                P[k]._b4c_lazy.catch_up(ids)
                P[k].grad[ids] = grad
            for k in ('a', 'b', 'c', 'tail'):
                P[k].grad.copy_(torch.from_numpy(rng.standard_normal(shapes[k]).astype(np.float32)).cuda())
            opt.step(0.5 if step % 3 == 0 else 1.0)
        sd = opt.state_dict()
        torch.cuda.synchronize()
    if count is not None:
        count.update(calls)
    return {k: p.detach().clone() for k, p in P.items()}, sd['m'].clone(), sd['v'].clone(), opt


@pytest.mark.parametrize('clip', [None, 2.0])
def test_excluded_parameters_take_exactly_the_update_without_decay(clip):
    """b, c (dense, between decayed neighbours in the same launch) and the whole lazy table t2 are excluded: bit-identical to
    the run with weight_decay=None (the gradients are fixed, so nothing else feeds back); a, t1 and the tail differ."""
    base, m0, v0, o0 = _mixed_run(clip=clip)
    n = {}
    dec, m1, v1, o1 = _mixed_run(clip=clip, weight_decay=WD, exclude=('b', 't2', 'c'), count=n)
    assert len(o1.dense_ranges) >= 1 and n['b4c_adamw_step'] == n['step'] == 12 * len(o1.dense_ranges)
    assert n['rows'] >= n['b4c_adamw_rows'] > 0           # (a call that names no row launches nothing)
    for k in ('b', 't2', 'c'):
        assert torch.equal(base[k], dec[k]), k
    for k in ('a', 't1', 'tail'):
        assert not torch.equal(base[k], dec[k]), k
        assert bool((base[k] != dec[k]).float().mean() > 0.9), k
    # the moments do not see the decay at all (fixed gradients)
    assert torch.equal(m0, m1) and torch.equal(v0, v1)
    # padding elements of the arena stay zero
    a = o1.arena
    for p, off in zip(a.params, a.offsets):
        end = (off + p.numel() + 63) // 64 * 64
        assert float(a.flat[off + p.numel():end].abs().sum()) == 0.0


@pytest.mark.parametrize('clip', [None, 2.0])
def test_zero_weight_decay_changes_no_bit_and_none_launches_nothing_new(clip):
    n_none, n_zero = {}, {}
    base, m0, v0, o0 = _mixed_run(clip=clip, count=n_none)
    zero, m1, v1, o1 = _mixed_run(clip=clip, weight_decay=0.0, count=n_zero)
    assert n_none == {'step': 0, 'rows': 0, 'b4c_adamw_step': 0, 'b4c_adamw_rows': 0}, n_none
    assert o0._wd_dev is None and o0._decay_blocks_dev is None           # no extra buffer either
    assert n_zero['b4c_adamw_step'] == n_zero['step'] > 0 and n_zero['rows'] >= n_zero['b4c_adamw_rows'] > 0, n_zero
    for k in base:
        assert torch.equal(base[k], zero[k]), k
    assert torch.equal(m0, m1) and torch.equal(v0, v1)
    assert torch.equal(o0.arena.flat, o1.arena.flat)


# ---- 4. against float64 -----------------------------------------------------------------------------------------------------
def _history(rows, width, T, staleness, clip=None, lr_change=None, wd=WD):
    """test_gpu_clipnorm._history with weight decay: the dense and the row-lazy optimizer on the same gradients, float64 AdamW
    beside them"""
    from bert4clickpath_amd import optim
    from oracle import numpy_ref as nr
    on = _grad_schedule(rows, T, staleness, seed=rows)
    scale = _magnitudes(rows)
    rng = np.random.default_rng(width)
    grads = [None] + [(rng.standard_normal((rows, width)) * scale[:, None] * on[t][:, None]).astype(np.float32) for t in range(1, T + 1)]
    norms = np.array([0.0] + [math.sqrt(float(np.sum((grads[t].astype(np.float64) * _mul(t)) ** 2))) for t in range(1, T + 1)])
    if clip == 'median':
        clip = float(np.float32(np.median(norms[1:])))
        clipped = norms[1:] > clip
        assert clipped.sum() >= T / 3 and (~clipped).sum() >= T / 3, (int(clipped.sum()), T)
        assert (np.abs(norms[1:] - clip) > 1e-6 * clip).all(), 'a step ties with the clip: fp32 and float64 may branch differently'
    g0 = torch.Generator().manual_seed(rows + width)
    p0 = torch.randn(rows, width, generator=g0) * 0.05
    dense_p, lazy_p = torch.nn.Parameter(p0.clone().cuda()), torch.nn.Parameter(p0.clone().cuda())
    od = optim.Adam([dense_p], global_clipnorm=clip, weight_decay=wd)
    ol = optim.Adam([lazy_p], lazy_rows=[lazy_p], max_staleness=staleness, global_clipnorm=clip, weight_decay=wd)
    lz = lazy_p._b4c_lazy
    P, M, V = p0.double().numpy(), np.zeros((rows, width)), np.zeros((rows, width))
    lr, lr_sum = 1e-3, 0.0
    for t in range(1, T + 1):
        if lr_change is not None and t == lr_change[0]:
            od.lr = ol.lr = lr = lr_change[1]
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
        g64 = g.astype(np.float64) * mul
        if clip is not None and norms[t] > clip:
            g64 = g64 * (clip / norms[t])
        P = P - (lr * wd) * P                              # decoupled decay first: not through the gradient, the clip or mul
        P, M, V = nr.adam_step(P, g64, M, V, t, lr=lr, beta1=B1, beta2=B2, eps=EPS)
        lr_sum += _lr_t(lr, t)
        assert float(lazy_p.grad.abs().max()) == 0.0, t
    ol.sync_rows()
    torch.cuda.synchronize()
    return dict(pd=dense_p.detach().cpu().numpy(), pl=lazy_p.detach().cpu().numpy(), od=od, ol=ol, P=P, lr_sum=lr_sum, on=on,
                p0=p0.numpy())


@pytest.mark.parametrize('clip', [None, 'median'])
@pytest.mark.parametrize('rows,width', [(1003, 4), (517, 8), (301, 128), (97, 256)])
def test_adamw_kernels_match_float64_over_long_histories(rows, width, clip):
    """300 steps of test_gpu_lazy_training's histories (_grad_schedule, _magnitudes: gaps around max_staleness = 16, an lr
    change at 150, grad_mul in {0.5, 1, 3}, gradients 1e-20 .. 1e15, rows that never receive one), weight_decay 0.01, the dense
    and the row-lazy kernel, unclipped and clipped at the median float64 norm.

    Bound:  |p - p64| <= 256 * sum_s lr_s * 2^-23 + 2 T ulp(p).  The first term is the project's _tolerance unchanged.  The second
    doubles its T ulp(p): the decay adds one more rounded subtraction from p per step, at most half an ulp like the Adam
    subtraction beside it; the rounding of d * p is below 2^-24 d |p| (d ~ 1e-5), that of d itself the same size, and
    (1 - d) < 1 contracts the error already there.
    Worst error / bound observed on an MI355X, dense = lazy and clipped = unclipped in every case: 0.135 (1003x4), 0.157 (517x8),
    0.157 (301x128), 0.164 (97x256).  The worst element is in a never-touched row each time (hence the clip does not show): its
    decrement d * p is nearly the same number every step, so the rounding of the subtraction repeats instead of averaging out
    and the error grows linearly, ~0.3 ulp(p) per step -- inside the half ulp per step the bound allows."""
    T = 300
    h = _history(rows, width, T, 16, clip=clip, lr_change=(150, 3.17e-4))
    pd, pl = h['pd'], h['pl']
    assert np.array_equal(pd, pl), 'lazy != dense in %d elements' % int((pd != pl).sum())
    assert torch.equal(h['od'].m, h['ol'].m) and torch.equal(h['od'].v, h['ol'].v)
    assert np.isfinite(pd).all()
    never = ~h['on'].any(axis=0)
    assert never.sum() >= rows // 8 and (pd[never] != h['p0'][never]).any(axis=1).all(), 'a row without a gradient did not decay'
    worst = 0.0
    for what, p in (('dense', pd), ('lazy', pl)):
        err = np.abs(p.astype(np.float64) - h['P'])
        mag = np.maximum(np.abs(h['P']), np.abs(p.astype(np.float64))).astype(np.float32)
        tol = _tolerance(h['P'], p, h['lr_sum'], T) + T * np.spacing(mag).astype(np.float64)      # ... + 2 T ulp(p) in all
        ratio = float((err / tol).max())
        ratio_never = float((err[never] / tol[never]).max())
        print('adamw %s %s %dx%d: worst |p - p64| / bound = %.4f (never-touched rows %.4f; worst error %.3g)'
              % (what, 'clipped' if clip else 'unclipped', rows, width, ratio, ratio_never, float(err.max())))
        worst = max(worst, ratio)
    assert worst <= 1.0, 'fp32 AdamW off float64: worst error / bound = %g' % worst


# ---- 5. through the model ----------------------------------------------------------------------------------------------------
def _train(dtype, lazy, steps=10, tmp=None, sync_debug=False, wd=WD):
    """test_gpu_clipnorm._train with the paper's recipe: clip 5, WarmupLinearDecay, weight_decay 0.01 but for no_decay_params"""
    from bert4clickpath_amd import checkpoint, ops, optim
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    from clickstream_transformer.training_utils import WarmupLinearDecay

    def make(seed):
        model = _model(dtype, seed=seed)
        opt = _optimizer(model, lazy, global_clipnorm=5.0, learning_rate=WarmupLinearDecay(2e-3, 3, 40), weight_decay=wd,
                         exclude_from_weight_decay=optim.no_decay_params(model) if wd is not None else ())
        return model, opt
    model, opt = make(5)
    T.set_dropout_seed(777)
    data = _batches(steps + 1)
    losses, norms = [], []
    for i in range(steps):
        if tmp is not None and i == steps // 2:
            path = checkpoint.save_checkpoint(os.path.join(tmp, 'ckpt-adamw'), model, opt, epoch=i)
            assert torch.load(path, weights_only=True)['optimizer']['weight_decay'] == wd
            model, opt = make(99)                          # the recipe is the caller's to construct again
            T.set_dropout_seed(5)
            checkpoint.load_checkpoint(path, model, opt)
            assert opt.iterations == i and opt.weight_decay == wd
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
        if sync_debug and i >= 1:
            ops.flush_pending_dw(opt.arena.ctx)
            ops.join_side_work(opt.arena.ctx)
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
    return losses, norms, None, opt.arena.flat.clone(), opt.m.clone(), opt.v.clone()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_the_papers_recipe_through_the_model(dtype):
    """10 steps (bench order, forward -> zero_grad -> backward -> step, two accumulated micro-batches): the row-lazy run equals
    the dense run in losses, logged norms, parameters and both moments; the decay changed the outcome"""
    d = _train(dtype, False)
    l = _train(dtype, True)
    _assert_same_run(d, l)
    assert np.isfinite(d[0]).all() and bool(torch.isfinite(d[3]).all())
    plain = _train(dtype, False, wd=None)
    assert not torch.equal(plain[3], d[3])


@pytest.mark.parametrize('dtype,lazy', [(torch.bfloat16, True), (torch.float32, False)])
def test_decayed_checkpoint_round_trip(tmp_path, dtype, lazy):
    """save in the middle of the run; load into a fresh model and an optimizer built with the same recipe; continue: equal to
    the run never interrupted, bit for bit"""
    a = _train(dtype, lazy, steps=6)
    b = _train(dtype, lazy, steps=6, tmp=str(tmp_path))
    _assert_same_run(a, b)


def test_decayed_step_makes_no_host_sync():
    """steps 2.. under torch.cuda.set_sync_debug_mode('error'), dense and lazy (the first step allocates the histories and
    copies the block flags to the device, once)"""
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
        _train(torch.bfloat16, lazy, steps=4, sync_debug=True)


# ---- 6. two ranks --------------------------------------------------------------------------------------------------------------
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
    opt = optim.Adam(model.parameters(), lazy_rows=[table], max_staleness=4, global_clipnorm=0.05, weight_decay=WD,
                     exclude_from_weight_decay=optim.no_decay_params(model))
    with _adamw_calls() as calls:
        head_end = max(opt.arena.slice_of(p)[1] for n, p in model.named_parameters() if n.startswith('head.'))
        red = parallel.GradReducer(opt.arena, bucket_bounds=[head_end], reduce='mean', sparse_params=[table], sparse_max_fill=fill)
        items, labels, flat = _batch(rank)
        table0 = table.detach().clone()
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
    assert calls['rows'] >= calls['b4c_adamw_rows'] > 0, 'the decayed table never reached b4c_adamw_rows: %r' % calls
    moved = (table.detach() != table0).any(dim=1) | (table0 == 0).all(dim=1)        # (an all-zero row has nothing to decay)
    assert bool(moved.all()), 'rows of the decayed table that did not move: %d' % int((~moved).sum())
    np.save(os.path.join(out_dir, 'rank%d.npy' % rank), opt.arena.flat.cpu().numpy())
    with open(os.path.join(out_dir, 'kind%d.txt' % rank), 'w') as f:
        f.write(','.join(kinds))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize('fill,kind', [(8.0, 'sparse'), (1e-6, 'dense')])
def test_two_ranks_decay_identically(tmp_path, fill, kind):
    """2 ranks, 3 steps, clipping and weight decay on, the item table row-lazy under the row-sparse exchange and under its dense
    fallback: replicas bit-identical, and every non-zero row of the table moved (the decay reached the rows no rank touched)"""
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
    assert np.isfinite(w0).all()
