"""Adam with Keras semantics (reference examples/BERT4Rec/source/main.py:87:
Adam(1e-3, beta_1=.9, beta_2=.999, epsilon=1e-9), constant lr) over one flat fp32 arena.  Beyond the reference's
hard-coded recipe: `learning_rate` may be a schedule (a callable step -> lr, Keras' LearningRateSchedule convention;
clickstream_transformer.training_utils has the reference's two) and `global_clipnorm` clips the gradient by its global L2
norm, computed and applied on the device (csrc/gradnorm.hip); `weight_decay` is Keras AdamW's decoupled decay.

All parameters are re-homed into a single contiguous buffer (64-element aligned slices), gradients
into a second one: the optimizer step is ONE HIP kernel launch over the arena and the data-parallel
all-reduce works on contiguous buckets of the gradient arena (parallel.py)."""
import math
import struct

import torch

from . import ops


class FlatArena:
    ALIGN = 64

    def __init__(self, params, order=None):
        params = [p for p in params if p.requires_grad]
        if order is not None:
            params = sorted(params, key=order)
        self.params = params
        dev = params[0].device
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.numel = n
        self.offsets = offs
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        # host state of this arena's training step (grad-ready callback of a reducer, side-stream work of the backward pass
        # in flight): per arena, not per process -- ops.ArenaContext
        self.ctx = ops.ArenaContext()
        with torch.no_grad():
            for p, o in zip(params, offs):
                if p.dtype != torch.float32:
                    raise ValueError('master parameters must be float32')
                view = self.flat[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = self.grad[o:o + p.numel()].view(p.shape)
                # the weight-gradient kernels may now add straight into this view (ops.arena_context finds the arena's
                # context through the parameter; a parameter outside any arena gets its gradient through autograd as usual)
                p._b4c_ctx = self.ctx

    def slice_of(self, p):
        i = next(k for k, q in enumerate(self.params) if q is p)
        return self.offsets[i], self.offsets[i] + p.numel()

    def zero_grad(self):
        self.ctx.reset()          # side-stream work a failed step left behind must not add into this step's gradients
        ops.zero_(self.grad)


def _f32(x):
    """the double x rounded to fp32 (to nearest), as a Python float: what a kernel argument and a device table both hold"""
    return struct.unpack('f', struct.pack('f', x))[0]


def no_decay_params(module):
    """the BERT convention for Adam(exclude_from_weight_decay=...): every parameter with dim() < 2 -- LayerNorm gamma / beta and
    every bias, the vocabulary head's among them.  Embedding tables and weight matrices decay."""
    return [p for p in module.parameters() if p.dim() < 2]


class StepHistory:
    """One fp32 value per optimizer step (index = step, entry 0 unused) as the row kernels replay it: a host list in double and
    a device table.  Entries of past steps never change; the table keeps its capacity: a step writes its own entry only (no
    host sync); it is reallocated, twice as large, when it is full, and rewritten when entries change (record / rebuild)."""

    def __init__(self, value_of):
        self.value_of = value_of      # step -> the value under the optimizer's PRESENT settings (look-ahead, rebuild)
        self.host, self.dev, self.valid = [0.0], None, 0

    def record(self, t, value):
        """step t is being taken with `value` (what the dense kernel is handed now)"""
        if len(self.host) == t:
            self.host.append(value)
        else:                               # (pre-computed with settings that have changed since)
            self.host[t:] = [value]
            self.valid = min(self.valid, t)

    def rebuild(self, t):
        self.host = [0.0] + [self.value_of(s) for s in range(1, t + 1)]
        self.valid = 0

    def table(self, t, device):
        """the device table, valid for steps 1 .. t"""
        while len(self.host) <= t:
            self.host.append(self.value_of(len(self.host)))
        n = len(self.host)
        if self.dev is None or self.dev.numel() < n:
            cap = max(1024, 2 * n)
            self.dev = ops.zeros(cap, dtype=torch.float32, device=device)
            self.valid = 0
        if self.valid < n:
            lo = self.valid
            if n - lo == 1:       # one entry per step: a fill (the value rounded to fp32 as below), stream-ordered behind the readers
                self.dev[lo:n].fill_(self.host[lo])
            else:
                self.dev[lo:n].copy_(torch.tensor(self.host[lo:n], dtype=torch.float64).to(torch.float32))
            self.valid = n
        return self.dev


class LazyRows:
    """Row-lazy Adam state of ONE row-sparse table of the arena (config 5's 2M-row tables; include/b4c.h b4c_adam_rows).
    `stamp[row]` = the last optimizer step the row is current through (0: never touched, all moments zero).  Whoever is
    about to READ rows of the table brings them up to date first -- `catch_up(ids)`, called by the gather sites of the forward
    pass (ops.EmbedFn, ops.SampledCEFn) -- and those are exactly the rows that can receive a gradient in this step, so the
    optimizer's step on this table runs over the ids seen since the last step and nothing else.  The table's gradient is all
    zeros between steps (the step kernel zeroes the rows it consumed), so zero_grad leaves the table alone."""

    def __init__(self, opt, p, lo):
        self.opt, self.p, self.lo = opt, p, lo
        self.rows, self.width = int(p.shape[0]), int(p.shape[1])
        if p.dim() != 2 or self.width % 4:
            raise ValueError('row-lazy Adam needs 2-D (rows, width) tables with width % 4 == 0')
        self.stamp = ops.zeros(self.rows, dtype=torch.int32, device=p.device)
        self.touched = []          # id tensors (int64, contiguous) read / named since the last step
        self.all_rows = False      # the whole table takes the next step (dense fallback of a data-parallel exchange)
        self.cursor = 0            # next row of the rotating catch-up
        self.decay = True          # the table takes weight decay, as a whole (Adam(exclude_from_weight_decay=...) clears it)

    def _slices(self):
        o, n = self.opt, self.rows * self.width
        a = o.arena
        return a.flat[self.lo:self.lo + n], a.grad[self.lo:self.lo + n], o.m[self.lo:self.lo + n], o.v[self.lo:self.lo + n]

    def _launch(self, ids, n, row_lo, t, mode, grad_mul=1.0, coef=None):
        o = self.opt
        p, g, m, v = self._slices()
        # coef, the clip coefficient, scales the gradient of step t alone: the zero-gradient steps a row replays (here and in
        # catch_up / sync) are g = 0 whatever was clipped at the time, so no past coefficient is ever needed.
        # decay_hist (AdamW): every replayed step decays with its own factor.  Also when weight_decay is None by now: the rows
        # still owe the decayed steps they missed (a step taken without decay has the factor 0.0: p - 0 p = p)
        ops.adam_rows_(p, g, m, v, self.stamp, ids, n, row_lo, self.rows, self.width, o.lr_hist(t), t, o.beta_1, o.beta_2, o.epsilon,
                       grad_mul, mode, coef, o.decay_hist(t) if self.decay and o._decay_seen else None)

    @staticmethod
    def _ids(ids):
        ids = ids.reshape(-1)
        if ids.dtype != torch.int64 or not ids.is_contiguous():
            ids = ids.to(torch.int64).contiguous()
        return ids

    def catch_up(self, ids, note=True):
        """rows `ids` (any integer tensor on the device; repeats and out-of-range values as the gather kernels take them) are
        brought to the optimizer's current step and -- note=True: the read is part of a pass that will be differentiated --
        remembered as this step's candidates for a gradient"""
        ids = self._ids(ids)
        if ids.numel() == 0:
            return
        if self.opt.iterations > 0:
            self._launch(ids, ids.numel(), 0, self.opt.iterations, 0)
        if note:
            self.touched.append(ids)

    def note(self, ids):
        """rows that receive a gradient in this step without having been read by this process (another rank's rows)"""
        ids = self._ids(ids)
        if ids.numel():
            self.touched.append(ids)

    def sync(self):
        """every row current (before the table is read as a whole: state_dict, checkpoint, full-vocabulary scoring)"""
        if self.opt.iterations > 0:
            self._launch(None, self.rows, 0, self.opt.iterations, 0)

    def grad_sumsq(self, partial):
        """this step's gradient rows into the chunk partials of the global norm (before step() consumes `touched`): the rows
        named since the last step are the only ones that can hold a gradient; the other chunks stay at the caller's 0.0"""
        g = self.opt.arena.grad
        if self.all_rows:
            ops.grad_sumsq_(g, self.lo, self.lo + self.rows * self.width, partial)
        else:
            for ids in self.touched:
                ops.grad_sumsq_rows_(g, self.lo, self.rows, self.width, ids, partial)

    def step(self, t, grad_mul, coef=None):
        if self.all_rows:
            self._launch(None, self.rows, 0, t, 1, grad_mul, coef)
        else:
            for ids in self.touched:
                self._launch(ids, ids.numel(), 0, t, 1, grad_mul, coef)
            # bounded staleness: a rotating slice of the table is caught up every step, so no row ever replays more than
            # `max_staleness` steps at once (a rare item's first re-occurrence after 50,000 steps would otherwise be 50,000
            # dependent iterations in one wave)
            per = -(-self.rows // max(self.opt.max_staleness, 1))
            lo = self.cursor
            n = min(per, self.rows - lo)
            self._launch(None, n, lo, t, 0)
            self.cursor = 0 if lo + n >= self.rows else lo + n
        self.touched, self.all_rows = [], False


class Adam:
    def __init__(self, params, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-9, arena=None, order=None, lazy_rows=(),
                 max_staleness=256, global_clipnorm=None, weight_decay=None, exclude_from_weight_decay=()):
        """learning_rate: a float, or a callable `step -> lr` called with the number of steps already taken (0 at the first
        step), as Keras calls a LearningRateSchedule.  `opt.lr` reads the current value; assigning to it (ReduceLROnPlateau)
        raises TypeError on a scheduled optimizer, as Keras does.  state_dict() / checkpoint.save_checkpoint store
        `iterations` and the current float: the schedule object is the caller's to construct again before loading.

        global_clipnorm (Keras' name; None: off, today's launches exactly): the gradient -- `grad_mul * g`, i.e. the mean
        gradient under a reducer with reduce='mean' -- is scaled by min(1, global_clipnorm / ||grad_mul * g||) over the whole
        arena.  A plain attribute: it may be switched between steps.  The norm never leaves the device; `last_grad_norm` is the
        0-d device tensor the last clipped step wrote (reading it is the caller's sync, and the next step overwrites it).
        Results are bit-identical between the row-lazy and the dense optimizer and between data-parallel replicas
        (csrc/gradnorm.hip: the reduction is defined by arena position) as long as the norm is finite; a non-finite norm makes
        the coefficient NaN and with it every parameter that takes the step.

        weight_decay (Keras AdamW; None: off, today's launches exactly -- no extra buffer, no other entry point): a float >= 0.
        A decayed parameter takes  p <- p - (lr * weight_decay) * p  first, with the plain learning rate of the step (the
        schedule's value or the float, not the bias-corrected lr_t), and then the Adam update unchanged.  The decay does not go
        through the gradient: grad_mul and the clip leave it alone and it does not enter the global norm.  A plain attribute:
        it may be changed between steps, and each step is recorded with the factor it was taken with.  Parameters in
        `exclude_from_weight_decay` (optim.no_decay_params(model) is the BERT convention) take exactly the update they take
        without decay; a row-lazy table decays, or not, as a whole.  A never-touched row of a decayed table moves every step,
        so the rotating catch-up and sync_rows() visit every row (max_staleness bounds the replay as before) and lazy == dense
        still holds bit for bit.  Switching the decay on in mid-run first brings every row of the decayed tables up to date
        and stamps it (launches, no host sync), so no row ever replays more than max_staleness steps.  state_dict() / checkpoint.save_checkpoint store `weight_decay` FOR THE RECORD ONLY: loading
        does not restore it (the exclusion set cannot be stored, and half a recipe would mislead) -- the constructor's
        arguments govern, as with a schedule.

        lazy_rows: 2-D (rows, width) parameters whose gradient is row-sparse (embedding tables, a vocabulary-major sampled
        projection): their share of the update runs over the rows in use only, with results bit-identical to the dense
        update (LazyRows).  Code that reads such a table as a whole calls `sync_rows()` first; `state_dict()` and
        checkpoint.save_checkpoint do."""
        self._learning_rate = learning_rate if callable(learning_rate) else float(learning_rate)
        self.global_clipnorm = global_clipnorm
        self.lazy, self.iterations = [], 0
        self._decay_seen = False                 # some step since reset_rows() may have decayed (set with weight_decay)
        self.weight_decay = weight_decay
        self.last_grad_norm = None
        self._clip_bufs = None
        self.arena = arena or FlatArena(list(params), order)
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon
        self.m = torch.zeros_like(self.arena.flat)
        self.v = torch.zeros_like(self.arena.flat)
        self.max_staleness = int(max_staleness)
        self._lr = StepHistory(self._lr_t)       # lr_t of every step so far
        self._wd = StepHistory(self._decay_t)    # the decay factor of every step so far, beside it
        self._decay_blocks_dev = None
        exclude = list(exclude_from_weight_decay)
        for q in exclude:
            if not any(q is p for p in self.arena.params):
                raise ValueError('exclude_from_weight_decay names a parameter that is not in the optimizer\'s arena')
        self._no_decay = {id(q) for q in exclude}
        self._grads_clean = False      # the lazy tables' gradient rows are all zero (left so by the last completed step)
        for p in lazy_rows:
            lo, _ = self.arena.slice_of(p)
            lz = LazyRows(self, p, lo)
            lz.decay = id(p) not in self._no_decay
            p._b4c_lazy = lz
            self.lazy.append(lz)
        # the dense share of the arena: what is left between the lazy tables
        cuts, pos = [], 0
        for lz in sorted(self.lazy, key=lambda z: z.lo):
            if lz.lo > pos:
                cuts.append((pos, lz.lo))
            pos = lz.lo + (lz.rows * lz.width + FlatArena.ALIGN - 1) // FlatArena.ALIGN * FlatArena.ALIGN
        if pos < self.arena.numel:
            cuts.append((pos, self.arena.numel))
        self.dense_ranges = cuts

    @property
    def global_clipnorm(self):
        return self._global_clipnorm

    @global_clipnorm.setter
    def global_clipnorm(self, value):
        if value is not None:
            value = float(value)
            if not value > 0.0:
                raise ValueError('global_clipnorm must be a positive number or None, got %r' % (value,))
        self._global_clipnorm = value

    @property
    def weight_decay(self):
        return self._weight_decay

    @weight_decay.setter
    def weight_decay(self, value):
        if value is not None:
            value = float(value)
            if not (value >= 0.0 and math.isfinite(value)):
                raise ValueError('weight_decay must be a finite number >= 0 or None, got %r' % (value,))
            if not self._decay_seen:
                self._start_decay()
        self._weight_decay = value

    def _start_decay(self):
        """the decay is switched on: from here the decayed tables take the AdamW row kernel.  In mid-run the plain kernel has
        left every never-touched row at stamp 0, and the AdamW kernel would replay the whole run so far for each of them on
        its first visit, which is what max_staleness exists to prevent.  So every row is brought up to date with the plain
        kernel (no step so far decayed) and stamped current -- launches only, and the notes of a forward pass already made
        (LazyRows.touched) stay."""
        if self.iterations > 0 and self.arena.flat.is_cuda:
            for lz in self.lazy:
                if lz.decay:
                    lz.sync()
                    lz.stamp.fill_(self.iterations)
        self._decay_seen = True

    # (the histories' parts under the names they had as plain attributes)
    _lr_host = property(lambda self: self._lr.host)
    _lr_dev = property(lambda self: self._lr.dev)
    _wd_host = property(lambda self: self._wd.host)
    _wd_dev = property(lambda self: self._wd.dev)

    def decay_blocks_host(self):
        """uint8 [arena.numel / 64]: 1 for every 64-element block of a parameter that decays.  Every arena slice starts at a
        multiple of FlatArena.ALIGN = 64 and is padded to one, so no block belongs to two parameters; a parameter's padding
        shares its last block (zeros stay zeros under the decay as under Adam)."""
        A = FlatArena.ALIGN
        a = self.arena
        blocks = torch.zeros(a.numel // A, dtype=torch.uint8)
        for p, o in zip(a.params, a.offsets):
            if id(p) not in self._no_decay:
                blocks[o // A:(o + p.numel() + A - 1) // A] = 1
        return blocks

    def _decay_blocks(self):
        if self._decay_blocks_dev is None:       # built once (the one host-to-device copy of the decay, at its first step)
            self._decay_blocks_dev = self.decay_blocks_host().to(self.arena.flat.device)
        return self._decay_blocks_dev

    @property
    def scheduled(self):
        return callable(self._learning_rate)

    @property
    def lr(self):
        """the learning rate of the next step (a schedule is evaluated at `iterations`, the number of steps taken)"""
        return float(self._learning_rate(self.iterations)) if self.scheduled else self._learning_rate

    @lr.setter
    def lr(self, value):
        if self.scheduled:
            raise TypeError('this optimizer was created with a learning-rate schedule (%r): its learning rate cannot be set; '
                            'only a float learning_rate is settable' % (self._learning_rate,))
        self._learning_rate = float(value)

    learning_rate = lr

    def _lr_t(self, t):
        """bias-corrected step size of step t (t = 1 is the first): a schedule sees t - 1, the steps taken before it"""
        lr = float(self._learning_rate(t - 1)) if self.scheduled else self._learning_rate
        return lr * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)

    def _decay_t(self, t):
        """decay factor of step t: fp32(lr(t - 1) * weight_decay), the product in double, rounded once -- the dense kernel's
        scalar and the row kernel's table entry are this same fp32 value.  0.0 while weight_decay is None."""
        if self._weight_decay is None:
            return 0.0
        lr = float(self._learning_rate(t - 1)) if self.scheduled else self._learning_rate
        return _f32(lr * self._weight_decay)

    def lr_hist(self, t):
        """device fp32 table of the lr_t of steps 1 .. t (what the dense kernel was / is handed at each of them): the replay of
        a missed step needs that step's own value.  Entries of past steps never change; a change of `self.lr` (ReduceLROnPlateau)
        shows from the step it first applies to.  The table keeps its capacity: a step writes its own entry only (no host sync);
        it is reallocated, twice as large, when it is full, and rewritten in place when past entries change (reset_rows)."""
        return self._lr.table(t, self.arena.flat.device)

    def decay_hist(self, t):
        """device fp32 table of the decay factors of steps 1 .. t beside lr_hist: same capacity rule, one entry per step, no
        host sync; a change of weight_decay or of lr shows from the step it first applies to"""
        return self._wd.table(t, self.arena.flat.device)

    def zero_grad(self):
        if self.lazy and self._grads_clean:
            self.arena.ctx.reset()
            for lo, hi in self.dense_ranges:
                ops.zero_(self.arena.grad[lo:hi])
        else:
            self.arena.zero_grad()
        # the lazy tables' row notes (touched / all_rows) stay: the forward pass may have run already
        # (`loss = model(x); opt.zero_grad(); loss.backward(); opt.step()`), and its notes name the rows that will receive a
        # gradient.  step() consumes them; a note left by a step that never ran is harmless (a row stepped with a zero
        # gradient takes exactly the dense update)
        self._grads_clean = False

    def sync_rows(self):
        for lz in self.lazy:
            lz.sync()

    def step(self, grad_mul=1.0):
        """p -= lr_t * m / (sqrt(v) + eps), lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t)  (Keras Adam, dense update)."""
        a = self.arena
        if not a.flat.is_cuda:
            raise ops.B4CError('Adam.step runs on the HIP device only')
        ops.flush_pending_dw(a.ctx)
        ops.join_side_work(a.ctx)
        t, lr_t, decay = self._begin_step()
        coef = self._clip_coef(grad_mul) if self._global_clipnorm is not None else None
        if not self.lazy:
            self._adam_range(0, a.numel, lr_t, grad_mul, coef, decay)
        else:
            for lo, hi in self.dense_ranges:
                self._adam_range(lo, hi, lr_t, grad_mul, coef, decay)
            for lz in self.lazy:
                lz.step(t, grad_mul, coef)
            self._grads_clean = True
        ops.bump_weights_epoch()

    def _begin_step(self):
        """the host side of a step: -> (t, lr_t, decay factor or None), all three as the dense kernel is handed them; with
        row-lazy tables step t also enters the histories their kernels replay from"""
        self.iterations += 1
        t = self.iterations
        lr_t = self._lr_t(t)
        decay = self._decay_t(t) if self._weight_decay is not None else None
        if self.lazy:
            self._lr.record(t, lr_t)
            self._wd.record(t, decay or 0.0)
        return t, lr_t, decay

    def _adam_range(self, lo, hi, lr_t, grad_mul, coef, decay=None):
        a = self.arena
        A = FlatArena.ALIGN      # (dense ranges start at slice boundaries: multiples of 64)
        blocks = self._decay_blocks()[lo // A:(hi + A - 1) // A] if decay is not None else None
        ops.adam_step_(a.flat[lo:hi], a.grad[lo:hi], self.m[lo:hi], self.v[lo:hi], lr_t, self.beta_1, self.beta_2, self.epsilon,
                       grad_mul, coef, decay, blocks)

    def _clip_coef(self, grad_mul):
        """the device's clip coefficient of this step (fp32 [1]); also sets last_grad_norm.  Launches only: no host sync.
        Chunk partials over the dense share (or the whole arena), the rows in use of each lazy table, then the fixed tree."""
        a = self.arena
        if self._clip_bufs is None:
            n_chunks = ops.grad_chunks(a.numel)
            dev = a.flat.device
            self._clip_bufs = (ops.zeros(n_chunks, dtype=torch.float64, device=dev),
                               ops.zeros((n_chunks + ops.L.GRAD_GROUP - 1) // ops.L.GRAD_GROUP, dtype=torch.float64, device=dev),
                               ops.zeros(2, dtype=torch.float32, device=dev))
            self.last_grad_norm = self._clip_bufs[2][0]
        partial, groups, norm_coef = self._clip_bufs
        if not self.lazy:
            ops.grad_sumsq_(a.grad, 0, a.numel, partial)
        else:
            ops.zero_(partial)        # (config 5: 4 MB) chunks of the lazy tables that nobody names this step: their gradient is zero
            for lo, hi in self.dense_ranges:
                ops.grad_sumsq_(a.grad, lo, hi, partial)
            for lz in self.lazy:
                lz.grad_sumsq(partial)
        ops.grad_clip_coef_(partial, groups, self._global_clipnorm, grad_mul, None, norm_coef)
        return norm_coef[1:]

    def state_dict(self):
        self.sync_rows()
        # (weight_decay: for the record only -- load_state_dict leaves the constructor's value alone)
        return {'iterations': self.iterations, 'm': self.m, 'v': self.v, 'lr': self.lr, 'weight_decay': self._weight_decay}

    def load_state_dict(self, sd):
        self.iterations = int(sd['iterations'])
        if not self.scheduled:        # (a schedule is a function of `iterations`: the stored float is for the record only)
            self.lr = float(sd['lr'])
        self.m.copy_(sd['m'])
        self.v.copy_(sd['v'])
        self.reset_rows()

    def reset_rows(self):
        """after the moments / parameters were loaded from outside: every row counts as current through `iterations`; the lr_t
        and decay histories of the steps before are rebuilt from the present lr and weight_decay, or by calling the schedule
        for each past step (nothing will replay them)"""
        self._lr.rebuild(self.iterations)
        self._wd.rebuild(self.iterations)
        self._decay_seen = self._weight_decay is not None
        for lz in self.lazy:
            lz.stamp.fill_(self.iterations)
            lz.touched, lz.all_rows, lz.cursor = [], False, 0
        self._grads_clean = False
