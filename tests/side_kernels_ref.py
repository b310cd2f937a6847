"""Restatements, case tables and error bounds for the small row and elementwise kernels of csrc/elemwise.hip, shared by
test_side_kernels_cpu.py (which runs them against what already exists and against deliberately wrong variants) and
test_gpu_side_kernels.py (which runs the kernels).  Everything here is CPU torch / numpy in float64 or integers, written from
the comment above each kernel.

Layout of every function family:  x_case(...) builds the inputs (seeded, on the CPU);  x_emulate(case, wrong=None) is the
buffer a kernel leaves -- the restatement rounded to the output type, written into a sentinel-filled buffer -- or, with
`wrong`, what a kernel with that one geometry mistake would leave;  x_check(case, got) is THE comparison: the GPU test hands it
the kernel's buffers, the CPU test hands it x_emulate's and expects an AssertionError for every wrong variant.

Buffers: an output is SENT-filled and TAIL elements longer than needed; a row output has the pitch width + GAP."""
import math

import numpy as np
import torch

from oracle import numpy_ref as nr

F32, BF16, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64
SENT, TAIL, GAP = -7, 64, 8
U24 = 2.0 ** -24             # half an fp32 ulp, relative: one fp32 rounding
BF_ULP = 2.0 ** -8           # "one bf16 ulp" as a relative bound (8 significant bits: an ulp is 2^-8 .. 2^-7 of the value).  The final
                             # rounding takes up to half an ulp, which just above a power of two is nearly all of 2^-8 |ref|; what is
                             # left there, 2^-16 |ref|, still is a hundred times the error of the fp32 work before the rounding
F32_EPS = float(np.float32(1e-7))                        # KERAS_EPS as the kernels hold it
F32_HI = float(np.float32(1.0) - np.float32(1e-7))       # 1 - 2^-23: what fp32 makes of 1 - 1e-7

EW_THREADS = 2048 * 256      # ew_grid: at most 2048 workgroups of 256 threads; work item EW_THREADS starts the second trip
BCE_THREADS = 512 * 256      # masked_bce / binary_counts: their own cap of 512 workgroups
ROW_CAP = 4096               # row-per-workgroup kernels: rows >= 4096 are a workgroup's second row
ROW_TRIP = 2048              # 256 threads x 8 columns: column 2048 starts a thread's second chunk

WRONG_ELEMWISE = ('second_trip',)
WRONG_ROWS = ('last_chunk', 'from_2048', 'tail_counts', 'rows_4096')


def gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def rup8(x):
    return (x + 7) // 8 * 8


def bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def flat_buffer(n, dtype, fill=SENT):
    return torch.full((n + TAIL,), fill, dtype=dtype)


def row_buffer(rows, ld, dtype, fill=SENT):
    """flat buffer of rows x ld (+ TAIL) and its [rows][ld] view"""
    buf = torch.full((rows * ld + TAIL,), fill, dtype=dtype)
    return buf, buf[:rows * ld].view(rows, ld)


def rows_of(buf, rows, ld):
    return buf[:rows * ld].view(rows, ld)


def pitched(x, ld, fill=SENT):
    """x [rows][width] copied into a SENT-filled buffer of pitch ld (gap columns and the tail hold `fill`)"""
    buf, v = row_buffer(x.shape[0], ld, x.dtype, fill)
    v[:, :x.shape[1]] = x
    return buf


def assert_tail(buf, used, what):
    assert bool((buf[used:] == SENT).all()), '%s: wrote past its %d elements' % (what, used)


def assert_gap(buf, rows, ld, width, what):
    assert bool((rows_of(buf, rows, ld)[:, width:] == SENT).all()), '%s: wrote into the gap columns' % what
    assert_tail(buf, rows * ld, what)


def chain_bound(additions, magnitude):
    """|fp32 sum - exact sum| of one addition chain: every one of `additions` roundings is off by at most 2^-24 of a partial sum,
    and no partial sum exceeds `magnitude`, the sum of the magnitudes of everything added"""
    return additions * U24 * magnitude


# =====================================================================================================================
# 1. one thread = 8 elements: dropout, sigmoid forward / backward, relu gate
# =====================================================================================================================
VEC8_N = (8, 2040, 2048, 2056, 8 * (524288 + 300))
VEC8_TRIP = 8 * EW_THREADS           # first element of the second trip


def elemwise_emulate(ref, wrong=None, trip=VEC8_TRIP):
    """the buffer of a whole-buffer output; wrong = 'second_trip': the elements from `trip` on are never written"""
    assert wrong in (None,) + WRONG_ELEMWISE
    n = ref.numel()
    buf = flat_buffer(n, ref.dtype)
    m = min(n, trip) if wrong == 'second_trip' else n
    buf[:m] = ref.reshape(-1)[:m]
    return buf


def dropout_case(n, dtype, rate, seed):
    from bert4clickpath_amd import ops
    x = torch.randn(n, generator=gen(1, n)).to(dtype)
    keep = torch.from_numpy(ops.keep_mask(seed, n, rate))
    return {'n': n, 'dtype': dtype, 'rate': rate, 'seed': seed, 'x': x, 'keep': keep}


def dropout_ref(c):
    """y[e] = keep(seed, e) ? x[e] / (1 - rate) : 0, the factor computed in fp32 as the kernel computes it"""
    mul = float(np.float32(1.0) / (np.float32(1.0) - np.float32(c['rate'])))
    return torch.where(c['keep'], c['x'].float() * mul, torch.zeros(())).to(c['dtype'])


def exact_check(ref, got, what):
    """bit for bit, and nothing past the end"""
    n = ref.numel()
    assert same_bits(got[:n], ref.reshape(-1)), '%s: %d of %d elements differ' % (what, int((bits(got[:n]) != bits(ref.reshape(-1))).sum()), n)
    assert_tail(got, n, what)


def relu_gate_case(n, dtype):
    g = gen(2, n)
    gr = torch.randn(n, generator=g).to(dtype)
    act = torch.randn(n, generator=g).to(dtype)
    act[0::5] = 0.0
    act[1::7] = -0.0
    act[n - 1] = 0.0 if n > 8 else act[n - 1]
    return {'n': n, 'dtype': dtype, 'g': gr, 'act': act}


def relu_gate_ref(c):
    return torch.where(c['act'] > 0, c['g'], torch.zeros((), dtype=c['dtype']))


SIGMOID_PLANTED = (0.0, -0.0, 20.0, -20.0, 88.0, -88.0)


def sigmoid_fwd_case(n, dtype):
    x = torch.randn(n, generator=gen(3, n)) * 6.0
    k = min(n, len(SIGMOID_PLANTED))
    x[:k] = torch.tensor(SIGMOID_PLANTED[:k])
    if n >= 16:
        x[n - 6:] = torch.tensor(SIGMOID_PLANTED)
    return {'n': n, 'dtype': dtype, 'x': x.to(dtype)}


def sigmoid_fwd_ref(c):
    return 1.0 / (1.0 + torch.exp(-c['x'].double()))


def sigmoid_fwd_bound(ref, dtype):
    """fp32: 1e-6 absolute, the project's bound for these probabilities (expf, one add, one division: a few 2^-24 of a value <= 1).
    bf16: one bf16 ulp of the float64 value."""
    return torch.full_like(ref, 1e-6) if dtype == F32 else BF_ULP * ref.abs()


def sigmoid_bwd_case(n, dtype):
    g = gen(4, n)
    y = torch.sigmoid(torch.randn(n, generator=g) * 6.0)
    y[0], y[min(1, n - 1)], y[min(2, n - 1)] = 0.0, 1.0, 0.5
    if n >= 16:
        y[n - 3:] = torch.tensor([0.0, 1.0, 0.5])
    return {'n': n, 'dtype': dtype, 'y': y.to(dtype), 'dy': torch.randn(n, generator=g).to(dtype)}


def sigmoid_bwd_ref(c):
    y = c['y'].double()
    return c['dy'].double() * y * (1.0 - y)


def sigmoid_bwd_bound(ref, dtype):
    """dy * y * (1 - y) in fp32 is three roundings (1 - y, the two products), each 2^-24 relative: 4 * 2^-24 covers them and their
    cross terms.  bf16: one bf16 ulp (the final rounding is 2^-9, the fp32 work far below it)."""
    return (4 * U24 if dtype == F32 else BF_ULP) * ref.abs()


def bounded_check(ref, bound, got, what):
    """|got - ref| <= bound on every element, nothing past the end; -> the worst err / bound (0 where both are 0)"""
    n = ref.numel()
    out = got[:n].double()
    assert bool(torch.isfinite(out).all()), '%s: non-finite output' % what
    err = (out - ref.reshape(-1)).abs()
    bad = err > bound.reshape(-1)
    assert not bool(bad.any()), '%s: %d of %d elements past the bound, first at %d (err %.3e, bound %.3e)' % (
        what, int(bad.sum()), n, int(bad.nonzero()[0]), float(err[bad][0]), float(bound.reshape(-1)[bad][0]))
    assert_tail(got, n, what)
    nz = bound.reshape(-1) > 0
    return float((err[nz] / bound.reshape(-1)[nz]).max()) if bool(nz.any()) else 0.0


# =====================================================================================================================
# 2. masked binary cross-entropy and the binary counts: one element per thread, 512 workgroups at most, float atomics
# =====================================================================================================================
BCE_N = (1, 255, 256, 257, 131071, 131073, 300001)
BCE_POS_WEIGHT = (0.0, 0.5, 3.0)
BCE_SUMS_START = (5.0, 3.0)


def bce_planted():
    """0, 1, 5e-8, 1 - 5e-8 and the two fp32 clip bounds themselves, as fp32"""
    return torch.tensor([0.0, 1.0, 5e-8, 1.0 - 5e-8, F32_EPS, F32_HI], dtype=torch.float64).float()


def bce_case(n, dtype, all_pad=False):
    g = gen(5, n)
    p = torch.rand(n, generator=g)
    lab = torch.randint(0, 2, (n,), generator=g).float()
    lab[torch.rand(n, generator=g) < 0.3] = -1.0
    pl = bce_planted()
    k = min(n, 12)                                  # the six values under label 1, then under label 0, at the head ...
    p[:k] = pl.repeat(2)[:k]
    lab[:k] = torch.tensor([1.0] * 6 + [0.0] * 6)[:k]
    if n >= 24:                                     # ... and at the very end, which the second trip handles when there is one
        p[n - 12:] = pl.repeat(2)
        lab[n - 12:] = torch.tensor([0.0] * 6 + [1.0] * 6)
    if all_pad:
        lab[:] = -1.0
    return {'n': n, 'dtype': dtype, 'p': p.to(dtype), 'labels': lab}


def bce_outside_clip(c):
    p = c['p'].double()
    return (p < F32_EPS) | (p > F32_HI)


def bce_ref(c, pos_weight, wrong=None):
    """-> item loss, d loss / d p (float64), both 0 at pads.  o = clip(p, eps, 1 - eps); bce = -(t log(o + eps) + (1 - t) log(1 - o + eps));
    weight = pos_weight where t == 1 (if pos_weight > 0) else 1; the derivative is 0 outside the clip range.  eps and 1 - eps are
    the fp32 values.  wrong: 'f64_clip' (1e-7 and 1 - 1e-7 as float64 hold them), 'weight_on_negatives'."""
    p, t = c['p'].double(), c['labels'].double()
    lo, hi, eps = (1e-7, 1.0 - 1e-7, 1e-7) if wrong == 'f64_clip' else (F32_EPS, F32_HI, F32_EPS)
    valid = t != -1.0
    tv = torch.where(valid, t, torch.zeros_like(t))
    o = p.clamp(lo, hi)
    w = torch.ones_like(p)
    if pos_weight > 0:
        w[tv == (0.0 if wrong == 'weight_on_negatives' else 1.0)] = float(np.float32(pos_weight))
    item = -(tv * torch.log(o + eps) + (1.0 - tv) * torch.log(1.0 - o + eps)) * w
    d = -(tv / (o + eps) - (1.0 - tv) / (1.0 - o + eps)) * w
    d = torch.where((p >= lo) & (p <= hi), d, torch.zeros_like(d))
    z = torch.zeros_like(p)
    return torch.where(valid, item, z), torch.where(valid, d, z)


def bce_grid(n):
    return min(-(-n // 256), 512)


def bce_sum_bound(n, item_abs_sum):
    """sums[0]: a thread adds ceil(n / (grid * 256)) items, the workgroup sum is 6 butterfly steps and 4 additions (the "10"), and
    `grid` atomics follow each other in some order: the longest chain of roundings, each 2^-24 of the sum of the items' magnitudes."""
    grid = bce_grid(n)
    return chain_bound(-(-n // (grid * 256)) + 10 + grid, item_abs_sum)


def bce_emulate(c, pos_weight, wrong=None):
    """-> item_loss buffer, dprobs buffer, sums (after one call from BCE_SUMS_START)"""
    n = c['n']
    item, d = bce_ref(c, pos_weight, wrong)
    cnt = (c['labels'] != -1.0).double()
    m = min(n, BCE_THREADS) if wrong == 'second_trip' else n
    s0, s1 = float(item[:m].sum()), float(cnt[:m].sum())
    if wrong != 'overwrite':
        s0, s1 = s0 + BCE_SUMS_START[0], s1 + BCE_SUMS_START[1]
    return (elemwise_emulate(item.float(), 'second_trip' if wrong == 'second_trip' else None, BCE_THREADS),
            elemwise_emulate(d.float(), 'second_trip' if wrong == 'second_trip' else None, BCE_THREADS),
            torch.tensor([s0, s1], dtype=torch.float64).float())


def bce_check(c, pos_weight, item_buf, d_buf, sums, item_for_sum=None):
    """item_buf / d_buf None: the call ran without that output, and sums[0] is compared with `item_for_sum` (the item losses of the
    call that had it).  -> worst err / bound of the per-element comparison"""
    n = c['n']
    item, d = bce_ref(c, pos_weight)
    pad = c['labels'] == -1.0
    worst = 0.0
    for name, ref, buf in (('item_loss', item, item_buf), ('dprobs', d, d_buf)):
        if buf is None:
            continue
        what = 'masked_bce %s n=%d' % (name, n)
        worst = max(worst, bounded_check(ref, 1e-6 + 1e-6 * ref.abs(), buf, what))
        assert bool((buf[:n][pad] == 0).all()), what + ': a pad is not exactly 0'
    if d_buf is not None:
        assert bool((d_buf[:n][bce_outside_clip(c)] == 0).all()), 'masked_bce n=%d: gradient outside the clip range' % n
    assert float(sums[1]) == BCE_SUMS_START[1] + float((~pad).sum()), 'masked_bce n=%d: count %r, %d items are no pads' % (n, float(sums[1]), int((~pad).sum()))
    own = (item_buf if item_buf is not None else item_for_sum)[:n].double()
    err = abs(float(sums[0]) - (BCE_SUMS_START[0] + float(own.sum())))
    assert err <= bce_sum_bound(n, float(own.abs().sum())), 'masked_bce n=%d: sum off by %.3e, bound %.3e' % (n, err, bce_sum_bound(n, float(own.abs().sum())))
    return worst


COUNTS_START = (1.0, 2.0, 3.0, 4.0, 5.0, 6.0)


def counts_case(n, dtype):
    g = gen(6, n)
    yp = torch.rand(n, generator=g) * 2.0
    yt = torch.randint(0, 2, (n,), generator=g).float()
    yt[torch.rand(n, generator=g) < 0.3] = -1.0
    k = min(n, 3)
    yp[:k] = torch.tensor([0.5, 1.5, 2.5])[:k]                  # ties: half to even gives 0, 2, 2
    yt[:k] = torch.tensor([1.0, 1.0, 0.0])[:k]
    if n >= 6:
        yp[n - 3:] = torch.tensor([2.5, 0.5, 1.5])
        yt[n - 3:] = torch.tensor([1.0, 0.0, 1.0])
    yp = yp.to(dtype)
    ones = (torch.round(yp.double()) == 1.0).nonzero().reshape(-1)
    yt[ones[::4]] = -1.0                                         # pads where the prediction rounds to 1: the F1 counts are not masked
    return {'n': n, 'dtype': dtype, 'y_true': yt, 'y_pred': yp}


def counts_ref(c, wrong=None, upto=None):
    """the six integer counts of one pass (int64); wrong = 'half_up': round(x) = floor(x + 0.5)"""
    yt, yp = c['y_true'].double()[:upto], c['y_pred'].double()[:upto]
    r = torch.floor(yp + 0.5) if wrong == 'half_up' else torch.round(yp)        # torch.round: half to even, as rintf and tf.round
    m = (yt != -1.0).double()
    ct, pt = yt.long() == 1, r.long() == 1
    return torch.tensor([float((m * yt).sum()), float(m.sum()), float((m * r).sum()), float((ct & pt).sum()), float(ct.sum()),
                         float(pt.sum())], dtype=torch.float64).long()


def counts_emulate(c, wrong=None):
    """the six floats after TWO calls from COUNTS_START"""
    one = counts_ref(c, wrong, min(c['n'], BCE_THREADS) if wrong == 'second_trip' else None).double()
    start = torch.tensor(COUNTS_START, dtype=torch.float64)
    return (one if wrong == 'overwrite' else start + 2 * one).float()


def counts_check(c, out6):
    want = torch.tensor(COUNTS_START, dtype=torch.float64) + 2 * counts_ref(c).double()
    assert float(want.max()) < 2 ** 24
    assert torch.equal(out6.double(), want), 'binary_counts n=%d: %r, restatement %r' % (c['n'], out6.tolist(), want.tolist())


# =====================================================================================================================
# 3. one workgroup per row: softmax backward, sparse CE on probabilities backward, sampled-softmax CE
# =====================================================================================================================
ROW_SHAPES = ((3, 5), (3, 2047), (3, 2048), (3, 2049), (3, 2056), (3, 4100), (4097, 24), (8200, 13))
ROW_PITCH_EXTRA = (0, 8)


def _row_wrong_columns(V, wrong):
    """columns a wrong variant never looks at"""
    if wrong == 'last_chunk':
        return slice((V - 1) // 8 * 8, V)
    if wrong == 'from_2048':
        return slice(min(V, ROW_TRIP), V)
    return slice(V, V)


def softmax_bwd_case(R, V, extra, dtype):
    g = gen(7, R, V, extra)
    ld = rup8(V) + extra
    logits = torch.randn(R, V, generator=g)
    logits[:, V - 1] = logits.max(dim=1)[0] + 2.0            # the largest g * p of a row sits in its last valid column:
    p = torch.softmax(logits, dim=1).to(dtype)
    gr = torch.randn(R, V, generator=g).clamp(-5.0, 5.0)
    gr[:, V - 1] = 6.0                                       # a lost tail chunk moves the row sum, and with it every output
    gr = gr.to(dtype)
    return {'R': R, 'V': V, 'ld': ld, 'dtype': dtype, 'p': p, 'g': gr, 'p_buf': pitched(p, ld), 'g_buf': pitched(gr, rup8(V) + 8 - extra)}


def softmax_bwd_ref(c):
    p, g = c['p'].double(), c['g'].double()
    return p * (g - (p * g).sum(dim=1, keepdim=True))


def softmax_bwd_bound(c, ref):
    """fp32: 1e-6 * max|g|, the bound of test_softmax_rows_backward_kernel (the row sum of g * p is a chain of at most
    V / 256 + 10 roundings of magnitudes that add up to <= max|g|, times p_j <= 1).  bf16: one bf16 ulp of the result beside it."""
    b = 1e-6 * float(c['g'].double().abs().max())
    return torch.full_like(ref, b) if c['dtype'] == F32 else BF_ULP * ref.abs() + b


def softmax_bwd_emulate(c, wrong=None):
    assert wrong in (None,) + WRONG_ROWS
    R, V, ld = c['R'], c['V'], c['ld']
    p, g = c['p'].double(), c['g'].double()
    gp = p * g
    s = gp.sum(dim=1, keepdim=True)
    lost = _row_wrong_columns(V, wrong)
    s = s - gp[:, lost].sum(dim=1, keepdim=True)
    if wrong == 'tail_counts':                               # the pad columns of the last chunk hold SENT in both operands
        s = s + (rup8(V) - V) * float(SENT) * float(SENT)
    buf, out = row_buffer(R, ld, c['dtype'])
    out[:] = 0
    out[:, :V] = (p * (g - s)).to(c['dtype'])
    out[:, lost] = SENT
    if wrong == 'rows_4096':
        out[ROW_CAP:] = SENT
    return buf


def softmax_bwd_check(c, buf):
    R, V, ld = c['R'], c['V'], c['ld']
    what = 'softmax_rows_bwd R=%d V=%d ld=%d %s' % (R, V, ld, c['dtype'])
    ref = softmax_bwd_ref(c)
    out = rows_of(buf, R, ld)
    err = (out[:, :V].double() - ref).abs()
    bound = softmax_bwd_bound(c, ref)
    assert bool((err <= bound).all()), '%s: %d elements past the bound, worst %.3e of it' % (what, int((err > bound).sum()), float((err / bound).max()))
    assert bool((out[:, V:] == 0).all()), what + ': columns V .. ld - 1 are not 0'
    assert_tail(buf, R * ld, what)


CE_TF, CE_PLAIN = 0, 1       # B4C_CE_TF, B4C_CE_PLAIN of include/b4c.h (the GPU test asserts that they agree)
SPARSE_GS = 0.37
SPARSE_GAP_FILL = 0.5


def sparse_bwd_case(R, V, extra, dtype):
    g = gen(8, R, V, extra)
    ld = rup8(V) + extra
    p = torch.softmax(torch.randn(R, V, generator=g) * 3.0, dim=1)
    if V > 2:
        p[:, 1] = 3e-8                                       # below the clip range
    if V > 3:
        p[:, 2] = 0.0
    lab = torch.randint(0, V, (R,), generator=g).float()
    lab[torch.rand(R, generator=g) < 0.3] = -1.0
    # three rows: class 0 / pad / class V - 1, or (the wider pitch) class V - 1 / a label past the table / class 0; long tables have all of them
    first = [0.0, -1.0, V - 1.0] if extra == 0 else [V - 1.0, V + 2.0, 0.0]
    lab[:3] = torch.tensor(first)
    if R > 8:
        lab[3:8] = torch.tensor([V - 1.0, V + 2.0, 0.0, -1.0, -2.0])
        lab[R - 3:] = torch.tensor([0.0, V + 0.0, V - 1.0])  # rows a workgroup reaches on its second or third turn
    rows_last = (lab == V - 1.0).nonzero().reshape(-1)
    p[rows_last[::2], V - 1] = 1.0                           # above the clip range, at the label
    if V > 3:
        p[lab == 2.0, 2] = 0.25                              # (the plain variant divides by p_y: no zero at a label)
    p = p.to(dtype)
    # the pad columns of the input hold SPARSE_GAP_FILL, a value inside the clip range: a kernel that let them count would add it to S
    return {'R': R, 'V': V, 'ld': ld, 'dtype': dtype, 'p': p, 'labels': lab, 'gs': float(np.float32(SPARSE_GS)),
            'p_buf': pitched(p, rup8(V) + 8 - extra, SPARSE_GAP_FILL)}


def sparse_bwd_ref(c, variant, wrong=None):
    """-> d loss / d p (float64; NaN rows where the label is out of range), the bound per row [R][1], pad mask, bad mask.
    TF: loss_r = log sum_j clip(p_j) - log clip(p_y), d/dp_j = u_j (1 / S - [j = y] / clip(p_y)), u_j = [eps <= p_j <= 1 - eps];
    plain: -[j = y] / p_y; times gs; 0 for pad rows.  Bound: S is a chain of at most V additions of positive terms, then 1 / S, the
    difference, the product with gs and (TF) u: (V + 4) * 2^-24 of gs * max(1 / S, 1 / clip(p_y)), for both variants (the plain one
    is a division and a product: two roundings of gs / p_y, and gs / p_y <= gs / clip(p_y) / 0.3 at the smallest planted p_y, 3e-8).
    Beside the issue's bound: a bf16 output adds its own rounding, BF_ULP of the value (sparse_bwd_check)."""
    R, V, gs = c['R'], c['V'], c['gs']
    p, lab = c['p'].double(), c['labels']
    pad = lab == -1.0
    y = lab.long()
    bad = ~pad & ((y < 0) | (y >= V))
    yc = y.clamp(0, V - 1)
    lo, hi = F32_EPS, F32_HI
    pc = p.clamp(lo, hi)
    S = pc.sum(dim=1, keepdim=True)
    lost = _row_wrong_columns(V, wrong)
    S = S - pc[:, lost].sum(dim=1, keepdim=True)
    if wrong == 'tail_counts':
        S = S + (rup8(V) - V) * SPARSE_GAP_FILL
    py = p.gather(1, yc[:, None])
    onehot = torch.zeros(R, V, dtype=torch.float64).scatter_(1, yc[:, None], 1.0)
    if variant == CE_TF:
        u = ((p >= lo) & (p <= hi)).double()
        d = u * (1.0 / S - onehot / py.clamp(lo, hi))
    else:
        d = torch.where(onehot > 0, -1.0 / py, torch.zeros_like(onehot))
    scale = torch.maximum(1.0 / S, 1.0 / py.clamp(lo, hi))
    d = d * gs
    d[pad] = 0.0
    d[bad] = float('nan')
    return d, (V + 4) * U24 * gs * scale, pad, bad


def sparse_bwd_emulate(c, variant, wrong=None):
    R, V, ld = c['R'], c['V'], c['ld']
    d, _, pad, bad = sparse_bwd_ref(c, variant, wrong)
    buf, out = row_buffer(R, ld, c['dtype'])
    out[:] = 0
    out[:, :V] = d.to(c['dtype'])
    out[:, _row_wrong_columns(V, wrong)] = SENT
    if wrong == 'rows_4096':
        out[ROW_CAP:] = SENT
    return buf


def sparse_bwd_check(c, variant, buf):
    R, V, ld = c['R'], c['V'], c['ld']
    what = 'sparse_ce_from_probs_bwd variant=%d R=%d V=%d ld=%d %s' % (variant, R, V, ld, c['dtype'])
    ref, bound, pad, bad = sparse_bwd_ref(c, variant)
    out = rows_of(buf, R, ld)
    good = ~pad & ~bad
    err = (out[good][:, :V].double() - ref[good]).abs()
    b = bound[good].expand(-1, V)
    if c['dtype'] == BF16:
        b = b + BF_ULP * ref[good].abs()
    assert bool((err <= b).all()), '%s: %d elements past the bound' % (what, int((~(err <= b)).sum()))
    assert bool((out[pad] == 0).all()), what + ': a pad row is not exactly 0'
    assert bool((out[:, V:] == 0).all()), what + ': columns V .. ld - 1 are not 0'
    assert bool(torch.isnan(out[bad][:, :V]).all()), what + ': a row with a label outside the table is not NaN'
    assert_tail(buf, R * ld, what)


SAMPLED_RANGE = 5000
SAMPLED_GS = (1.0, 0.37)
SAMPLED_GAP_FILL = 50.0      # what the pad columns of Z hold on entry: a kernel that let them count would see exp(50 - m)


def log_uniform_ids_host(seed, n, range_max):
    """host restatement of b4c_log_uniform_sample's ids (the CPU tests' stand-in for the device sampler)"""
    from bert4clickpath_amd import ops
    u = (ops.rand64_host(seed, np.arange(n, dtype=np.uint64)) >> np.uint64(40)).astype(np.float64) / 16777216.0
    return torch.from_numpy(np.clip(np.floor(np.exp(u * np.log(range_max + 1.0))).astype(np.int64) - 1, 0, range_max - 1))


def sampled_case(R, K, extra, dtype, gs, samples, all_hits=False):
    """samples: int64 [K] from the log-uniform sampler.  all_hits: the draw is one id K times, and row 0 carries it as its label"""
    g = gen(9, R, K, extra)
    ld = rup8(K) + extra
    samples = samples.clone()
    if all_hits:
        samples[:] = samples[0]
    lab = torch.randint(0, SAMPLED_RANGE, (R,), generator=g).int()
    lab[0] = int(samples[K - 1])                             # an accidental hit in column K - 1
    lab[1] = int(samples[2047]) if K > 2047 else lab[1]      # and in column 2047, the last of a thread's first chunk
    lab[2] = -1 if extra == 0 else SAMPLED_RANGE + 5
    if R > 8:
        lab[3::5] = samples[torch.randint(0, K, (len(lab[3::5]),), generator=g)].int()
        lab[4::11] = -1
        lab[5::13] = SAMPLED_RANGE + torch.arange(len(lab[5::13]), dtype=torch.int32)
        lab[R - 1] = int(samples[0])
    Z = (torch.randn(R, K, generator=g) * 2.0).to(dtype)
    zbuf = pitched(Z, ld)
    rows_of(zbuf, R, ld)[:, K:] = SAMPLED_GAP_FILL
    return {'R': R, 'K': K, 'ld': ld, 'dtype': dtype, 'gs': float(np.float32(gs)), 'samples': samples, 'labels': lab, 'Z': Z,
            'Z_buf': zbuf, 'ztrue': torch.randn(R, generator=g)}


def sampled_hits(c):
    return c['samples'][None, :] == c['labels'].long()[:, None]


def sampled_ref(c, wrong=None):
    """-> loss [R], gs * softmax over the negatives [R][K], dtrue [R] (float64), ignored-row mask.
    z_t = ztrue - logQ(y), negatives equal to the label removed (-inf), loss = logsumexp(z_t, z_.) - z_t,
    Z <- gs * softmax_j, dtrue = gs * (softmax_t - 1); rows with label < 0 or >= range_max: loss 0, zero gradient."""
    K, gs = c['K'], c['gs']
    lab = c['labels'].long()
    ign = (lab < 0) | (lab >= SAMPLED_RANGE)
    zt = c['ztrue'].double() - torch.from_numpy(nr.log_uniform_logq(lab.clamp(0, SAMPLED_RANGE - 1).numpy(), SAMPLED_RANGE, K))
    zn = c['Z'].double().clone()
    zn[sampled_hits(c)] = -math.inf
    zn[:, _row_wrong_columns(K, wrong)] = -math.inf
    if wrong == 'tail_counts' and rup8(K) > K:
        zn = torch.cat([zn, torch.full((c['R'], rup8(K) - K), SAMPLED_GAP_FILL, dtype=torch.float64)], dim=1)
    m = torch.maximum(zt, zn.max(dim=1)[0])
    e, et = torch.exp(zn - m[:, None]), torch.exp(zt - m)
    s = e.sum(dim=1) + et
    loss = torch.log(s) + m - zt
    dZ = gs * e[:, :K] / s[:, None]
    dtrue = gs * (et / s - 1.0)
    loss[ign], dtrue[ign], dZ[ign] = 0.0, 0.0, 0.0
    return loss, dZ, dtrue, ign


def sampled_emulate(c, wrong=None):
    """-> Z buffer (in place), item_loss buffer, dtrue buffer"""
    assert wrong in (None,) + WRONG_ROWS
    R, K, ld = c['R'], c['K'], c['ld']
    loss, dZ, dtrue, _ = sampled_ref(c, wrong)
    zbuf = c['Z_buf'].clone()
    out = rows_of(zbuf, R, ld)
    keep = out.clone()
    out[:] = 0
    out[:, :K] = dZ.to(c['dtype'])
    lost = _row_wrong_columns(K, wrong)
    out[:, lost] = keep[:, lost]
    ibuf, dbuf = elemwise_emulate(loss.float()), elemwise_emulate(dtrue.float())
    if wrong == 'rows_4096':
        out[ROW_CAP:] = keep[ROW_CAP:]
        ibuf[ROW_CAP:], dbuf[ROW_CAP:] = SENT, SENT
    return zbuf, ibuf, dbuf


def sampled_sum_bound(c, magnitude, z_magnitude):
    """sum_j Z[r][j] + dtrue[r] = gs * (sum_j softmax_j + softmax_t - 1) = 0 exactly.  In fp32 the kernel's s is a chain of 8 * ceil(K / 2048) additions per
    thread, 6 butterfly steps, 4 workgroup partials and the true class's term; every output then takes 1 / s, two products and
    (dtrue) a difference: 6 more.  The exponentials are the same values in s and in the outputs, so their own error cancels.
    bf16 rows: each stored Z adds its rounding, up to BF_ULP of itself (z_magnitude = sum_j |Z[r][j]|)."""
    b = chain_bound(8 * -(-c['K'] // ROW_TRIP) + 11 + 6, magnitude)
    return b if c['dtype'] == F32 else b + BF_ULP * z_magnitude


def sampled_check(c, zbuf, ibuf, dbuf):
    """-> worst err / bound of the Z / dtrue comparison"""
    R, K, ld, gs = c['R'], c['K'], c['ld'], c['gs']
    what = 'sampled_ce_fwd_bwd R=%d K=%d ld=%d %s gs=%g' % (R, K, ld, c['dtype'], gs)
    loss, dZ, dtrue, ign = sampled_ref(c)
    out = rows_of(zbuf, R, ld)
    got_loss, got_dt = ibuf[:R].double(), dbuf[:R].double()
    assert bool(torch.isfinite(out.double()).all() and torch.isfinite(got_loss).all() and torch.isfinite(got_dt).all()), what + ': non-finite'
    err = (got_loss - loss).abs()
    assert bool((err <= 1e-5 * loss.abs().clamp(min=1.0)).all()), '%s: item_loss off by %.3e' % (what, float(err.max()))
    assert bool((got_loss[ign] == 0).all() and (got_dt[ign] == 0).all() and (out[ign] == 0).all()), what + ': an ignored row is not all 0'
    assert bool((out[:, :K][sampled_hits(c)] == 0).all()), what + ': a removed accidental hit has a gradient'
    assert bool((out[:, K:] == 0).all()), what + ': columns K .. ld - 1 are not 0'
    total = out.double().sum(dim=1) + got_dt           # gs * (1 - softmax_t) + gs * (softmax_t - 1); softmax_t itself is of size 1: gs in `mag`
    zmag = out.double().abs().sum(dim=1)
    mag = zmag + got_dt.abs() + gs
    live = ~ign
    assert bool((total[live].abs() <= sampled_sum_bound(c, mag[live], zmag[live])).all()), '%s: softmax rows do not sum to 1 (worst %.3e)' % (what, float(total[live].abs().max()))
    bz = torch.full_like(dZ, 2e-5 * gs)
    if c['dtype'] == BF16:
        bz = bz + BF_ULP * dZ.abs()
    ez, ed = (out[:, :K].double() - dZ).abs(), (got_dt - dtrue).abs()
    assert bool((ez <= bz).all()), '%s: %d gradients past the bound, worst %.3f of it' % (what, int((ez > bz).sum()), float((ez / bz).max()))
    assert bool((ed <= 2e-5 * gs).all()), '%s: dtrue off by %.3e' % (what, float(ed.max()))
    assert_tail(zbuf, R * ld, what)
    assert_tail(ibuf, R, what)
    assert_tail(dbuf, R, what)
    return max(float((ez / bz).max()), float(ed.max()) / (2e-5 * gs))


# =====================================================================================================================
# 4. a wave per row, a vector per element
# =====================================================================================================================
ROW_DOT_R = (1, 3, 4, 5, 8193)
ROW_DOT_WIDTH = (8, 512, 520, 1032)
ROW_DOT_ROW_TRIP = 4 * 2048          # 4 rows per workgroup, 2048 workgroups: row 8192 is a second trip
ROW_DOT_LANE_TRIP = 64 * 8           # a lane's second 8-column chunk starts at column 512


def row_dot_case(R, width, dtype, integers, pitch_a):
    g = gen(10, R, width, integers)
    if integers:
        a, b = (torch.randint(-8, 9, (R, width), generator=g).to(dtype) for _ in range(2))
    else:
        a, b = (torch.randn(R, width, generator=g).to(dtype) for _ in range(2))
    lda, ldb = (width + GAP, width) if pitch_a else (width, width + GAP)
    return {'R': R, 'width': width, 'dtype': dtype, 'integers': integers, 'a': a, 'b': b, 'lda': lda, 'ldb': ldb,
            'a_buf': pitched(a, lda), 'b_buf': pitched(b, ldb)}


def row_dot_ref(c, wrong=None):
    prod = c['a'].double() * c['b'].double()
    if wrong == 'lane_trip':
        prod = prod[:, :ROW_DOT_LANE_TRIP]
    if wrong == 'last_chunk':
        prod = prod[:, :c['width'] - 8]
    return prod.sum(dim=1)


def row_dot_bound(c):
    """a lane adds width / 512 chunks of 8 products (fused multiply-adds: one rounding each), the wave sum is 6 butterfly steps:
    width / 8 + 8 roundings cover the longest chain, each 2^-24 of a partial sum that is at most sum |a b|"""
    return chain_bound(c['width'] / 8 + 8, (c['a'].double() * c['b'].double()).abs().sum(dim=1))


def row_dot_emulate(c, wrong=None):
    return elemwise_emulate(row_dot_ref(c, wrong).float(), 'second_trip' if wrong == 'second_trip' else None, ROW_DOT_ROW_TRIP)


def row_dot_check(c, buf):
    what = 'row_dot R=%d width=%d %s integers=%d' % (c['R'], c['width'], c['dtype'], c['integers'])
    ref = row_dot_ref(c)
    if c['integers']:
        assert float(ref.abs().max()) < 2 ** 24
        exact_check(ref.float(), buf, what)
    else:
        bounded_check(ref, row_dot_bound(c), buf, what)


ROWS8_SHAPES = ((1, 8), (37, 72), (70000, 64))           # 70,000 x 64 / 8 = 560,000 work items: past EW_THREADS
SCALES = (-2.0, -0.5, 0.0, 0.25, 3.0)


def rows8_trip_row(width):
    return EW_THREADS // (width // 8)                    # the first row whose chunks all belong to the second trip (rounded down: partly)


def row_scale_case(R, width, dtype):
    g = gen(11, R, width)
    src = torch.randint(-8, 9, (R, width), generator=g).to(dtype)
    scale = torch.tensor(SCALES)[torch.randint(0, len(SCALES), (R,), generator=g)]
    return {'R': R, 'width': width, 'dtype': dtype, 'src': src, 'scale': scale, 'ld': width + GAP, 'ld_out': width + GAP,
            'src_buf': pitched(src, width + GAP)}


def row_scale_emulate(c, wrong=None):
    out = c['src'].float() * c['scale'][:, None]
    buf = pitched(out, c['ld_out'])
    if wrong == 'second_trip':
        flat = rows_of(buf, c['R'], c['ld_out'])[:, :c['width']].reshape(-1, 8).clone()
        flat[EW_THREADS:] = SENT
        rows_of(buf, c['R'], c['ld_out'])[:, :c['width']] = flat.view(c['R'], c['width'])
    return buf


def pitched_exact_check(ref, ld, buf, what):
    """[rows][width] bit for bit, the gap columns and the tail untouched"""
    rows, width = ref.shape
    got = rows_of(buf, rows, ld)[:, :width]
    assert same_bits(got.contiguous(), ref.contiguous()), '%s: %d elements differ' % (what, int((bits(got) != bits(ref)).sum()))
    assert_gap(buf, rows, ld, width, what)


def row_scale_check(c, buf):
    pitched_exact_check(c['src'].float() * c['scale'][:, None], c['ld_out'], buf, 'row_scale_f32 R=%d width=%d %s' % (c['R'], c['width'], c['dtype']))


ROWS_ADD_DTYPES = ((F32, F32), (BF16, BF16), (BF16, F32))      # (destination, source)


def rows_add_case(n_src, width, dtype, src_dtype):
    g = gen(12, n_src, width)
    n_dst = n_src + 5
    perm = torch.randperm(n_dst, generator=g).int()
    idx = perm[:n_src].clone()                                 # injective
    idx[torch.randperm(n_src, generator=g)[:(n_src + 2) // 3]] = -1
    if n_src > 8:
        idx[n_src - 1] = perm[n_src]                           # the last source row counts (a destination nobody else has)
    src = torch.randint(-8, 9, (n_src, width), generator=g).to(src_dtype)
    dst = torch.randint(-4, 5, (n_dst, width), generator=g).to(dtype)
    return {'n_src': n_src, 'n_dst': n_dst, 'width': width, 'dtype': dtype, 'src_dtype': src_dtype, 'idx': idx, 'src': src, 'dst': dst,
            'ld_dst': width + GAP, 'ld_src': width + GAP, 'src_buf': pitched(src, width + GAP), 'dst_buf': pitched(dst, width + GAP)}


def rows_add_ref(c, wrong=None):
    live = (c['idx'] >= 0).nonzero().reshape(-1)
    if wrong == 'second_trip':
        live = live[live < rows8_trip_row(c['width'])]
    src, to = c['src'].double()[live], c['idx'].long()[live]
    if wrong == 'overwrite':
        return c['dst'].double().index_copy(0, to, src).to(c['dtype'])
    return c['dst'].double().index_add(0, to, src).to(c['dtype'])


def rows_add_emulate(c, wrong=None):
    return pitched(rows_add_ref(c, wrong), c['ld_dst'])


def rows_add_check(c, buf):
    pitched_exact_check(rows_add_ref(c), c['ld_dst'], buf, 'rows_add n=%d width=%d %s <- %s' % (c['n_src'], c['width'], c['dtype'], c['src_dtype']))


ROWS4_SHAPES = ((1, 4), (100, 36), (33000, 64))          # 33,000 x 64 / 4 = 528,000 work items: past EW_THREADS
HOT_SOURCES = 1000


def rows4_trip_row(width):
    return EW_THREADS // (width // 4)


def rows_gather_case(n, width):
    g = gen(13, n, width)
    rows = max(7, n // 3)
    table = torch.randint(-8, 9, (rows, width), generator=g).float()
    idx = torch.randint(0, rows, (n,), generator=g)
    idx[torch.rand(n, generator=g) < 0.2] = -1
    if n > 8:
        idx[n - 1], idx[n - 2] = rows - 1, -3
    return {'n': n, 'width': width, 'rows': rows, 'table': table, 'idx': idx, 'ld_src': width + GAP, 'ld_out': width + GAP,
            'table_buf': pitched(table, width + GAP)}


def rows_gather_ref(c):
    out = c['table'][c['idx'].clamp(min=0)]
    out[c['idx'] < 0] = 0.0
    return out


def rows_gather_emulate(c, wrong=None):
    out = rows_gather_ref(c)
    if wrong == 'second_trip':
        out[rows4_trip_row(c['width']):] = SENT
    return pitched(out, c['ld_out'])


def rows_gather_check(c, buf):
    pitched_exact_check(rows_gather_ref(c), c['ld_out'], buf, 'rows_gather_f32 n=%d width=%d' % (c['n'], c['width']))


def rows_scatter_case(n, width):
    g = gen(14, n, width)
    rows = max(7, n // 3)
    src = torch.randint(-8, 9, (n, width), generator=g).float()
    idx = torch.randint(0, rows, (n,), generator=g)
    idx[torch.rand(n, generator=g) < 0.2] = -1
    hot = torch.randperm(n, generator=g)[:min(HOT_SOURCES, (2 * n + 2) // 3)]       # one row receives a thousand sources
    idx[hot] = 3
    if n > 8:
        idx[n - 1] = rows - 1
        src[n - 1] = 8.0
    dst = torch.randint(-4, 5, (rows, width), generator=g).float()
    return {'n': n, 'width': width, 'rows': rows, 'src': src, 'idx': idx, 'dst': dst, 'ld_src': width + GAP, 'ld_dst': width + GAP,
            'src_buf': pitched(src, width + GAP), 'dst_buf': pitched(dst, width + GAP)}


def rows_scatter_ref(c, wrong=None):
    live = (c['idx'] >= 0).nonzero().reshape(-1)
    if wrong == 'second_trip':
        live = live[live < rows4_trip_row(c['width'])]
    if wrong == 'lost_duplicate':                            # the last of the hot row's sources never arrives
        hot = live[c['idx'][live] == 3]
        live = live[live != hot[-1]]
    src, to = c['src'].double()[live], c['idx'][live]
    if wrong == 'overwrite':
        return c['dst'].double().index_copy(0, to, src).float()
    return c['dst'].double().index_add(0, to, src).float()


def rows_scatter_emulate(c, wrong=None):
    return pitched(rows_scatter_ref(c, wrong), c['ld_dst'])


def rows_scatter_check(c, buf):
    ref = rows_scatter_ref(c)
    assert float(ref.abs().max()) < 2 ** 24
    pitched_exact_check(ref, c['ld_dst'], buf, 'rows_scatter_add_f32 n=%d width=%d' % (c['n'], c['width']))


FLAT_N = (1, 257, 524288 + 300)


def scatter_1d_case(n):
    g = gen(15, n)
    slots = 300
    src = torch.randint(-8, 9, (n,), generator=g).float()
    idx = torch.randint(0, slots, (n,), generator=g)
    idx[torch.rand(n, generator=g) < 0.2] = -1
    if n > 8:
        idx[n - 1], src[n - 1] = slots - 1, 8.0
    return {'n': n, 'slots': slots, 'src': src, 'idx': idx, 'dst': torch.randint(-4, 5, (slots,), generator=g).float()}


def scatter_1d_ref(c, wrong=None):
    live = (c['idx'] >= 0).nonzero().reshape(-1)
    if wrong == 'second_trip':
        live = live[live < EW_THREADS]
    if wrong == 'lost_duplicate':
        live = live[:-1]
    src, to = c['src'].double()[live], c['idx'][live]
    if wrong == 'overwrite':
        return c['dst'].double().index_copy(0, to, src).float()
    return c['dst'].double().index_add(0, to, src).float()


def scatter_1d_emulate(c, wrong=None):
    return elemwise_emulate(scatter_1d_ref(c, wrong))


def scatter_1d_check(c, buf):
    ref = scatter_1d_ref(c)
    assert float(ref.abs().max()) < 2 ** 24
    exact_check(ref, buf, 'scatter_add_1d n=%d' % c['n'])


def gather_i64_case(n):
    g = gen(16, n)
    src = torch.randint(-2 ** 40, 2 ** 40, (1000,), generator=g)
    src[:4] = torch.tensor([2 ** 32 + 1, -2 ** 32 - 1, 2 ** 62, 0])
    idx = torch.randint(0, 1000, (n,), generator=g).int()
    idx[n - 1] = 0
    return {'n': n, 'src': src, 'idx': idx}


def gather_i64_emulate(c, wrong=None):
    return elemwise_emulate(c['src'][c['idx'].long()], wrong, EW_THREADS)


def gather_i64_check(c, buf):
    assert torch.equal(buf[:c['n']], c['src'][c['idx'].long()]), 'gather_i64 n=%d' % c['n']
    assert_tail(buf, c['n'], 'gather_i64')


TRANSPOSE_SHAPES = ((1, 1), (31, 33), (32, 32), (33, 31), (128, 1003))


def transpose_add_case(K, N, extra_src, extra_dst):
    g = gen(17, K, N)
    src = torch.randint(-8, 9, (K, N), generator=g).float()
    dst = torch.randint(-4, 5, (N, K), generator=g).float()
    return {'K': K, 'N': N, 'src': src, 'dst': dst, 'ld_src': N + extra_src, 'ld_dst': K + extra_dst,
            'src_buf': pitched(src, N + extra_src), 'dst_buf': pitched(dst, K + extra_dst)}


def transpose_add_emulate(c, wrong=None):
    return pitched(c['src'].t().contiguous() if wrong == 'overwrite' else c['dst'] + c['src'].t(), c['ld_dst'])


def transpose_add_check(c, buf):
    pitched_exact_check(c['dst'] + c['src'].t(), c['ld_dst'], buf, 'transpose_add K=%d N=%d' % (c['K'], c['N']))


POISON_SHAPES = ((1, 1), (7, 5), (2100, 257))            # 2100 x 257 = 539,700 elements: past EW_THREADS
POISON_DTYPES = (F32, BF16, I32)


def poison_case(rows, width, extra, dtype):
    x = torch.randint(-4, 5, (rows, width), generator=gen(18, rows, width)).to(dtype)
    return {'rows': rows, 'width': width, 'ld': width + extra, 'dtype': dtype, 'x_buf': pitched(x, width + extra)}


def poison_emulate(c, flag, wrong=None):
    buf = c['x_buf'].clone()
    if flag < 0:
        block = rows_of(buf, c['rows'], c['ld'])[:, :c['width']]
        new = torch.full((c['rows'] * c['width'],), -1 if c['dtype'] == I32 else float('nan'), dtype=c['dtype'])
        if wrong == 'second_trip':
            new[EW_THREADS:] = block.reshape(-1)[EW_THREADS:]
        block[:] = new.view(c['rows'], c['width'])
    return buf


def poison_check(c, flag, buf):
    what = 'poison_rows rows=%d width=%d ld=%d %s flag=%d' % (c['rows'], c['width'], c['ld'], c['dtype'], flag)
    if flag >= 0:
        assert same_bits(buf, c['x_buf']), what + ': the buffer changed'
        return
    block = rows_of(buf, c['rows'], c['ld'])[:, :c['width']]
    assert bool((block == -1).all() if c['dtype'] == I32 else torch.isnan(block).all()), what + ': the block is not all poison'
    keep = torch.ones(buf.shape, dtype=torch.bool)
    rows_of(keep, c['rows'], c['ld'])[:, :c['width']] = False
    assert same_bits(buf[keep], c['x_buf'][keep]), what + ': something outside [rows][width] changed'


BOOKKEEPING_R = (0, 1, 3, 4, 5, 1023, 1025, 4099)


def label_scale_case(R, V=37):
    lab = torch.randint(-3, V + 3, (R + 1,), generator=gen(19, R)).int()        # element 0: in front of the one-off pointer
    return {'R': R, 'V': V, 'buf': lab}


def label_scale_ref(c, off, wrong=None):
    """-> (1 / n as fp32 computes it, n); wrong = 'scalar_tail': the elements after the last whole group of four are not counted"""
    lab = c['buf'][off:off + c['R']]
    if wrong == 'scalar_tail':
        lab = lab[:c['R'] // 4 * 4]
    n = int(((lab >= 0) & (lab < c['V'])).sum())
    return torch.tensor([float(np.float32(1.0) / np.float32(n)) if n else 0.0, float(n)])


def label_scale_check(c, off, buf):
    """buf: the two outputs in a SENT-filled buffer of 2 + TAIL"""
    assert torch.equal(buf[:2], label_scale_ref(c, off)), 'label_scale R=%d off=%d: %r' % (c['R'], off, buf[:2].tolist())
    assert_tail(buf, 2, 'label_scale')


def sum_scaled_case(R):
    return {'R': R, 'buf': torch.randint(-8, 9, (R + 1,), generator=gen(20, R)).float(), 'scale': 0.25}


def sum_scaled_ref(c, off, wrong=None):
    item = c['buf'][off:off + c['R']]
    if wrong == 'scalar_tail':
        item = item[:c['R'] // 4 * 4]
    return float(item.double().sum()) * c['scale']


def sum_scaled_check(c, off, plain, flag_ok, flag_bad):
    want = sum_scaled_ref(c, off)
    assert plain == want and flag_ok == want and math.isnan(flag_bad), 'sum_scaled R=%d off=%d: %r %r %r, restatement %r' % (
        c['R'], off, plain, flag_ok, flag_bad, want)
