"""The extended sampled-negative losses (include/b4c.h: BPR, the weighted BCE of gBCE, the logQ correction), the parts
that need no GPU (NO REFERENCE ORACLE: an extension -- the float64 restatement is tests/candidate_loss_ex_ref.py): the entry
point's declaration and its binding, the argument checks that refuse a call before any launch, the host checks of ops.candidate_loss_fwd_ex
and of the model's keywords, the restatement against candidate_loss_ref's and against itself, cloze.log_expected_count."""
import math
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import abi_pin
import candidate_loss_ex_ref as cx
import candidate_loss_ref as cl

A = 1 << 20                                                       # a well-aligned, never dereferenced "pointer"
NAME = 'b4c_candidate_loss_fwd_ex'


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_it_is_bound():
    from bert4clickpath_amd import _lib, ops
    c = _lib.ctypes
    lib = _lib.lib()
    declared = _lib.signatures()
    ptr, i32, i64, f32 = c.c_void_p, c.c_int, c.c_int64, c.c_float
    # (h, ld_h, table, ld_t, rows, row_off, bias, cand, ld_c, R, C, V, K, dtype, kind, beta, corr, flags, item_loss, g, ld_g, scores,
    #  ld_s, stream): b4c_candidate_loss_fwd's operands in its order, with beta, corr and flags after kind
    want = [ptr, i32, ptr, i32, i64, i64, ptr, ptr, i32, i64, i32, i32, i32, i32, i32, f32, ptr, i32, ptr, ptr, i32, ptr, i32, ptr]
    assert declared[NAME] == (c.c_int, want)
    assert list(getattr(lib, NAME).argtypes) == want and getattr(lib, NAME).restype is c.c_int
    legacy = declared['b4c_candidate_loss_fwd'][1]
    assert want[:15] == legacy[:15] and want[18:] == legacy[15:]
    consts = {k: v for k, v in _lib.header_constants(_lib._header_text(_lib.HEADER_PATH)).items() if k.startswith('B4C_CANDX_')}
    assert consts == {'B4C_CANDX_BCE': 0, 'B4C_CANDX_SOFTMAX': 1, 'B4C_CANDX_BPR': 2, 'B4C_CANDX_KINDS': 3, 'B4C_CANDX_CORR_TARGET': 1}
    assert (_lib.CANDX_BCE, _lib.CANDX_SOFTMAX, _lib.CANDX_BPR, _lib.CANDX_KINDS, _lib.CANDX_CORR_TARGET) == (0, 1, 2, 3, 1)
    assert ops.CANDX_LOSS_KINDS == {'bce': 0, 'softmax': 1, 'bpr': 2}
    assert ops.CAND_LOSS_KINDS == {'bce': 0, 'softmax': 1}       # the first feature's surface is as it was
    assert _lib.ABI_VERSION == abi_pin.ABI_VERSION and lib.b4c_abi_version() == abi_pin.ABI_VERSION
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    if cc:              # what a C compiler sees of b4c.h alone
        pre = subprocess.run([cc, '-E', '-dD', _lib.HEADER_PATH], capture_output=True, text=True, check=True).stdout
        assert re.search(r'\bint %s\(' % NAME, pre)
        for d in ('B4C_CANDX_BCE 0', 'B4C_CANDX_SOFTMAX 1', 'B4C_CANDX_BPR 2', 'B4C_CANDX_KINDS 3', 'B4C_CANDX_CORR_TARGET 1'):
            assert re.search(r'#define %s\b' % d, pre), d


def _fwd(L, h=A, ld_h=128, table=A, ld_t=128, rows=1000, row_off=10, bias=A, cand=A, ld_c=8, R=4, C=8, V=500, K=128, dtype=1, kind=2,
         beta=1.0, corr=None, flags=0, item=A, g=A, ld_g=8, scores=None, ld_s=0):
    return L.b4c_candidate_loss_fwd_ex(h, ld_h, table, ld_t, rows, row_off, bias, cand, ld_c, R, C, V, K, dtype, kind, beta, corr, flags,
                                       item, g, ld_g, scores, ld_s, None)


# what b4c_candidate_loss_fwd refuses (tests/test_candidate_loss_cpu.py: BAD_BOTH and BAD_FWD without its kind 2) ...
BAD_AS_BEFORE = [dict(h=None), dict(table=None), dict(cand=None), dict(K=0), dict(K=12), dict(K=1032), dict(C=0),
                 dict(C=1025, ld_c=1025, ld_g=1025), dict(ld_h=120), dict(ld_t=120), dict(ld_c=7), dict(ld_g=7), dict(h=A + 8),
                 dict(table=A + 4), dict(ld_h=132), dict(ld_t=130), dict(dtype=2), dict(dtype=-1), dict(V=0), dict(R=-1), dict(row_off=-1),
                 dict(row_off=501), dict(bias=None), dict(item=None), dict(g=None), dict(kind=-1), dict(scores=A, ld_s=7)]
# ... and what is new
BAD_NEW = [dict(kind=3), dict(kind=100), dict(flags=2), dict(flags=3, corr=A), dict(flags=-1, corr=A), dict(flags=1), dict(beta=-0.5),
           dict(beta=float('inf')), dict(beta=float('nan')), dict(beta=-float('inf'))]


def test_bad_arguments_are_refused_without_a_launch():
    """(every call here would fault on its made-up pointers if it were launched, and there is no device to launch on)"""
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    for kw in BAD_AS_BEFORE + BAD_NEW:
        for extra in ({}, {'R': 0}):                             # refused before R == 0 is looked at, too
            if 'R' in kw and extra:
                continue
            assert _fwd(L, **kw, **extra) == _lib._C['B4C_EINVAL'], kw
            assert b'candidate_loss_fwd_ex' in L.b4c_last_error(), (kw, L.b4c_last_error())
    assert _fwd(L, kind=3) == -1 and b'kind 3' in L.b4c_last_error()
    assert _fwd(L, flags=2) == -1 and b'flags' in L.b4c_last_error()
    assert _fwd(L, flags=1) == -1 and b'B4C_CANDX_CORR_TARGET without corr' in L.b4c_last_error()
    assert _fwd(L, beta=-0.5) == -1 and b'beta' in L.b4c_last_error()
    # nothing to do is not an error (and launches nothing): every kind, with and without the correction
    for kind in range(3):
        assert _fwd(L, R=0, kind=kind) == 0 and _fwd(L, R=0, kind=kind, corr=A, flags=1, beta=0.0) == 0
    assert _fwd(L, R=0, beta=3.0e38) == 0
    # the first entry point still refuses kind 2, under its own name
    assert L.b4c_candidate_loss_fwd(A, 128, A, 128, 1000, 10, A, A, 8, 4, 8, 500, 128, 1, 2, A, A, 8, None, 0, None) == -1
    assert b'candidate_loss_fwd: kind 2' in L.b4c_last_error()


def test_host_wrapper_validates_before_the_device_is_needed():
    from bert4clickpath_amd import ops
    h, tab, b = torch.zeros(4, 16), torch.zeros(30, 16), torch.zeros(20)
    cand = torch.zeros(4, 3, dtype=torch.int32)
    ex = ops.candidate_loss_fwd_ex
    with pytest.raises(ops.B4CError, match="'bce', 'softmax' or 'bpr'"):
        ex(h, tab, b, cand, 20, 'gbce')
    for beta in (-1.0, float('inf'), float('nan'), 'much'):
        with pytest.raises(ops.B4CError, match='beta'):
            ex(h, tab, b, cand, 20, 'bce', beta=beta)
    with pytest.raises(ops.B4CError, match='correct_target needs corr'):
        ex(h, tab, b, cand, 20, 'bpr', correct_target=True)
    for corr in (torch.zeros(19), torch.zeros(20, dtype=torch.float64), torch.zeros(2, 20), torch.zeros(40)[::2], np.zeros(20, np.float32)):
        with pytest.raises(ops.B4CError, match='corr must be a contiguous fp32'):
            ex(h, tab, b, cand, 20, 'bpr', corr=corr)
    with pytest.raises(ops.B4CError, match='multiple of 8'):
        ex(torch.zeros(4, 12), tab, b, cand, 20, 'bpr')
    with pytest.raises(ops.B4CError, match='rows 11 .. 31'):
        ex(h, tab, b, cand, 20, 'bpr', row_off=11)
    with pytest.raises(ops.B4CError, match='HIP device only'):    # everything on the host is in order: only the device is missing
        ex(h, tab, b, cand, 20, 'bpr', beta=0.0, corr=torch.zeros(20), correct_target=True)
    with pytest.raises(ops.B4CError, match="'bce' or 'softmax'"):  # the first wrapper keeps its kinds and its message
        ops.candidate_loss_fwd(h, tab, b, cand, 20, 'bpr')


def _tiny_model(V=20, d=16):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, ClozeMaskedItemPrediction
    hd = ClozeMaskedItemPrediction([], V)
    return ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': d}, hd, value_to_head='[MASK]',
                                  num_encoder_layers=1, num_attention_heads=2, dropout_rate=0.0)


def test_model_keywords_are_checked_on_the_host():
    from bert4clickpath_amd import ops
    m = _tiny_model()
    feats, labels = {'asin': torch.zeros(2, 5, dtype=torch.int64)}, torch.full((2, 3), -1.0)
    batch = dict(items=feats['asin'], labels=labels, flat_idx=None, n_real_tokens=0, candidates=torch.zeros(2, 3, dtype=torch.int32))
    for call, who in ((lambda **kw: m.candidate_loss(feats, labels, num_negatives=2, **kw), 'candidate_loss'),
                      (lambda **kw: m.next_item_loss(batch, **kw), 'next_item_loss')):
        with pytest.raises(ops.B4CError, match=r"%s: loss 'hinge' \(.*'bce', 'softmax', 'bpr' or 'gbce'\)" % who):
            call(loss='hinge')
        for t in (1.5, -0.1, float('nan'), None):
            with pytest.raises(ops.B4CError, match='gbce_t'):
                call(loss='gbce', gbce_t=t)
        with pytest.raises(ops.B4CError, match='correct_target=True needs logq'):
            call(loss='bpr', correct_target=True)
        for logq in (torch.zeros(20, dtype=torch.float64), torch.zeros(1, 20), [0.0] * 20):
            with pytest.raises(ops.B4CError, match='logq must be a device fp32'):
                call(loss='softmax', logq=logq)
    with pytest.raises(ops.B4CError, match=r"next_item_loss: loss 'hinge' \('full', "):
        m.next_item_loss(batch, loss='hinge')
    with pytest.raises(ops.B4CError, match=r"candidate_loss: loss 'full' \('bce', "):    # the whole vocabulary is next_item_loss's
        m.candidate_loss(feats, labels, num_negatives=2, loss='full')


def test_gbce_beta():
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer
    for N, V in ((1, 200), (5, 200), (100, 12102), (256, 257)):
        alpha = N / (V - 1.0)
        for fn in (cx.gbce_beta, ClickstreamTransformer.gbce_beta):
            assert abs(fn(N, V, 0.0) - 1.0) < 1e-13 and abs(fn(N, V, 1.0) - alpha) < 1e-13
            assert abs(fn(N, V, 0.75) - (0.75 * alpha + 0.25)) < 1e-13          # linear in t between the two
        assert abs(cx.gbce_beta(N, V, 0.3) - ClickstreamTransformer.gbce_beta(N, V, 0.3)) < 1e-15


# ---- cloze.log_expected_count -------------------------------------------------------------------------------------------------------
def test_log_expected_count_against_numpy():
    from bert4clickpath_amd import cloze
    cnt = cx.item_counts(300)
    assert 10 <= int((cnt == 0).sum()) <= 60 and cnt.max() >= 20 * np.median(cnt[cnt > 0])
    for N in (1, 5, 100):
        got = cloze.log_expected_count(torch.from_numpy(cnt), num_negatives=N)
        assert got.dtype == torch.float32 and got.shape == (300,)
        want = np.where(cnt > 0, np.log(np.where(cnt > 0, N * cnt / cnt.sum(), 1.0)), 0.0)
        assert np.array_equal(got.numpy()[cnt == 0], np.zeros(int((cnt == 0).sum()), np.float32))
        assert float(np.abs(got.numpy() - want).max()) <= 2.0 ** -23 * float(np.abs(want).max())
        assert np.array_equal(got.numpy(), cx.log_expected_count(cnt, N))
        # the counterpart of the cdf the sampler draws by: N q sums to N over the items that can be drawn
        assert abs(float(np.exp(want[cnt > 0]).sum()) - N) < 1e-9 * N
        uni = cloze.log_expected_count(num_items=300, num_negatives=N)
        assert uni.dtype == torch.float32 and uni.shape == (300,) and bool((uni == np.float32(math.log(N / 300.0))).all())
        assert torch.equal(cloze.log_expected_count(cnt.tolist(), num_items=300, num_negatives=N), got)
    for bad in (dict(), dict(item_counts=torch.ones(3)), dict(item_counts=torch.zeros(3, dtype=torch.int64)),
                dict(item_counts=torch.tensor([1, -1])), dict(item_counts=torch.ones(3, dtype=torch.int64), num_items=4),
                dict(num_items=0), dict(num_items=5, num_negatives=0)):
        with pytest.raises(ValueError, match='log_expected_count'):
            cloze.log_expected_count(**bad)


# ---- the restatement against candidate_loss_ref's and against itself ---------------------------------------------------------------
def _small(R=6, C=5, K=8, V=9, seed=0):
    rng = np.random.default_rng(seed)
    h, W, b = rng.standard_normal((R, K)), rng.standard_normal((V, K)) * 0.7, rng.standard_normal(V) * 0.3
    corr = rng.standard_normal(V) * 0.8
    cand = rng.integers(0, V, size=(R, C)).astype(np.int32)
    cand[1, 0] = -1                     # an ignored row
    cand[4, 0] = V + 3                  # another
    cand[0, 2] = -1                     # absent entries in the middle of a list
    cand[2, 1] = V
    cand[3, 3] = cand[3, 1]             # a repeated id
    cand[5, 4] = cand[5, 0]             # the target once more, as a negative
    return h, W, b, corr, cand


OUT = ('s', 'item', 'g', 'loss', 'dh', 'dW', 'db')


def _close(a, b, names=OUT, tol=1e-13):
    for n in names:
        assert float(np.abs(np.asarray(a[n]) - np.asarray(b[n])).max()) < tol, n


@pytest.mark.parametrize('kind', cl.KINDS)
def test_defaults_are_the_first_restatement(kind):
    h, W, b, _, cand = _small(seed=1)
    for dtype in (np.float64, np.float32):
        a, r = cx.restate(h, W, b, cand, kind, dtype=dtype), cl.restate(h, W, b, cand, kind, dtype=dtype)
        for n in OUT:
            assert np.array_equal(a[n], r[n]), (n, dtype)
        assert np.array_equal(a['z'], a['s'])
    for case in cl.CASES[:2]:
        hh, table, bb, cc = cl.inputs(*case, False)
        WW = cl.operand_rows(table, 10, case[3], False)
        _close(cx.restate(hh, WW, bb, cc, kind), cl.restate(hh, WW, bb, cc, kind))


def test_bpr_with_one_negative_is_the_softmax_over_two():
    h, W, b, corr, cand = _small(seed=2)
    cand = cand[:, :2]
    for kw in (dict(), dict(corr=corr), dict(corr=corr, correct_target=True)):
        _close(cx.restate(h, W, b, cand, 'bpr', **kw), cx.restate(h, W, b, cand, 'softmax', **kw))
    _close(cx.restate(h, W, b, cand, 'bpr'), cl.restate(h, W, b, cand, 'softmax'))


def test_softmax_ignores_a_constant_correction_of_every_entry():
    h, W, b, _, cand = _small(seed=3)
    const = np.full(W.shape[0], 1.75)
    a = cx.restate(h, W, b, cand, 'softmax', corr=const, correct_target=True)
    _close(a, cl.restate(h, W, b, cand, 'softmax'))
    # without the target it is not a constant shift of the list: the loss moves
    assert abs(float(cx.restate(h, W, b, cand, 'softmax', corr=const)['loss']) - float(a['loss'])) > 1e-3


@pytest.mark.parametrize('kind', cx.KINDS)
def test_correcting_every_entry_is_a_bias_shift(kind):
    h, W, b, corr, cand = _small(seed=4)
    a = cx.restate(h, W, b, cand, kind, corr=corr, correct_target=True)
    r = cx.restate(h, W, b - corr, cand, kind)
    _close(a, r, names=('item', 'g', 'loss', 'dh', 'dW', 'db'))
    assert float(np.abs(a['z'] - r['s']).max()) < 1e-13 and float(np.abs(a['s'] - cl.restate(h, W, b, cand, 'bce')['s']).max()) == 0
    if kind in cl.KINDS:
        _close(a, cl.restate(h, W, b - corr, cand, kind), names=('item', 'g', 'loss', 'dh', 'dW', 'db'))


def test_weighted_bce_scales_the_target_term_only():
    h, W, b, corr, cand = _small(seed=5)
    one, w = cx.restate(h, W, b, cand, 'bce', corr=corr), cx.restate(h, W, b, cand, 'bce', beta=0.37, corr=corr)
    assert float(np.abs(w['g'][:, 0] - 0.37 * one['g'][:, 0]).max()) < 1e-13 and np.array_equal(w['g'][:, 1:], one['g'][:, 1:])
    assert float(np.abs((one['item'] - w['item']) - 0.63 * one['term'][:, 0]).max()) < 1e-13
    zero = cx.restate(h, W, b, cand, 'bce', beta=0.0, corr=corr)            # beta = 0: the negatives' terms alone
    assert not zero['g'][:, 0].any() and float(np.abs(zero['item'] - one['term'][:, 1:].sum(1)).max()) < 1e-13


@pytest.mark.parametrize('target', [False, True], ids=['negatives', 'target-too'])
@pytest.mark.parametrize('kind', cx.KINDS)
def test_gradients_match_central_finite_differences(kind, target):
    h, W, b, corr, cand = _small(seed=6)
    kw = dict(beta=0.37, corr=corr, correct_target=target)
    r = cx.restate(h, W, b, cand, kind, **kw)
    eps = 1e-6
    for name, x in (('dh', h), ('dW', W), ('db', b)):
        num = np.zeros_like(x)
        it = np.nditer(x, flags=['multi_index'])
        for _ in it:
            i = it.multi_index
            keep = x[i]
            x[i] = keep + eps
            up = float(cx.restate(h, W, b, cand, kind, **kw)['loss'])
            x[i] = keep - eps
            dn = float(cx.restate(h, W, b, cand, kind, **kw)['loss'])
            x[i] = keep
            num[i] = (up - dn) / (2 * eps)
        assert float(np.abs(num - r[name]).max()) < 1e-8, name


@pytest.mark.parametrize('kind', cx.KINDS)
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_exact_zeros(kind, dtype):
    """ignored rows, absent entries and a row without a present negative"""
    h, W, b, corr, cand = _small(seed=7)
    V = W.shape[0]
    cand[2, 1:] = [-1, V, -5, V + 1]                              # a valid target and no present negative
    kw = dict(beta=0.37, corr=corr)
    r = cx.restate(h, W, b, cand, kind, dtype=dtype, **kw)
    absent = (cand < 0) | (cand >= V)
    ignored = absent[:, 0]
    assert ignored.sum() == 2 and not r['item'][ignored].any() and not r['g'][ignored].any() and not r['dh'][ignored].any()
    assert not r['g'][absent].any()
    live = ~ignored
    live[2] = False
    assert r['item'][live].all() and r['g'][live, 0].all()
    if kind == 'bce':                                           # the target's own term is all there is
        assert r['item'][2] > 0 and r['g'][2, 0] < 0
    else:                                                       # bpr: the empty sum; softmax: over the target alone
        assert r['item'][2] == 0 and not r['g'][2].any() and not r['dh'][2].any()
    # an absent entry has no term: the row's loss is the loss of the list without it
    r2 = cx.restate(h[:1], W, b, np.delete(cand[:1], 2, axis=1), kind, gscale=float(r['gs']), dtype=dtype, **kw)
    assert r2['item'][0] == r['item'][0] and np.array_equal(r2['dh'][0], r['dh'][0])
    # items no live list names receive nothing
    named = np.unique(cand[~ignored][~absent[~ignored]])
    rest = np.setdiff1d(np.arange(V), named)
    assert not r['dW'][rest].any() and not r['db'][rest].any()
    # one entry: bpr and softmax are exactly 0 whatever the scores, the sinks keep G0
    G0 = (np.random.default_rng(1).standard_normal(W.shape), np.random.default_rng(2).standard_normal(b.shape))
    if kind != 'bce':
        r1 = cx.restate(h * 30, W, b, cand[:, :1], kind, corr=corr, correct_target=True, G0=G0, dtype=dtype)
        assert not r1['item'].any() and not r1['g'].any() and not r1['dh'].any() and float(r1['loss']) == 0.0
        assert np.array_equal(r1['dW'], G0[0].astype(dtype)) and np.array_equal(r1['db'], G0[1].astype(dtype))
        bd = cx.bounds(h * 30, W, b, cx.restate(h * 30, W, b, cand[:, :1], kind, corr=corr, correct_target=True, G0=G0), kind, G0=G0)
        assert not bd['item'].any() and not bd['g'].any() and not bd['dW'].any()


def test_bpr_is_stable_at_scores_of_a_hundred():
    h, W, b, corr, cand = _small(seed=9)
    C = cand.shape[1]
    for dtype in (np.float64, np.float32):
        r = cx.restate(h * 40, W, b, cand, 'bpr', corr=corr, dtype=dtype)
        assert float(np.abs(r['s']).max()) > 100 and np.isfinite(r['item']).all() and np.isfinite(r['dW']).all()
        assert ((r['g'][:, 1:] >= 0) & (r['g'][:, 1:] <= 1)).all() and ((r['g'][:, 0] <= 0) & (r['g'][:, 0] >= -(C - 1))).all()


def test_the_committed_correction():
    for R, C, K, V, scale in cl.CASES:
        cnt, corr = cx.item_counts(V), cx.corr_for(C, V)
        assert corr.dtype == np.float32 and corr.shape == (V,) and np.isfinite(corr).all()
        assert np.array_equal(cx.item_counts(V), cnt) and (cnt >= 0).all() and cnt.any()
        assert not corr[cnt == 0].any()
        if V >= 50:
            assert 0.03 * V <= (cnt == 0).sum() <= 0.2 * V and cnt.max() >= 20 * np.median(cnt[cnt > 0])
    assert cx.SETTINGS == (('bpr', 1.0, False, False), ('bpr', 1.0, True, False), ('bce', 0.37, True, False),
                           ('softmax', 1.0, True, False), ('softmax', 1.0, True, True))


@pytest.fixture(scope='module')
def ratios():
    return {case: cx.measured_ratio([case]) for case in cl.CASES}


@pytest.mark.parametrize('case', cl.CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_measured_ratio_ex_of_a_case(case, ratios):
    """the float32 mode's worst distance from float64, in units of the derived bound, on the inputs and settings of the GPU tests
    (also: where the bound is 0 the float32 mode is exact)"""
    print('measured ratio %s: %.4f' % (case, ratios[case]))
    assert ratios[case] <= cx.MEASURED_RATIO_EX


def test_measured_ratio_ex_is_current(ratios):
    """the committed constant is at least the recomputed worst ratio and within 10 % of it"""
    worst = max(ratios.values())
    print('measured ratio: %.5f, committed %.5f' % (worst, cx.MEASURED_RATIO_EX))
    assert worst <= cx.MEASURED_RATIO_EX <= 1.1 * worst
