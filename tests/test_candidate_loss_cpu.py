"""Sampled-negative training losses over per-row candidate lists, the parts that need no GPU (NO REFERENCE ORACLE: an extension --
the float64 restatement is tests/candidate_loss_ref.py): the entry points' declarations and their binding, the argument checks that refuse
a call before any launch, the restatement against itself, and the head that cannot take the loss."""
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import abi_pin
import candidate_loss_ref as cl

A = 1 << 20                                                       # a well-aligned, never dereferenced "pointer"
NAMES = ('b4c_candidate_loss_fwd', 'b4c_candidate_loss_bwd')


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_they_are_bound():
    from bert4clickpath_amd import _lib, ops
    c = _lib.ctypes
    lib = _lib.lib()
    declared = _lib.signatures()
    ptr, i32, i64 = c.c_void_p, c.c_int, c.c_int64
    lists = {
        # (h, ld_h, table, ld_t, rows, row_off, bias, cand, ld_c, R, C, V, K, dtype, kind, item_loss, g, ld_g, scores, ld_s, stream)
        'b4c_candidate_loss_fwd': [ptr, i32, ptr, i32, i64, i64, ptr, ptr, i32, i64, i32, i32, i32, i32, i32, ptr, ptr, i32, ptr, i32, ptr],
        # (h, ld_h, table, ld_t, rows, row_off, cand, ld_c, g, ld_g, gscale, R, C, V, K, dtype, dh, ld_dh, dtable, ld_dt, dbias, stream)
        'b4c_candidate_loss_bwd': [ptr, i32, ptr, i32, i64, i64, ptr, i32, ptr, i32, ptr, i64, i32, i32, i32, i32, ptr, i32, ptr, i32, ptr,
                                   ptr],
    }
    for name in NAMES:
        assert name in declared, name
        assert declared[name] == (c.c_int, lists[name]), name
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == lists[name] and getattr(lib, name).restype is c.c_int
    consts = _lib.header_constants(_lib._header_text(_lib.HEADER_PATH))
    assert (consts['B4C_CAND_BCE'], consts['B4C_CAND_SOFTMAX'], consts['B4C_CAND_KINDS']) == (0, 1, 2)
    assert (_lib.CAND_BCE, _lib.CAND_SOFTMAX) == (0, 1) and ops.CAND_LOSS_KINDS == {'bce': 0, 'softmax': 1}
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    assert '#ifndef B4C_H' in text and 'extern "C"' in text
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    if cc:              # what a C compiler sees of b4c.h alone
        pre = subprocess.run([cc, '-E', '-dD', _lib.HEADER_PATH], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(r'\bint %s\(' % name, pre), name
        for d in ('B4C_CAND_BCE 0', 'B4C_CAND_SOFTMAX 1', 'B4C_CAND_KINDS 2'):
            assert re.search(r'#define %s\b' % d, pre), d


def test_the_pinned_lists_still_hold():
    from bert4clickpath_amd import _lib
    lib = _lib.lib()
    assert len(_lib.signatures()) == abi_pin.ENTRY_POINTS == len(_lib.declared_symbols())
    assert _lib.ABI_VERSION == abi_pin.ABI_VERSION and lib.b4c_abi_version() == abi_pin.ABI_VERSION


def _fwd(L, h=A, ld_h=128, table=A, ld_t=128, rows=1000, row_off=10, bias=A, cand=A, ld_c=8, R=4, C=8, V=500, K=128, dtype=1, kind=0,
         item=A, g=A, ld_g=8, scores=None, ld_s=0):
    return L.b4c_candidate_loss_fwd(h, ld_h, table, ld_t, rows, row_off, bias, cand, ld_c, R, C, V, K, dtype, kind, item, g, ld_g, scores,
                                    ld_s, None)


def _bwd(L, h=A, ld_h=128, table=A, ld_t=128, rows=1000, row_off=10, cand=A, ld_c=8, g=A, ld_g=8, gscale=A, R=4, C=8, V=500, K=128,
         dtype=1, dh=A, ld_dh=128, dtable=A, ld_dt=128, dbias=A):
    return L.b4c_candidate_loss_bwd(h, ld_h, table, ld_t, rows, row_off, cand, ld_c, g, ld_g, gscale, R, C, V, K, dtype, dh, ld_dh, dtable,
                                    ld_dt, dbias, None)


BAD_BOTH = [dict(h=None), dict(table=None), dict(cand=None), dict(K=0), dict(K=12), dict(K=1032), dict(C=0), dict(C=1025, ld_c=1025, ld_g=1025),
            dict(ld_h=120), dict(ld_t=120), dict(ld_c=7), dict(ld_g=7), dict(h=A + 8), dict(table=A + 4), dict(ld_h=132), dict(ld_t=130),
            dict(dtype=2), dict(dtype=-1), dict(V=0), dict(R=-1), dict(row_off=-1), dict(row_off=501)]
BAD_FWD = [dict(bias=None), dict(item=None), dict(g=None), dict(kind=2), dict(kind=-1), dict(scores=A, ld_s=7)]
BAD_BWD = [dict(g=None), dict(gscale=None), dict(dh=None), dict(dtable=None), dict(dbias=None), dict(ld_dh=120), dict(ld_dt=120),
           dict(dh=A + 8), dict(ld_dh=132)]


def test_bad_arguments_are_refused_without_a_launch():
    """(every call here would fault on its made-up pointers if it were launched, and there is no device to launch on)"""
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    for fn, who, bad in ((_fwd, b'candidate_loss_fwd', BAD_BOTH + BAD_FWD), (_bwd, b'candidate_loss_bwd', BAD_BOTH + BAD_BWD)):
        for kw in bad:
            assert fn(L, **kw) == _lib._C['B4C_EINVAL'], (who, kw)
            assert who in L.b4c_last_error(), (who, kw, L.b4c_last_error())
    assert _fwd(L, kind=2) == -1 and b'kind 2' in L.b4c_last_error()
    assert _bwd(L, dh=A + 8) == -1 and b'16-byte aligned' in L.b4c_last_error()
    # nothing to do is not an error (and launches nothing)
    assert _fwd(L, R=0) == 0 and _bwd(L, R=0) == 0
    # fp32 rows need a pitch that is a multiple of 4 only
    assert _fwd(L, dtype=0, ld_h=132, R=0) == 0 and _fwd(L, dtype=1, ld_h=132, R=0) == -1


def test_host_wrappers_validate_before_the_device_is_needed():
    from bert4clickpath_amd import ops
    h, tab, b = torch.zeros(4, 16), torch.zeros(30, 16), torch.zeros(20)
    cand = torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(ops.B4CError, match="'bce' or 'softmax'"):
        ops.candidate_loss_fwd(h, tab, b, cand, 20, 'bpr')
    with pytest.raises(ops.B4CError, match='multiple of 8'):
        ops.candidate_loss_fwd(torch.zeros(4, 12), tab, b, cand, 20, 'bce')
    with pytest.raises(ops.B4CError, match='fp32 master table'):
        ops.candidate_loss_fwd(h, tab.bfloat16(), b, cand, 20, 'bce')
    with pytest.raises(ops.B4CError, match='rows 11 .. 31'):
        ops.candidate_loss_fwd(h, tab, b, cand, 20, 'bce', row_off=11)
    with pytest.raises(ops.B4CError, match='int32'):
        ops.candidate_loss_fwd(h, tab, b, cand.long(), 20, 'bce')
    with pytest.raises(ops.B4CError, match='HIP device only'):
        ops.candidate_loss_fwd(h, tab, b, cand, 20, 'bce')


def test_plain_softmax_head_names_the_heads_that_work():
    from bert4clickpath_amd import ops
    from bert4clickpath_amd.clickstream_transformer import SoftMaxHead
    head = SoftMaxHead([16], 20, input_dim=16)
    with pytest.raises(ops.B4CError, match='ClozeMaskedItemPrediction or SampledSoftmaxHead'):
        head.candidate_loss(torch.zeros(4, 16), torch.zeros(4, 3, dtype=torch.int32), 'bce')


# ---- the restatement against itself ---------------------------------------------------------------------------------------------
def _small(R=6, C=5, K=8, V=9, seed=0):
    rng = np.random.default_rng(seed)
    h, W, b = rng.standard_normal((R, K)), rng.standard_normal((V, K)) * 0.7, rng.standard_normal(V) * 0.3
    cand = rng.integers(0, V, size=(R, C)).astype(np.int32)
    cand[1, 0] = -1                     # an ignored row
    cand[4, 0] = V + 3                  # another
    cand[0, 2] = -1                     # absent entries in the middle of a list
    cand[2, 1] = V
    cand[3, 3] = cand[3, 1]             # a repeated id
    cand[5, 4] = cand[5, 0]             # the target once more, as a negative
    return h, W, b, cand


def test_softmax_over_the_whole_vocabulary_is_plain_cross_entropy():
    h, W, b, _ = _small()
    R, V = h.shape[0], W.shape[0]
    y = np.array([3, 0, 8, 5, 1, 7])
    cand = np.stack([np.concatenate([[t], np.setdiff1d(np.arange(V), [t])]) for t in y]).astype(np.int32)
    r = cl.restate(h, W, b, cand, 'softmax')
    ht, Wt, bt = [torch.tensor(x, requires_grad=True) for x in (h, W, b)]
    loss = torch.nn.functional.cross_entropy(ht @ Wt.T + bt, torch.tensor(y), reduction='mean')
    loss.backward()
    assert abs(float(loss.detach()) - float(r['loss'])) < 1e-13
    for got, ref in ((r['dh'], ht.grad), (r['dW'], Wt.grad), (r['db'], bt.grad)):
        assert float(np.abs(got - ref.numpy()).max()) < 1e-13


@pytest.mark.parametrize('kind', cl.KINDS)
def test_gradients_match_central_finite_differences(kind):
    h, W, b, cand = _small(seed=3)
    r = cl.restate(h, W, b, cand, kind)
    eps = 1e-6
    for name, x in (('dh', h), ('dW', W), ('db', b)):
        num = np.zeros_like(x)
        it = np.nditer(x, flags=['multi_index'])
        for _ in it:
            i = it.multi_index
            keep = x[i]
            x[i] = keep + eps
            up = float(cl.restate(h, W, b, cand, kind)['loss'])
            x[i] = keep - eps
            dn = float(cl.restate(h, W, b, cand, kind)['loss'])
            x[i] = keep
            num[i] = (up - dn) / (2 * eps)
        assert float(np.abs(num - r[name]).max()) < 1e-8, name


@pytest.mark.parametrize('kind', cl.KINDS)
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_ignored_rows_and_absent_entries_have_exactly_zero_terms(kind, dtype):
    h, W, b, cand = _small(seed=5)
    r = cl.restate(h, W, b, cand, kind, dtype=dtype)
    V = W.shape[0]
    absent = (cand < 0) | (cand >= V)
    ignored = absent[:, 0]
    assert ignored.sum() == 2 and not r['item'][ignored].any() and not r['g'][ignored].any() and not r['dh'][ignored].any()
    assert not r['g'][absent].any() and r['item'][~ignored].all()
    # an absent entry has no term: the row's loss is the loss of the list without it
    r2 = cl.restate(h[:1], W, b, np.delete(cand[:1], 2, axis=1), kind, gscale=float(r['gs']), dtype=dtype)
    assert r2['item'][0] == r['item'][0] and np.array_equal(r2['dh'][0], r['dh'][0])
    # items no live list names receive nothing
    named = np.unique(cand[~ignored][~absent[~ignored]])
    rest = np.setdiff1d(np.arange(V), named)
    assert not r['dW'][rest].any() and not r['db'][rest].any()
    # a repeated id is two terms, not one: dropping the repeat changes the loss
    r3 = cl.restate(h[3:4], W, b, np.delete(cand[3:4], 3, axis=1), kind, dtype=dtype)
    assert r3['item'][0] != r['item'][3]


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_softmax_over_the_target_alone_is_exactly_zero(dtype):
    h, W, b, cand = _small(seed=7)
    G0 = (np.random.default_rng(1).standard_normal(W.shape), np.random.default_rng(2).standard_normal(b.shape))
    r = cl.restate(h * 30, W, b, cand[:, :1], 'softmax', G0=G0, dtype=dtype)
    assert not r['item'].any() and not r['g'].any() and not r['dh'].any() and float(r['loss']) == 0.0
    assert np.array_equal(r['dW'], G0[0].astype(dtype)) and np.array_equal(r['db'], G0[1].astype(dtype))


def test_stable_at_scores_of_a_hundred():
    h, W, b, cand = _small(seed=9)
    for dtype in (np.float64, np.float32):
        r = cl.restate(h * 40, W, b, cand, 'bce', dtype=dtype)
        live = ~((cand[:, 0] < 0) | (cand[:, 0] >= W.shape[0]))
        assert float(np.abs(r['s']).max()) > 100 and np.isfinite(r['item']).all() and np.isfinite(r['dW']).all()
        assert (np.abs(r['g']) <= 1).all() and (r['g'][live, 0] <= 0).all() and (r['g'][:, 1:] >= 0).all()


@pytest.mark.parametrize('case', cl.CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_measured_ratio_is_current(case):
    """the float32 mode's worst distance from float64, in units of the derived bound, on the inputs of the GPU tests: what the gate
    of tests/test_gpu_candidate_loss.py is built from.  (Also: where the bound is 0 the float32 mode is exact.)"""
    ratio = cl.measured_ratio([case])
    print('measured ratio %s: %.4f' % (case, ratio))
    assert ratio <= cl.MEASURED_RATIO
