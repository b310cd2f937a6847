"""The contrastive-loss section of include/b4c.h and its binding, without a GPU: the header says what the issue's lists say; a
name declared twice is refused; the built library exports the two names; include/ holds the one header; every argument the entry
points refuse is refused with NULL pointers (the checks come before any pointer is looked at); N == 0 is B4C_OK.  And the
restatement tests/nce_ref.py: its float32 mode against float64 in units of the derived bound (the number the GPU gate is built
from), and the exact zeros of its bound."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import abi_pin
import nce_ref as nr

V, I, I64, F, U32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint32
FWD = [V, I, I64, I, I, V, V, F, U32, V, V, V, V]
BWD = [V, I, I64, I, I, V, V, F, U32, V, V, V, V, I, V]


@pytest.fixture(scope='module')
def L():
    from bert4clickpath_amd import _lib
    return _lib


NAMES = {'b4c_nce_fwd', 'b4c_nce_bwd'}


def test_header_parses_and_matches_the_declared_lists(L):
    sig = L.signatures()
    assert sig['b4c_nce_fwd'] == (I, FWD) and sig['b4c_nce_bwd'] == (I, BWD)
    const = L.header_constants(L._header_text(L.HEADER_PATH))
    assert const['B4C_NCE_COSINE'] == 1 == L.NCE_COSINE and const['B4C_NCE_MAX_N'] == 1 << 24 == L.NCE_MAX_N


def test_one_header_declares_the_family(L):
    sig = L.signatures()
    assert len(sig) == abi_pin.ENTRY_POINTS and L.ABI_VERSION == abi_pin.ABI_VERSION
    assert os.listdir(os.path.dirname(L.HEADER_PATH)) == ['b4c.h']
    assert NAMES <= set(sig)
    assert L.declared_symbols() == sorted(sig)


def test_a_name_declared_twice_is_refused(L):
    with pytest.raises(L.B4CError, match=r'declares b4c_nce_fwd twice'):
        L.parse_header(L._header_text(L.HEADER_PATH) + '\nint b4c_nce_fwd(const void *z, int ld_z);\n')


def test_the_built_library_exports_the_family(L):
    nm = shutil.which('nm')
    if nm:
        out = subprocess.run([nm, '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    else:
        lib = ctypes.CDLL(L.LIB_PATH)
        exported = {n for n in NAMES if hasattr(lib, n)}
    assert NAMES <= exported, sorted(NAMES - exported)


def test_a_library_without_a_declared_name_is_refused(L, tmp_path, monkeypatch):
    """lib() raises its usual error for a name the .so lacks: here a header that declares one more name than the library has"""
    more = tmp_path / 'b4c_more.h'
    with open(L.HEADER_PATH) as f:
        more.write_text(f.read() + '\nint b4c_nce_not_there(int n);\n')
    monkeypatch.setattr(L, 'HEADER_PATH', str(more))
    monkeypatch.setattr(L, '_lib', None)
    with pytest.raises(L.B4CError, match=r'does not export b4c_nce_not_there; rebuild it'):
        L.lib()


GOOD = dict(N=5, K=64, dtype=1, inv_temp=1.0, flags=0)
BAD = [('K', dict(K=0)), ('K', dict(K=4)), ('K', dict(K=60)), ('K', dict(K=136)), ('dtype', dict(dtype=2)), ('dtype', dict(dtype=-1)),
       ('inv_temp', dict(inv_temp=0.0)), ('inv_temp', dict(inv_temp=-1.0)), ('inv_temp', dict(inv_temp=float('inf'))),
       ('inv_temp', dict(inv_temp=float('nan'))), ('flags', dict(flags=2)), ('flags', dict(flags=0x80000001)),
       ('rnorm', dict(flags=1)), ('N', dict(N=1 << 24)), ('N', dict(N=-1))]


def _call(lib, which, a):
    if which == 'fwd':
        return lib.b4c_nce_fwd(None, 0, a['N'], a['K'], a['dtype'], None, None, a['inv_temp'], a['flags'], None, None, None, None)
    return lib.b4c_nce_bwd(None, 0, a['N'], a['K'], a['dtype'], None, None, a['inv_temp'], a['flags'], None, None, None, None, 0, None)


@pytest.mark.parametrize('which', ['fwd', 'bwd'])
@pytest.mark.parametrize('name,change', BAD, ids=['%s-%s' % (n, list(c.values())[0]) for n, c in BAD])
def test_bad_arguments_are_refused_before_any_pointer_is_looked_at(L, which, name, change):
    lib = L.lib()
    rc = _call(lib, which, dict(GOOD, **change))
    msg = lib.b4c_last_error().decode()
    assert rc == L._C['B4C_EINVAL'], (rc, msg)
    assert msg.startswith('nce_%s:' % which) and name in msg, msg


@pytest.mark.parametrize('which', ['fwd', 'bwd'])
def test_no_rows_is_ok(L, which):
    assert _call(L.lib(), which, dict(GOOD, N=0)) == 0
    assert _call(L.lib(), which, dict(GOOD, N=0, flags=1)) == 0


def test_null_pointers_with_good_scalars_are_refused(L):
    lib = L.lib()
    for which in ('fwd', 'bwd'):
        assert _call(lib, which, GOOD) == L._C['B4C_EINVAL']
        assert 'null pointer' in lib.b4c_last_error().decode()


@pytest.mark.parametrize('case', nr.CASES, ids=nr.case_id)
def test_measured_ratio_is_current(case):
    """the float32 mode's worst distance from float64, in units of the derived bound, on the inputs of the GPU tests: what the gate
    of tests/test_gpu_nce.py is built from.  (Also: where the bound is 0 the float32 mode is exact.)"""
    ratio = nr.measured_ratio([case])
    print('measured ratio %s: %.4f' % (case, ratio))
    assert ratio <= nr.MEASURED_RATIO


def test_only_positive_keys_have_a_zero_bound():
    """N = 2 and the all-one-group batch: every live row's only key is its positive -- item_loss and dz are 0 with a bound of 0"""
    for case in nr.CASES:
        N, K, pad, pattern, gkind, sim, temp = case
        if not (N == 2 or gkind == 'same'):
            continue
        zf, pos, group = nr.inputs(case, False)
        ref = nr.restate(zf[:, :K], pos, group, nr.inv_temp(temp), sim == 'cos')
        bd = nr.bounds(zf[:, :K], ref, nr.inv_temp(temp), sim == 'cos')
        assert (ref['key'].sum(1) == ref['live']).all()
        assert not ref['item'].any() and not bd['item'].any()
        assert not ref['dz'].any() and not bd['dz'].any()
        assert (bd['lse'][ref['live']] > 0).all()


def test_restatement_against_torch_autograd():
    """dz of the restatement is the gradient of its own loss: torch autograd over a dense float64 evaluation of the definition"""
    import torch
    for case in (nr.CASES[2], nr.CASES[5], nr.CASES[9]):
        N, K, pad, pattern, gkind, sim, temp = case
        zf, pos, group = nr.inputs(case, False)
        ref = nr.restate(zf[:, :K], pos, group, nr.inv_temp(temp), sim == 'cos')
        z = torch.tensor(zf[:, :K], dtype=torch.float64, requires_grad=True)
        loss = nr.dense_loss(z, pos, group, nr.inv_temp(temp), sim == 'cos')
        loss.backward()
        assert abs(float(loss.detach()) - float(ref['loss'])) < 1e-12 * max(1.0, abs(float(ref['loss'])))
        np.testing.assert_allclose(z.grad.numpy(), ref['dz'], rtol=1e-9, atol=1e-12)
