"""The split plan of every committed weight-gradient case (tests/tn_cases.py), asked of the library without a GPU.

tests/test_gpu_weight_grad.py covers the forms of the TN family (one split / narrow / wide reduction / several trips of the split loop,
linear and XCD tile order of the grouped launch) only as long as its cases land in them.  The split count is not an argument of any
entry point: it follows from M and the tile count by tn_plan / tn_group_plan.  Here it is read back from the workspace sizes the
library reports, and every case must be in the class it is listed for; every class must stay populated."""
import pytest

import tn_cases as T


@pytest.fixture(scope='module')
def L():
    from bert4clickpath_amd import _lib
    _lib.lib()
    return _lib


@pytest.mark.parametrize('case', T.SINGLE, ids=T.case_id)
def test_single_case_is_in_its_class(L, case):
    M, K, N, dtype, _, klass, why = case
    ns = T.single_nsplit(L, M, K, N, dtype)
    assert T.split_class(ns) == klass, '%s: %d splits, listed for %r (%s)' % (T.case_id(case), ns, klass, why)
    tk, tn = T.single_tiles(K, N)
    if tk * tn >= 192:
        assert ns == 1


@pytest.mark.parametrize('case', T.GROUP, ids=T.group_id)
def test_group_case_is_in_its_class(L, case):
    M, probs, klass, order, why = case
    ns = T.group_nsplit(L, M, probs)
    assert T.split_class(ns) == klass, '%s: %d splits, listed for %r (%s)' % (T.group_id(case), ns, klass, why)
    assert ('swizzled' if ns % 8 == 0 else 'linear') == order, (ns, order, why)


def test_every_class_is_populated(L):
    single = {(dt, T.split_class(T.single_nsplit(L, M, K, N, dt))) for M, K, N, dt, _, _, _ in T.SINGLE}
    assert single == {(dt, k) for dt in ('bf16', 'f32') for k in T.CLASSES}
    # the segmented cases: one split, narrow and wide in both types
    seg = {(dt, T.split_class(T.single_nsplit(L, M, K, N, dt))) for M, K, N, dt, _, _, _ in T.SINGLE if N in T.SEGMENTS}
    assert seg >= {('f32', 'one'), ('f32', 'narrow'), ('f32', 'wide'), ('bf16', 'narrow'), ('bf16', 'wide')}
    group = {(T.split_class(ns), ns % 8 == 0) for ns in (T.group_nsplit(L, c[0], c[1]) for c in T.GROUP)}
    assert group == {('one', False), ('narrow', False), ('narrow', True), ('wide', True)}
    # the named plans: 65 splits put exactly one element into the second trip of the 64-partition loop; the fallback leaves 7
    assert T.single_nsplit(L, 16448, 128, 128, 'bf16') == 65
    assert T.group_nsplit(L, 2049, T.GROUP[3][1]) == 7
    assert max(T.group_tiles(c[1]) for c in T.GROUP) > 8 and max(len(c[1]) for c in T.GROUP) == 8
    # the real-valued cases are committed cases
    shapes = {c[:4] for c in T.SINGLE}
    assert all(c in shapes for c in T.REAL) and T.GROUP_REAL in T.GROUP


def test_group_refuses_a_db_missing_beside_db0(L):
    """b4c_gemm_tn_group looks at db[0] alone to decide whether a problem has column sums (as b4c_gemm_tn_seg): a later segment
    without a db beside a db[0] would be written through a NULL pointer, so it is refused before any launch.  (No GPU is touched:
    the pointers are never followed.)"""
    probs = [(104, 312, 3)]
    descs = T.group_descs(L, probs)
    d = descs[0]
    d.A, d.G, d.lda, d.ldg, d.ldw = 0x10000, 0x20000, 104, 312, 104
    for i in range(3):
        d.dW[i] = 0x30000 + 0x10000 * i
        d.db[i] = 0x80000 + 0x1000 * i
    d.db[2] = None
    need = int(L.lib().b4c_gemm_tn_group_workspace_bytes(descs, 1, 1000))
    rc = L.lib().b4c_gemm_tn_group(descs, 1, 1000, L.BF16, 0x100000, need, None)
    assert rc != 0 and 'no db beside' in L.lib().b4c_last_error().decode()
    d.dW[1] = None                       # (a missing dW was refused before, and still is)
    d.db[2] = 0x82000
    assert L.lib().b4c_gemm_tn_group(descs, 1, 1000, L.BF16, 0x100000, need, None) != 0
