"""Static check of the hand-counted vector-memory waits of the GELU feed-forward kernels (csrc/ffn_act_fwd.hip, ffn_act_bwd.hip),
with the checker of tests/test_vmcnt_accounting.py (read its docstring first): CPU test, compiles to gfx950 assembly.

The table, from the source comments (N: the count of the wait, m: the awaited request is the m-th LDS-DMA request back, after: the
checked waits every execution passes first):
  ffn_act_fwd   the body is ffn_fwd.hip's (ffn_fwd_body.h), with the tags it carries there.  "x(t) landed -- its DMA went out in
                iteration t - 3": the DMAs of x(t + 2), x(t + 1), x(t) -> m = 3.  The u store of a training call only adds to
                what is issued behind it; the fewest are the inference call's (U == NULL) 7 > 6.  The first three iterations:
                vmcnt(1).  One kernel per activation (erf, tanh).
  ffn_act_bwd   a fetch is three requests, h | x | u.  steady: tile t's three row requests went out in iteration t - 1, then
                [3 DMA of h | x | u (t + 2)] [dX store of t - 2]: the youngest row request is the 4th DMA back, m = 4, N = 4.
                t == 1: no store yet, N = 3.  The compiler unrolls the even and the odd tile: two copies of the steady wait.
"""
import re

import pytest

from test_vmcnt_accounting import DRAINED, check_asm, compile_asm
import test_vmcnt_accounting as va

FILES = ('ffn_act_fwd', 'ffn_act_bwd')
ACTS = (2, 3)                       # B4C_ACT_GELU, B4C_ACT_GELU_TANH
FWD = '_Z18ffn_act_fwd_kernelILi{}EEv13FfnFwdActArgs'
BWD = '_Z18ffn_act_bwd_kernelILi{}EEv13FfnActBwdArgs'


def _table():
    t = {}
    for act in ACTS:
        t[('ffn_act_fwd', FWD.format(act), 'ffn_fwd.first', 0)] = (1, 3, 0)
        t[('ffn_act_fwd', FWD.format(act), 'ffn_fwd.first', 1)] = (1, 3, 0)
        t[('ffn_act_fwd', FWD.format(act), 'ffn_fwd.steady', 0)] = (6, 3, 3)
        t[('ffn_act_bwd', BWD.format(act), 'ffn_act_bwd.second', 0)] = (3, 4, 0)
        t[('ffn_act_bwd', BWD.format(act), 'ffn_act_bwd.steady', 0)] = (4, 4, 1)
        t[('ffn_act_bwd', BWD.format(act), 'ffn_act_bwd.steady', 1)] = (4, 4, 1)
    return t


TABLE = _table()


@pytest.fixture(scope='module')
def asm(tmp_path_factory):
    return compile_asm(tmp_path_factory.mktemp('vmcnt_ffn_act'), files=FILES)


def test_hand_counted_waits_of_the_gelu_kernels(asm):
    failures, report = check_asm(asm, TABLE)
    assert not failures, '\n'.join(failures)
    assert set(report) == set(TABLE)
    for key, (n, cnt) in sorted(report.items()):
        print(key[0], key[1], key[2], key[3], 'vmcnt(%d)' % n, 'fewest issued behind the awaited request:', cnt)
        assert cnt == DRAINED or cnt >= n, (key, n, cnt)


def test_every_hand_written_wait_is_tagged(asm):
    """(check_asm fails on an untagged one; this names them) and the kernels use no scratch, the forward fits two workgroups per CU"""
    for f in FILES:
        text = open(asm[f]).read()
        kernels = va.parse_kernels(text)
        for act in ACTS:
            k = kernels[(FWD if f == 'ffn_act_fwd' else BWD).format(act)]
            waits = va.hand_waits(k)
            assert waits and all(x.tag for _, _, x in waits), [(x.line, x.text) for _, _, x in waits if not x.tag]
        assert re.findall(r'; ScratchSize: (\d+)', text) == ['0', '0'], f
        vgprs = [int(v) for v in re.findall(r'; NumVgprs: (\d+)', text)]
        assert len(vgprs) == 2 and max(vgprs) <= (128 if f == 'ffn_act_fwd' else 256), (f, vgprs)


def _min_path_store(path, kernel, tag, copy):
    """line number (1-based) of the last store on the path that sets the minimum count of a wait"""
    k = va.parse_kernels(open(path).read())[kernel]
    b, i, _ = [w for w in va.hand_waits(k) if w[2].tag == tag][copy]
    n, m, after = TABLE[('ffn_act_bwd', kernel, tag, copy)]
    lines = open(path).read().splitlines()
    stores = [ln for ln in va.min_path_lines(k, b, i, m, after) if va._STORE.match(lines[ln - 1].split()[0])]
    assert stores, (kernel, tag)
    return stores[-1]


@pytest.mark.parametrize('act', ACTS)
def test_checker_catches_a_removed_store(asm, tmp_path, act):
    """ffn_act_bwd's steady vmcnt(4) counts the dX store of tile t - 2: without it only the 3 DMA of tile t + 2 follow the awaited
    request"""
    kernel = BWD.format(act)
    ln = _min_path_store(asm['ffn_act_bwd'], kernel, 'ffn_act_bwd.steady', 0)
    lines = open(asm['ffn_act_bwd']).read().splitlines(keepends=True)
    assert 'global_store' in lines[ln - 1]
    del lines[ln - 1]
    p = tmp_path / 'ffn_act_bwd.s'
    p.write_text(''.join(lines))
    table = {k: v for k, v in TABLE.items() if k[0] == 'ffn_act_bwd'}
    fails = check_asm({'ffn_act_bwd': str(p)}, table)[0]
    assert any(kernel in s and 'ffn_act_bwd.steady' in s and 'vmcnt(4) but only 3' in s for s in fails), fails
