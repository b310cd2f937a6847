"""Static check of the hand-counted vector-memory waits of the four persistent kernels (CPU test: compiles to gfx950 assembly).

The kernels in csrc/ffn_fwd.hip, ffn_bwd.hip, attn_out_bwd.hip and gemm_dxdw.hip move their tiles into LDS with LDS-DMA requests
written in inline assembly.  The compiler cannot see those requests, so the wait that orders a tile's arrival before its first
ds_read is written by hand: `s_waitcnt vmcnt(N)`, N = the vector-memory operations issued AFTER the one waited for.  A ds_read
that runs ahead of its DMA reads the OLD LDS bytes -- no fault, no stall, a stale row now and then.  N is derived in a source
comment from the order in which the compiler is expected to issue the vector-memory instructions; this test reads the order the
compiler actually emitted.

For every hand-written wait (an `s_waitcnt vmcnt(N > 0)` between ;;#ASMSTART and ;;#ASMEND, tagged `; vmcheck <name>` in its
source) the table below gives m: the awaited request is the m-th LDS-DMA request met walking backwards from the wait.  On every
backward path through the kernel's control-flow graph (loop back edges included) at least N counted instructions must lie between
that request and the wait.  The compiler's own waits ignore the unseen requests and can only wait longer: they are not checked,
and a compiler wait of vmcnt(k > 0) met on a path is not taken as a guarantee (stricter).  A vmcnt(0) met first ends the path:
everything older has landed.

Counted: vector global_ / buffer_ / flat_ / scratch_ loads, stores and atomics (gfx9 counts stores in vmcnt too); anything else is
not counted, which can only make the check stricter.

Paths that cannot run are left out, each by a rule the code below spells out:
- an edge taken only when exec is empty (s_cbranch_execz taken, s_cbranch_execnz falling through) where exec is provably the whole
  wave (the kernels launch whole waves);
- the same edge around a block of stores only, when the mask is the kernels' int64 row guard `row < M`: every row of a wave lies
  past M only in the last tile of the last workgroup, after which no checked wait runs;
- a path whose branches contradict one another (the compiler tests one source condition several times);
- a path on which fewer checked waits precede this one than every execution passes (`after` in the table): the first iterations,
  which the source sends through the first-iteration waits, checked by their own entries.
"""
import os
import re
import shutil
import subprocess
from collections import defaultdict
from functools import lru_cache
from heapq import heappop, heappush

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bert4clickpath_amd', 'csrc')
FILES = ('ffn_fwd', 'ffn_bwd', 'attn_out_bwd', 'gemm_dxdw')

# One entry per hand-counted wait: (file, kernel symbol, tag, copy) -> (N, m, after).  `copy` numbers the copies of one source wait in
# the order the compiler lays them out (unrolled tiles, template instances).  N and m from the source comments:
# `after`: the checked waits every execution passes before this one (the first iterations take those).
#   ffn_fwd   "x(t) landed -- its DMA went out in iteration t - 3": the DMAs of x(t + 2), x(t + 1), x(t) -> m = 3.  Issued after
#             it (inference, the fewest): h(t - 3), out(t - 3), x(t + 1), h(t - 2), out(t - 2), x(t + 2), h(t - 1) = 7 > 6.  The
#             first three iterations: vmcnt(1), x(t) with x(t + 1) .. behind it.
#   ffn_bwd   steady: tile t's three row requests went out in iteration t - 1, then [2 DMA of h | x (t + 2)] [dX store of t - 2]:
#             the youngest row request is the 3rd DMA back, m = 3, N = 3.  t == 1: no store yet, N = 2.
#   attn_out_bwd  steady: [3 row requests of t] [dz store of t - 1] [d_o store of t - 2] [1 DMA of o(t + 2)]: m = 2, N = 3.  t == 1:
#             [dz store of 0] [DMA of o(3)], N = 2.
#   gemm_dxdw every wait awaits the operation issued right before its N younger LDS-DMA requests: m = N + 1.
#             prologue: tiles 1 and 2 behind tile 0 (N = 2 ND, ND = 1 + NG requests per tile); steady: tile t + 3's ND requests
#             behind tile t - 1's residual chunk (or tile t + 2's last request), N = ND; the first tile's closing wait: tiles 2, 3
#             and the residual chunk behind tile 1, N = 2 ND + (residual).
FFN_FWD = '_Z14ffn_fwd_kernel10FfnFwdArgs'
FFN_BWD = '_Z14ffn_bwd_kernel10FfnBwdArgs'
AO_BWD = '_Z13ao_bwd_kernel9AoBwdArgs'
DXDW = '_Z16gemm_dxdw_kernelILi{}EEv8DxDwArgs'


def _table():
    t = {}
    t[('ffn_fwd', FFN_FWD, 'ffn_fwd.first', 0)] = (1, 3, 0)
    t[('ffn_fwd', FFN_FWD, 'ffn_fwd.first', 1)] = (1, 3, 0)
    t[('ffn_fwd', FFN_FWD, 'ffn_fwd.steady', 0)] = (6, 3, 3)
    t[('ffn_bwd', FFN_BWD, 'ffn_bwd.second', 0)] = (2, 3, 0)
    t[('ffn_bwd', FFN_BWD, 'ffn_bwd.steady', 0)] = (3, 3, 1)
    t[('ffn_bwd', FFN_BWD, 'ffn_bwd.steady', 1)] = (3, 3, 1)
    t[('attn_out_bwd', AO_BWD, 'attn_out_bwd.second', 0)] = (2, 2, 0)
    t[('attn_out_bwd', AO_BWD, 'attn_out_bwd.steady', 0)] = (3, 2, 1)
    # gemm_dxdw<NG>: copies of the steady wait (one per unrolled tile the compiler kept)
    for ng, steady_copies in ((3, 4), (2, 4), (1, 7)):
        nd = 1 + ng
        k = DXDW.format(ng)
        t[('gemm_dxdw', k, 'dxdw.prologue', 0)] = (2 * nd, 2 * nd + 1, 0)
        for c in range(steady_copies):
            t[('gemm_dxdw', k, 'dxdw.steady', c)] = (nd, nd + 1, 2)
        # DD_WAIT_VM(2 ND + residual): the with-residual and the without-residual case, in layout order
        for c, n in enumerate((2 * nd + 1, 2 * nd)):
            t[('gemm_dxdw', k, 'dxdw.first', c)] = (n, n + 1, 1)
    return t


TABLE = _table()

# ---------------------------------------------------------------------------------------------------------------------------------
# compile


def _hipcc():
    for p in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if p and os.path.isfile(p) and os.access(p, os.X_OK):
            return p
    return None


def _makefile_cxxflags():
    """CXXFLAGS of csrc/Makefile with its variables substituted (ARCH from the Makefile, EXTRA empty)."""
    text = open(os.path.join(CSRC, 'Makefile')).read()
    arch = re.search(r'^ARCH\s*\?=\s*(\S+)', text, re.M).group(1)
    flags = re.search(r'^CXXFLAGS\s*=\s*(.*)$', text, re.M).group(1)
    flags = flags.replace('$(ARCH)', arch).replace('$(EXTRA)', '')
    assert '$(' not in flags, flags
    return flags.split()


def compile_asm(outdir, files=FILES, src_dir=CSRC):
    """-> {file: path of its gfx950 device assembly}; compile errors fail the caller."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip('hipcc not found')
    flags = _makefile_cxxflags()
    procs = {}
    for f in files:
        out = os.path.join(str(outdir), f + '.s')
        procs[f] = (out, subprocess.Popen([hipcc] + flags + ['--cuda-device-only', '-S', os.path.join(src_dir, f + '.hip'), '-o', out],
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=src_dir))
    res = {}
    for f, (out, p) in procs.items():
        log = p.communicate()[0].decode(errors='replace')
        assert p.returncode == 0, f'{f}.hip failed to compile:\n{log}'
        res[f] = out
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# parse

_VM_PREFIX = re.compile(r'^(global|buffer|flat|scratch)_(load|store|atomic)')
_STORE = re.compile(r'^(global|buffer|flat|scratch)_store')
_WAIT_VM = re.compile(r'\bvmcnt\((\d+)\)')
_TAG = re.compile(r'vmcheck\s+(\S+)')
_LABEL = re.compile(r'^(\.LBB\w+):')


class Ins:
    __slots__ = ('line', 'text', 'op', 'args', 'in_asm', 'tag', 'w')

    def __init__(self, line, text, in_asm, tag):
        self.line, self.text, self.in_asm, self.tag = line, text, in_asm, tag
        self.w = None
        parts = text.split(None, 1)
        self.op = parts[0]
        self.args = parts[1] if len(parts) > 1 else ''

    @property
    def counted(self):
        return bool(_VM_PREFIX.match(self.op))

    @property
    def dma(self):
        return self.counted and '_load' in self.op and re.search(r'\blds\b', self.args) is not None

    @property
    def store(self):
        return bool(_STORE.match(self.op))

    @property
    def vm_wait(self):
        if self.op != 's_waitcnt':
            return None
        m = _WAIT_VM.search(self.args)
        return int(m.group(1)) if m else None


class Kernel:
    def __init__(self, name):
        self.name = name
        self.blocks = []            # [(label or None, [Ins])]
        self.succ = {}              # block -> [(block, dead_wave)]
        self.pred = defaultdict(list)


def parse_kernels(asm_text):
    """-> {symbol: Kernel} for every function in one assembly file."""
    kernels = {}
    cur = None
    in_asm = False
    for ln, raw in enumerate(asm_text.splitlines(), 1):
        s = raw.strip()
        if cur is None:
            m = re.match(r'^([A-Za-z_][\w.$]*):\s*;\s*@', raw)
            if m:
                cur = Kernel(m.group(1))
                kernels[cur.name] = cur
                cur.blocks.append((None, []))
            continue
        if s.startswith('.Lfunc_end'):
            _link(cur)
            cur = None
            continue
        if s.startswith(';;#ASMSTART'):
            in_asm = True
            continue
        if s.startswith(';;#ASMEND'):
            in_asm = False
            continue
        m = _LABEL.match(s)
        if m:
            cur.blocks.append((m.group(1), []))
            continue
        code, _, comment = s.partition(';')
        code = code.strip()
        if not code or code.startswith('.'):
            continue
        tm = _TAG.search(comment)
        ins = Ins(ln, code, in_asm, tm.group(1) if tm else None)
        if cur.blocks[-1][1] and _ends_block(cur.blocks[-1][1][-1]):
            cur.blocks.append((None, []))
        cur.blocks[-1][1].append(ins)
    return kernels


def _ends_block(ins):
    return ins.op == 's_branch' or ins.op.startswith('s_cbranch_') or ins.op == 's_endpgm'


def _link(k):
    index = {lab: i for i, (lab, _) in enumerate(k.blocks) if lab}
    for i, (_, ins) in enumerate(k.blocks):
        last = ins[-1] if ins else None
        out = []
        if last is not None and last.op in ('s_setpc_b64', 's_swappc_b64', 's_cbranch_g_fork', 's_cbranch_join'):
            raise AssertionError(f'{k.name}: control flow the checker does not model: line {last.line}: {last.text}')
        if last is not None and last.op == 's_endpgm':
            pass
        elif last is not None and last.op == 's_branch':
            out.append((index[last.args.split()[0]], False))
        elif last is not None and last.op.startswith('s_cbranch_'):
            tgt = index[last.args.split()[0]]
            if i + 1 < len(k.blocks):
                dead = last.op == 's_cbranch_execnz' and tgt > i and _row_guard(ins) and _no_request(k.blocks[tgt][1])
                out.append((i + 1, dead))
            dead = last.op == 's_cbranch_execz' and i + 1 < len(k.blocks) and _row_guard(ins) and _no_request(k.blocks[i + 1][1])
            out.append((tgt, dead))
        elif i + 1 < len(k.blocks):
            out.append((i + 1, False))
        k.succ[i] = out
    full = _exec_full_at_branch(k)
    for i, out in k.succ.items():
        ins = k.blocks[i][1]
        last = ins[-1] if ins else None
        if last is not None and full.get(i) and last.op in ('s_cbranch_execz', 's_cbranch_execnz'):
            # exec is the whole wave here: its empty-exec edge is never taken
            tgt = [j for j, _ in out if k.blocks[j][0] == last.args.split()[0]][0]
            out = [(j, True if ((last.op == 's_cbranch_execz' and j == tgt) or (last.op == 's_cbranch_execnz' and j == i + 1 and j != tgt))
                    else d) for j, d in out]
            k.succ[i] = out
        for j, dead in k.succ[i]:
            k.pred[j].append((i, dead))


def _exec_full_at_branch(k):
    """-> {block: exec is the whole launch mask at the block's end} (forward dataflow; the kernels launch whole waves).
    s_and_saveexec_b64 sX saves the mask it narrows; s_or_b64 exec, exec, sX puts the saved one back; any other write of exec
    narrows it as far as this analysis knows."""
    FULL, NARROW = 'full', 'narrow'

    def step(state, snaps, x):
        ops = [t.strip() for t in x.args.split(',')] if x.args else []
        if x.op == 's_and_saveexec_b64':
            snaps = {r: v for r, v in snaps.items() if r != ops[0]}
            snaps[ops[0]] = state
            return NARROW, snaps
        if x.op == 's_or_b64' and ops[:2] == ['exec', 'exec'] and len(ops) == 3:
            return snaps.get(ops[2], NARROW), snaps
        if x.op.startswith('s_cbranch'):
            return state, snaps
        if 'exec' in x.op or (ops and ops[0] in ('exec', 'exec_lo', 'exec_hi')):
            return NARROW, {r: v for r, v in snaps.items() if not ops or r != ops[0]}
        if ops and ops[0] in snaps:
            snaps = {r: v for r, v in snaps.items() if r != ops[0]}
        return state, snaps

    at_in = {0: (FULL, {})}
    at_out = {}
    work = [0]
    while work:
        b = work.pop()
        state, snaps = at_in[b]
        for x in k.blocks[b][1]:
            state, snaps = step(state, dict(snaps), x)
        at_out[b] = state
        for j, _ in k.succ.get(b, []):
            old = at_in.get(j)
            if old is None:
                new = (state, snaps)
            else:
                new = (old[0] if old[0] == state else NARROW, {r: v for r, v in old[1].items() if snaps.get(r) == v})
            if new != old:
                at_in[j] = new
                work.append(j)
    return {b: st == FULL for b, st in at_out.items()}


def _row_guard(ins):
    """the block's branch tests an exec mask that `s_and_saveexec_b64` made from a 64-bit signed compare (the kernels' int64
    `row < M`), alone or AND-ed with a lane mask made before the block (the column test `opart * 8 < Fp` of ffn_fwd's h store,
    which the first 8-column piece of every row passes).  Not a mask that a uniform condition can empty (a null pointer: ffn_fwd's
    statistics store narrows exec with `s_and_b64 exec, exec, ...` and keeps its edge)."""
    def made_by_row_compare(mask, j):
        for i in range(j - 1, -1, -1):
            y = ins[i]
            ops = [t.strip() for t in y.args.split(',')] if y.args else []
            if mask == 'vcc' and y.op.startswith('v_cmp') and y.op.endswith('_e32') or ops[:1] == [mask]:
                if re.match(r'^v_cmp_(lt|le|gt|ge)_i64', y.op):
                    return True
                if y.op == 's_and_b64' and len(ops) == 3 and 'exec' not in ops:
                    return made_by_row_compare(ops[1], i) or made_by_row_compare(ops[2], i)
                return False
        return False
    for j in range(len(ins) - 2, -1, -1):
        x = ins[j]
        if x.op == 's_and_saveexec_b64':
            return made_by_row_compare(x.args.split(',')[1].strip(), j)
        if 'exec' in x.op or x.args.split(',')[0].strip() == 'exec':
            return False
    return False


def _no_request(ins):
    """the block issues no vector-memory load (LDS-DMA or other): at most stores"""
    return all(x.store for x in ins if x.counted)


# ---------------------------------------------------------------------------------------------------------------------------------
# check


def hand_waits(k):
    """-> [(block, index, Ins)] of the hand-written waits vmcnt(N > 0), in layout order"""
    out = []
    for b, (_, ins) in enumerate(k.blocks):
        for i, x in enumerate(ins):
            n = x.vm_wait
            if x.in_asm and n is not None and n > 0:
                out.append((b, i, x))
    return out



# ---- which paths can run --------------------------------------------------------------------------------------------------
# The compiler splits one source condition into several branches (`if (body)` of a tile tested again around other code, the loop's
# exit test a few blocks later) and tests them on recomputed copies of the flag.  A path that takes contradicting sides cannot
# run: the walk carries what the branches it took say about the registers, rewritten backwards through the instructions that
# compute them (weakest precondition), and drops a path once two facts contradict.  Understood: copies and constant adds of 64-bit
# scalar pairs, 64-bit signed compares (and equality) of pairs and constants, `s_and_b64 vcc, exec, s[..]` and its andn2 form,
# s_cselect_b64 -1 / 0, v_cndmask 0 / 1 of a flag and its compare with 1.  Any other write to a register a fact names forgets
# the fact -- more paths, a stricter check.  Facts: ('b', reg, bool) and ('r', a, b, cc, c): a - b cc c (a, b: pairs or '0').
# (s_cbranch_vcc(n)z is the compiler's uniform branch: the flags and compared values it tests hold one value for the whole wave.)
# This is load-bearing, not an optimisation: without it the walk reports waits the source gets right as broken -- on today's
# assembly ffn_fwd.steady (5 < 6), both copies of ffn_bwd.steady (2 < 3) and attn_out_bwd.steady (2 < 3), each over a path that
# takes `if (body)` on one side and then the other.  A change here that drops paths wrongly shows as a wait no path reaches
# (check_asm fails on it), or as a smaller count in the mutation tests below.

_REG = re.compile(r'^([sv])\[(\d+):(\d+)\]$|^([sv])(\d+)$')
_FLIP = {'lt': 'gt', 'gt': 'lt', 'le': 'ge', 'ge': 'le', 'eq': 'eq', 'ne': 'ne'}
_NEG = {'lt': 'ge', 'ge': 'lt', 'gt': 'le', 'le': 'gt', 'eq': 'ne', 'ne': 'eq'}
_NO_SCC = ('s_mov', 's_cselect', 's_movk', 's_cmov', 's_cbranch', 's_branch', 's_waitcnt', 's_barrier', 's_nop', 's_endpgm',
           's_setprio', 's_sleep', 's_getpc', 's_load', 's_buffer_load')


@lru_cache(maxsize=None)
def _units(tok):
    if tok in ('vcc', 'vcc_lo', 'vcc_hi'):
        return frozenset(('vcc',))
    if tok in ('exec', 'exec_lo', 'exec_hi', 'scc', 'm0'):
        return frozenset((tok.split('_')[0],))
    m = _REG.match(tok)
    if not m:
        return frozenset()
    if m.group(1):
        return frozenset(f'{m.group(1)}{r}' for r in range(int(m.group(2)), int(m.group(3)) + 1))
    return frozenset((f'{m.group(4)}{m.group(5)}',))


def _operands(x):
    return [t.strip() for t in x.args.split(',')] if x.args else []


def _written(x):
    if x.w is None:
        x.w = _written_now(x)
    return x.w


def _written_now(x):
    op, ops = x.op, _operands(x)
    if op.startswith(('s_cmp', 's_bitcmp')):
        return frozenset(('scc',))
    if op.startswith(('s_cbranch', 's_branch', 's_waitcnt', 's_barrier', 's_nop', 's_endpgm', 's_setprio', 's_sleep')) or \
            _STORE.match(op) or op.startswith('ds_write') or x.dma:
        return frozenset()
    w = set(_units(ops[0])) if ops else set()
    if len(ops) > 1 and op.startswith('v_') and ('_co_' in op or 'addc' in op or 'subb' in op):
        w |= _units(ops[1])
    if 'exec' in op:
        w.add('exec')
    if op.startswith('v_') and op.endswith('_e32') and (op.startswith('v_cmp') or '_co_' in op or 'addc' in op or 'subb' in op):
        w.add('vcc')
    if op.startswith('s_') and not op.startswith(_NO_SCC):
        w.add('scc')
    return frozenset(w)


@lru_cache(maxsize=None)
def _fact_units(f):
    if f[0] == 'b':
        return _units(f[1]) if f[1] != 'scc' else frozenset(('scc',))
    return (_units(f[1]) if f[1] != '0' else frozenset()) | (_units(f[2]) if f[2] != '0' else frozenset())


def _lin(tok):
    """-> (key, offset) of a 64-bit operand: a register pair or an integer constant"""
    if re.match(r'^-?(0x[0-9a-fA-F]+|\d+)$', tok):
        return ('0', int(tok, 0))
    m = _REG.match(tok)
    if m and m.group(1) and int(m.group(3)) == int(m.group(2)) + 1:
        return (tok, 0)
    return None


def _rel(a, b, cc, c):
    """-> fact (a - b cc c) over linear operands, True / False when it is decided, None when not expressible"""
    if a is None or b is None or cc not in _FLIP:
        return None
    (ka, oa), (kb, ob) = a, b
    c = c - oa + ob
    if ka == kb:
        return {'lt': 0 < c, 'le': 0 <= c, 'gt': 0 > c, 'ge': 0 >= c, 'eq': c == 0, 'ne': c != 0}[cc]
    if ka > kb:
        ka, kb, cc, c = kb, ka, _FLIP[cc], -c
    if abs(c) > 8:
        return None                             # (a loop counter carried round and round: forget it, the walk ends)
    return ('r', ka, kb, cc, c)


def _feasible(facts):
    bools, rng = {}, {}
    for f in facts:
        if f[0] == 'b':
            if bools.setdefault(f[1], f[2]) != f[2]:
                return False
        else:
            lo, hi, ex = rng.get((f[1], f[2]), (None, None, set()))
            cc, c = f[3], f[4]
            if cc in ('lt', 'le'):
                h = c - 1 if cc == 'lt' else c
                hi = h if hi is None else min(hi, h)
            elif cc in ('gt', 'ge'):
                lw = c + 1 if cc == 'gt' else c
                lo = lw if lo is None else max(lo, lw)
            elif cc == 'eq':
                lo = c if lo is None else max(lo, c)
                hi = c if hi is None else min(hi, c)
            else:
                ex = ex | {c}
            if lo is not None and hi is not None and (lo > hi or (lo == hi and lo in ex)):
                return False
            rng[(f[1], f[2])] = (lo, hi, ex)
    return True


def _add(facts, new):
    """-> facts + the decided-or-fact `new`, or None when they contradict"""
    if new is True:
        return facts
    if new is False:
        return None
    out = facts | {new}
    return out if _feasible(out) else None


def _subst(facts, key, repl):
    """facts (all touching a register just written) with pair `key` := repl (a linear operand, or None: unknown) -> facts or None"""
    out = frozenset()
    for f in facts:
        if f[0] == 'r' and key in (f[1], f[2]):
            a = repl if f[1] == key else (f[1], 0)
            b = repl if f[2] == key else (f[2], 0)
            g = _rel(a, b, f[3], f[4]) if repl is not None else None
            if g is None:
                continue                        # not expressible: forget it
            out = _add(out, g)
        else:
            continue                            # (a fact on a register the instruction writes in part: forget it)
        if out is None:
            return None
    return out


def _cmp_fact(op, a, b, val):
    """fact of `v_cmp_<cc>_<t>` / `s_cmp_<cc>_<t>` a, b being `val`, or None when the checker does not model the compare"""
    m = re.match(r'^[vs]_cmp_(lt|le|gt|ge|eq|ne|lg)_([iu])(64|32)', op)
    if not m:
        return None
    cc, sign, bits = ('ne' if m.group(1) == 'lg' else m.group(1)), m.group(2), m.group(3)
    if bits == '64' and (sign == 'i' or cc in ('eq', 'ne')):
        return _rel(_lin(a), _lin(b), cc if val else _NEG[cc], 0)
    return None


def _transfer(x, facts, prev):
    """facts after instruction x -> facts before it (None: contradiction).  prev: the instruction laid out before x (for the
    s_add_u32 / s_addc_u32 pair of a 64-bit add)"""
    w = _written(x)
    hit = [f for f in facts if _fact_units(f) & w]
    if not hit:
        return facts
    keep = frozenset(f for f in facts if not (_fact_units(f) & w))
    op, ops = x.op, _operands(x)
    dest = ops[0] if ops else None
    on_dest = [f for f in hit if f[0] == 'b' and f[1] == dest]
    rel_dest = [f for f in hit if f[0] == 'r' and dest in (f[1], f[2])]
    out = keep
    if op in ('s_and_b64', 's_andn2_b64') and len(ops) == 3 and 'exec' in ops[1:]:
        src = ops[2] if ops[1] == 'exec' else ops[1]
        if op == 's_andn2_b64' and ops[1] != 'exec':
            return keep
        for f in on_dest:
            out = _add(out, ('b', src, f[2] if op == 's_and_b64' else not f[2]))
            if out is None:
                return None
        return out
    if (op.startswith('v_cmp_') or op.startswith('s_cmp_')) and len(ops) >= 2:
        a, b = (ops[1], ops[2]) if op.startswith('v_cmp_') and len(ops) == 3 else (ops[0], ops[1])
        d = 'scc' if op.startswith('s_cmp_') else ('vcc' if op.endswith('_e32') else dest)
        m = re.match(r'^v_cmp_(eq|ne)_u32', op)
        for f in hit:
            if f[0] == 'b' and f[1] == d:
                if m and ('1' in (a, b)):
                    v = b if a == '1' else a
                    g = ('b', v, f[2] if m.group(1) == 'eq' else not f[2])
                else:
                    g = _cmp_fact(op, a, b, f[2])
                if g is not None:
                    out = _add(out, g)
                    if out is None:
                        return None
        return out
    if op == 'v_cndmask_b32_e64' and ops[1:3] == ['0', '1'] and len(ops) == 4:
        for f in on_dest:
            out = _add(out, ('b', ops[3], f[2]))
            if out is None:
                return None
        return out
    if op == 's_cselect_b64' and ops[1:] in (['-1', '0'], ['0', '-1']):
        for f in on_dest:
            out = _add(out, ('b', 'scc', f[2] if ops[1] == '-1' else not f[2]))
            if out is None:
                return None
        return out
    if op in ('s_mov_b64', 'v_mov_b64_e32') and len(ops) == 2:
        src = ops[1]
        if src in ('-1', '0') and on_dest:
            for f in on_dest:
                if f[2] != (src == '-1'):
                    return None
        res = frozenset(f for f in hit if not (f[0] == 'b' and f[1] == dest))
        if _units(src) or src in ('-1', '0'):
            out2 = keep
            for f in on_dest:
                if _units(src):
                    out2 = _add(out2, ('b', src, f[2]))
                    if out2 is None:
                        return None
            r = _subst(res, dest, _lin(src))
            return None if r is None else _union(out2, r)
        return keep
    if op in ('s_addc_u32', 's_subb_u32') and prev is not None and prev.op == ('s_add_u32' if op == 's_addc_u32' else 's_sub_u32'):
        lo, hi = _operands(prev), ops
        pair = _pair(lo[0], hi[0])
        srcp = _pair(lo[1], hi[1])
        if pair and srcp and re.match(r'^-?(0x[0-9a-fA-F]+|\d+)$', lo[2]) and re.match(r'^-?(0x[0-9a-fA-F]+|\d+)$', hi[2]):
            c = ((int(hi[2], 0) & 0xffffffff) << 32) | (int(lo[2], 0) & 0xffffffff)
            c = c - (1 << 64) if c >= (1 << 63) else c
            c = c if op == 's_addc_u32' else -c
            res = frozenset(f for f in hit if f[0] == 'r' and pair in (f[1], f[2]))
            r = _subst(res, pair, (srcp, c))
            return None if r is None else _union(keep, r)
    return keep


def _union(a, b):
    out = a
    for f in b:
        out = _add(out, f)
        if out is None:
            return None
    return out


def _pair(lo, hi):
    ml, mh = _REG.match(lo), _REG.match(hi)
    if ml and mh and ml.group(4) == 's' and mh.group(4) == 's' and int(mh.group(5)) == int(ml.group(5)) + 1:
        return f's[{ml.group(5)}:{mh.group(5)}]'
    return None


def _edge_fact(pins, taken):
    last = pins[-1]
    if last.op in ('s_cbranch_vccz', 's_cbranch_vccnz'):
        return ('b', 'vcc', taken == (last.op == 's_cbranch_vccnz'))
    if last.op in ('s_cbranch_scc0', 's_cbranch_scc1'):
        return ('b', 'scc', taken == (last.op == 's_cbranch_scc1'))
    return True


def _reachable(k, b0, i0, facts, limit=20000):
    """can an execution arrive at instruction i0 of block b0 with `facts` true?  Walks on backwards until the facts are all used
    up or the kernel entry is met (yes), or every way back contradicts them (no).  Gives up with yes after `limit` states."""
    stack, seen = [(b0, i0, facts)], set()
    while stack:
        b, i, f = stack.pop()
        if (b, i, f) in seen:
            continue
        seen.add((b, i, f))
        if len(seen) > limit:
            return True
        ins = k.blocks[b][1]
        for j in range(i - 1, -1, -1):
            if not f:
                return True
            f = _transfer(ins[j], f, ins[j - 1] if j > 0 else None)
            if f is None:
                break
        if f is None:
            continue
        if not f or b == 0:
            return True
        for p, _ in k.pred.get(b, []):
            pins = k.blocks[p][1]
            fp = f
            if pins and pins[-1].op.startswith('s_cbranch_'):
                fp = _add(f, _edge_fact(pins, taken=k.blocks[b][0] == pins[-1].args.split()[0]))
            if fp is not None:
                stack.append((p, len(pins), fp))
    return False


def _tagged(x):
    return x.in_asm and x.tag is not None and (x.vm_wait or 0) > 0


def _waits_before(k, cap=16):
    """-> {block: the most checked waits an execution can have passed on its way from the kernel entry to the block's start}"""
    best = {0: 0}
    inner = {b: sum(_tagged(x) for x in ins) for b, (_, ins) in enumerate(k.blocks)}
    changed = True
    while changed:
        changed = False
        for u, outs in k.succ.items():
            if u not in best:
                continue
            c = min(best[u] + inner[u], cap)
            for v, _ in outs:
                if best.get(v, -1) < c:
                    best[v] = c
                    changed = True
    return best


DRAINED = 'drained'


def min_count(k, b0, i0, m, after=0):
    """-> (count, [block labels of that path], entry_reached).  count: DRAINED when every path that can run meets a vmcnt(0)
    before the awaited request, None when no path that can run reaches either (a checker fault: the wait's table entry or the
    path rules are wrong -- check_asm fails on it)"""
    return _search(k, b0, i0, m, after)[:3]


def _search(k, b0, i0, m, after=0):
    """Fewest counted instructions between the m-th LDS-DMA request behind instruction i0 of block b0 and that instruction, over
    every backward path (Dijkstra over (block, requests still to find, checked waits passed)).  A path on which fewer than `after`
    checked waits can precede this one is an earlier iteration: the source sends those through the first-iteration waits, checked
    by their own entries.  -> (count, [block labels], entry_reached: the kernel entry met before m requests on a feasible path)"""
    before = _waits_before(k)
    best = None
    entry = drained = False
    seen = set()
    heap = [(0, 0, b0, i0, m, 0, frozenset(), (b0,))]
    tie = 1
    while heap:
        cost, _, b, i, need, s, facts, path = heappop(heap)
        key = (b, i, need, s, facts)
        if key in seen:
            continue
        seen.add(key)
        if best is not None and cost >= best[0]:
            break
        ins = k.blocks[b][1]
        done = False
        for j in range(i - 1, -1, -1):
            x = ins[j]
            if x.vm_wait == 0:
                done = True                     # everything older has landed: this path is safe
                if not drained and before.get(b, 0) + sum(_tagged(y) for y in ins[:j]) + s >= after and _reachable(k, b, j, facts):
                    drained = True
                break
            if x.dma:
                need -= 1
                if need == 0:
                    prefix = before.get(b, 0) + sum(_tagged(y) for y in ins[:j])
                    if prefix + s >= after and (best is None or cost < best[0]) and _reachable(k, b, j, facts):
                        best = (cost, path, j)
                    done = True
                    break
            if x.counted:
                cost += 1
            if _tagged(x):
                s = min(s + 1, after)
            facts = _transfer(x, facts, ins[j - 1] if j > 0 else None) if facts else facts
            if facts is None:
                done = True                     # this path cannot run
                break
        if done:
            continue
        preds = [p for p, dead in k.pred.get(b, []) if not dead]
        if not preds:
            if b == 0 and s >= after:
                entry = True
            continue
        for p in preds:
            pins = k.blocks[p][1]
            fp = facts
            if pins and pins[-1].op.startswith('s_cbranch_'):
                tgt = pins[-1].args.split()[0]
                fp = _add(facts, _edge_fact(pins, taken=k.blocks[b][0] == tgt))
            if fp is None:
                continue                        # both sides of one flag: this path cannot run
            heappush(heap, (cost, tie, p, len(pins), need, s, fp, path + (p,)))
            tie += 1
    if best is None:
        return (DRAINED if drained else None), [], entry, None
    labels = [k.blocks[b][0] or f'#{b}' for b in reversed(best[1])]
    return best[0], labels, entry, best


def min_path_lines(k, b0, i0, m, after=0):
    """-> assembly line numbers of the counted instructions between the awaited request and the wait on the path min_count reports"""
    _, _, _, found = _search(k, b0, i0, m, after)
    if found is None:
        return []
    _, path, j = found
    blocks = list(reversed(path))
    out = []
    for n, b in enumerate(blocks):
        ins = k.blocks[b][1]
        lo = j + 1 if n == 0 else 0
        hi = i0 if n == len(blocks) - 1 else len(ins)
        out += [x.line for x in ins[lo:hi] if x.counted]
    return out


def check_asm(asm_by_file, table=TABLE):
    """-> (failures, report): report[(file, kernel, tag, copy)] = (N, minimum count found)"""
    failures, report, matched = [], {}, defaultdict(int)
    for f, path in asm_by_file.items():
        kernels = parse_kernels(open(path).read())
        for name, k in kernels.items():
            copies = defaultdict(int)
            for b, i, x in hand_waits(k):
                n = x.vm_wait
                if x.tag is None:
                    failures.append(f'{f}: {name}: hand-written vmcnt({n}) at line {x.line} without a `; vmcheck <name>` tag')
                    continue
                key = (f, name, x.tag, copies[x.tag])
                copies[x.tag] += 1
                matched[key] += 1
                if key not in table:
                    failures.append(f'{f}: {name}: wait {x.tag} (copy {key[3]}, vmcnt({n})) has no table entry')
                    continue
                n_tab, m, after = table[key]
                if n != n_tab:
                    failures.append(f'{f}: {name}: wait {x.tag} (copy {key[3]}): the table says vmcnt({n_tab}), the assembly has vmcnt({n})')
                cnt, labels, entry = min_count(k, b, i, m, after)
                report[key] = (n, cnt)
                if cnt is None:
                    failures.append(f'{f}: {name}: wait {x.tag} (copy {key[3]}, vmcnt({n})): no path that can run reaches it from '
                                    f'LDS-DMA request {m} back or from a vmcnt(0)')
                if entry:
                    failures.append(f'{f}: {name}: wait {x.tag} (copy {key[3]}, vmcnt({n})): a path reaches the kernel entry before '
                                    f'{m} LDS-DMA requests')
                if cnt not in (None, DRAINED) and cnt < n:
                    failures.append(f'{f}: {name}: wait {x.tag} (copy {key[3]}): vmcnt({n}) but only {cnt} counted instructions issued '
                                    f'after the awaited request (LDS-DMA request {m} back) on path {" -> ".join(labels)}')
    for key in table:
        if key[0] in asm_by_file and matched.get(key, 0) != 1:
            failures.append(f'{key[0]}: {key[1]}: table entry {key[2]} copy {key[3]} matched {matched.get(key, 0)} waits')
    return failures, report


@pytest.fixture(scope='module')
def asm(tmp_path_factory):
    return compile_asm(tmp_path_factory.mktemp('vmcnt_asm'))


def test_hand_counted_waits(asm):
    failures, report = check_asm(asm)
    assert not failures, '\n'.join(failures)
    assert set(report) == set(TABLE)
    for key, (n, cnt) in sorted(report.items()):
        assert cnt == DRAINED or cnt >= n, (key, n, cnt)


# ---- the checker itself fails on a broken schedule -------------------------------------------------------------------------------


def _mutated(asm, tmp_path, f, edit):
    lines = open(asm[f]).read().splitlines(keepends=True)
    edit(lines)
    p = tmp_path / (f + '.s')
    p.write_text(''.join(lines))
    return {f: str(p)}


def _wait_line(lines, tag, copy=0):
    hits = [i for i, s in enumerate(lines) if 's_waitcnt' in s and re.search(r'vmcheck\s+' + re.escape(tag) + r'\b', s)]
    return hits[copy]


def _failures_for(asm_one, f):
    table = {k: v for k, v in TABLE.items() if k[0] == f}
    return check_asm(asm_one, table)[0]


def _min_path_store(path, kernel, tag, copy=0):
    """line number (1-based) of the store on the path that sets the minimum count of a wait"""
    k = parse_kernels(open(path).read())[kernel]
    b, i, _ = [w for w in hand_waits(k) if w[2].tag == tag][copy]
    n, m, after = next(v for key, v in TABLE.items() if key[1:] == (kernel, tag, copy))
    lines = open(path).read().splitlines()
    stores = [ln for ln in min_path_lines(k, b, i, m, after) if _STORE.match(lines[ln - 1].split()[0])]
    assert stores, (kernel, tag)
    return stores[-1]


def test_checker_catches_a_removed_store(asm, tmp_path):
    """ffn_bwd's steady vmcnt(3) counts the dX store of tile t - 2: without it only 2 operations follow the awaited request"""
    ln = _min_path_store(asm['ffn_bwd'], FFN_BWD, 'ffn_bwd.steady', 0)

    def edit(lines):
        assert 'global_store' in lines[ln - 1]
        del lines[ln - 1]
    fails = _failures_for(_mutated(asm, tmp_path, 'ffn_bwd', edit), 'ffn_bwd')
    assert any('ffn_bwd.steady' in s and 'vmcnt(3) but only 2' in s for s in fails), fails


def test_checker_catches_a_raised_count(asm, tmp_path):
    """gemm_dxdw<3>'s steady wait has no margin: vmcnt(5) would let tile t - 1's residual chunk still be on its way"""
    def edit(lines):
        w = _wait_line(lines, 'dxdw.steady')
        assert 'vmcnt(4)' in lines[w]
        lines[w] = lines[w].replace('vmcnt(4)', 'vmcnt(5)')
    fails = _failures_for(_mutated(asm, tmp_path, 'gemm_dxdw', edit), 'gemm_dxdw')
    assert any('dxdw.steady' in s and 'vmcnt(5) but only 4' in s for s in fails), fails


def test_checker_catches_a_dma_moved_below_a_store(asm, tmp_path):
    """attn_out_bwd's steady wait awaits the youngest row request of its tile, issued a tile ahead and followed by the dz store
    of that iteration: moved below that store, only [d_o store, DMA] = 2 operations would follow it"""
    def edit(lines):
        w = _wait_line(lines, 'attn_out_bwd.steady')
        # the dz store laid out above the wait (`nt`: the non-temporal row store of tile t - 1) and the row request right above it
        st = max(j for j in range(w) if lines[j].split()[:1] == ['global_store_dwordx4'] and lines[j].rstrip().endswith(' nt'))
        st = min(j for j in range(w) if lines[j].split()[:1] == ['global_store_dwordx4'] and j > max(
            k for k in range(st) if 'buffer_load_dwordx4' in lines[k] and re.search(r'\blds\b', lines[k])))
        d = max(k for k in range(st) if 'buffer_load_dwordx4' in lines[k] and re.search(r'\blds\b', lines[k]))
        ins = lines.pop(d)
        lines.insert(st, ins)       # (st moved up by one: the request now sits right behind the store)
    fails = _failures_for(_mutated(asm, tmp_path, 'attn_out_bwd', edit), 'attn_out_bwd')
    assert any('attn_out_bwd.steady' in s and 'vmcnt(3) but only 2' in s for s in fails), fails
