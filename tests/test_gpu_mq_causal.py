"""The causal form of the masked-query last-layer kernels (b4c_attn_mq_fwd_ex / b4c_attn_mq_bwd_ex with B4C_ATTN_CAUSAL), the route
ops.mq_causal opens for a causal encoder, and ranking at rows the caller names (predict_topk(flat_idx=, row_offsets=)).

NO REFERENCE ORACLE: the checker is a float64 restatement written here -- _ref of tests/test_gpu_mq.py with a -inf mask for the
keys behind each query's position -- and the full causal layer's own kernels (ops.attn_fwd(..., causal=True)) at the same rows.

Kernel cases: B = 9 sequences per layout, two layouts per dtype that together hold the lengths {1, 3, 31, 32, 33, 64, 65, 128, 129,
200} and 257 (fp32: a third 128-key block) or 512 (bf16), with {0, 1, 16, 17, 32, 33, 40} queries per sequence (the edges of the
16-query chunks and the 32-query tiles).  Positions ascend, hold position 0 and the last position wherever a sequence has two or
more queries (a single query sits at the last position: the ranking row), and one sequence of 129 keys has all its queries in its
first 32 positions (its later key tiles / its second key block are never entered)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
KERNELS = [(F32, 2, 64), (F32, 4, 32), (BF16, 2, 64), (BF16, 2, 32), (BF16, 3, 64)]
TOL = {F32: dict(o=2e-5, lse=1e-4, g=1e-4), BF16: dict(o=1.5e-2, lse=2e-2, g=3e-2)}      # test_attn_mq_kernels_match_fp64's


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops
    return ops


def _positions(n, nq, first32, g, short):
    """short: the positions end in front of the sequence's last two fifths (rows behind the last query in most sequences)"""
    if nq == 0:
        return []
    hi = 32 if first32 else max(nq, (3 * n) // 5) if short else n
    if nq == 1:
        return [hi - 1]
    assert nq <= hi
    inner = torch.randperm(hi - 2, generator=g)[:nq - 2] + 1
    return sorted([0, hi - 1] + inner.tolist())


class Layout:
    """(length, query count) per sequence -> cu, moff, q_rows (one more row, outside every range, holds -1)"""

    def __init__(self, spec, seed, first32=None, short=False):
        g = torch.Generator().manual_seed(seed)
        self.lens = [s[0] for s in spec]
        self.pos = [_positions(n, nq, b == first32, g, short) for b, (n, nq) in enumerate(spec)]
        self.B, self.S_arg = len(spec), max(self.lens)
        self.cu = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)
        self.moff = np.concatenate([[0], np.cumsum([len(p) for p in self.pos])]).astype(np.int32)
        self.T, self.R = int(self.cu[-1]), int(self.moff[-1]) + 1
        self.q_rows = np.asarray([int(self.cu[b]) + p for b in range(self.B) for p in self.pos[b]] + [-1], dtype=np.int32)
        self.seq_of = [b for b in range(self.B) for _ in self.pos[b]]
        self.qpos = [p for b in range(self.B) for p in self.pos[b]]
        self.cu_d, self.moff_d = torch.from_numpy(self.cu).cuda(), torch.from_numpy(self.moff).cuda()
        self.q_rows_d = torch.from_numpy(self.q_rows).cuda()

    def last(self, b):
        """the last query position of sequence b (-1: none)"""
        return self.pos[b][-1] if self.pos[b] else -1


def _specs(dtype):
    big = 257 if dtype == F32 else 512
    a = [(1, 1), (3, 0), (31, 16), (32, 17), (33, 32), (64, 33), (65, 40), (128, 1), (129, 17)]       # [8]: queries in the first 32
    b = [(200, 40), (big, 33), (129, 16), (65, 0), (33, 33), (3, 1), (1, 0), (64, 32), (128, 17)]
    assert {n for n, _ in a + b} == {1, 3, 31, 32, 33, 64, 65, 128, 129, 200, big}
    assert {m for _, m in a + b} == {0, 1, 16, 17, 32, 33, 40}
    return {'a': (a, 8), 'b': (b, None)}


_LAYOUTS = {}


def _layout(dtype, name, short=False):
    key = (dtype, name, short)
    if key not in _LAYOUTS:
        spec, first32 = _specs(dtype)[name]
        _LAYOUTS[key] = Layout(spec, 17 + len(name) + spec[1][0], first32, short)
    return _LAYOUTS[key]


def _operands(lay, dtype, H, dh, seed):
    """random q | k | v of every token, dO of every query row; q of a query row = the q columns of its token row"""
    g = torch.Generator().manual_seed(seed)
    d = H * dh
    qkv = (torch.randn(lay.T, 3 * d, generator=g) * 0.8).to(dtype)
    do = torch.randn(lay.R, d, generator=g).to(dtype)
    q = qkv[torch.from_numpy(lay.q_rows).long().clamp(min=0), :d].contiguous()        # (the unused slot: any row)
    return qkv, q, qkv[:, d:].contiguous(), do


def _pads(lay, kind, seed=1):
    """None; 'random': 15 % of the keys, never a sequence's first; 'leading': the first keys of some sequences (a query in front
    of the first live key sees padded keys only)"""
    if kind is None:
        return None
    pad = torch.zeros(lay.T, dtype=torch.uint8)
    if kind == 'random':
        pad = (torch.rand(lay.T, generator=torch.Generator().manual_seed(seed)) < 0.15).to(torch.uint8)
        pad[torch.from_numpy(lay.cu[:-1]).long()] = 0
    else:
        for b in range(lay.B):
            if lay.lens[b] >= 31 and b % 2 == 0:
                pad[int(lay.cu[b]):int(lay.cu[b]) + 5] = 1
    return pad


def _ref(lay, q, kv, go, H, dh, key_pad=None, keep=None, rate=0.0):
    """float64, the rows of lay.q_rows[:-1]: softmax over the keys k <= p with -inf behind p (tests/test_gpu_mq.py::_ref plus that
    mask); keep [B, H, S_arg, S_arg] bool: dropout on P with 1 / (1 - rate)"""
    q64 = q.double().clone().requires_grad_(True)
    kv64 = kv.double().clone().requires_grad_(True)
    d = H * dh
    outs, lses = [], []
    for b in range(lay.B):
        t0, t1, r0, r1 = int(lay.cu[b]), int(lay.cu[b + 1]), int(lay.moff[b]), int(lay.moff[b + 1])
        if r1 == r0:
            continue
        p = torch.tensor(lay.pos[b])
        behind = torch.arange(t1 - t0)[None, :] > p[:, None]
        o_b, l_b = [], []
        for h in range(H):
            s = q64[r0:r1, h * dh:(h + 1) * dh] @ kv64[t0:t1, h * dh:(h + 1) * dh].t() / np.sqrt(dh)
            if key_pad is not None:
                s = s + key_pad[t0:t1].double()[None, :] * -1e9
            s = s.masked_fill(behind, float('-inf'))
            P = torch.softmax(s, 1)
            if keep is not None:
                P = P * keep[b, h][p][:, :t1 - t0].double() / (1.0 - rate)
            l_b.append(torch.logsumexp(s, 1))
            o_b.append(P @ kv64[t0:t1, d + h * dh:d + (h + 1) * dh])
        outs.append(torch.cat(o_b, 1))
        lses.append(torch.stack(l_b, 1))
    o = torch.cat(outs, 0)
    (o * go[:-1].double()).sum().backward()
    return o.detach(), torch.cat(lses, 0).detach(), q64.grad[:-1], kv64.grad


def _run(ops, lay, q, kv, do, H, dh, kp, rate=0.0, seed=0, causal=True):
    kp_d = kp.cuda() if kp is not None else None
    qd, kvd, dod = q.cuda(), kv.cuda(), do.cuda()
    kw = {'causal': True} if causal else {}
    o, lse = ops.attn_mq_fwd(qd, kvd, lay.cu_d, lay.moff_d, lay.B, lay.S_arg, H, dh, kp_d, lay.q_rows_d, rate, seed, **kw)
    dq, dkv = ops.attn_mq_bwd(qd, kvd, lay.cu_d, lay.moff_d, o, dod, lse, lay.B, lay.S_arg, H, dh, kp_d, lay.q_rows_d, rate, seed, **kw)
    torch.cuda.synchronize()
    return o, lse, dq, dkv


def _full_causal(ops, lay, qkv, dtype, H, dh, kp, rate=0.0, seed=0):
    """o [T, d] and lse [B, H, S_arg] of the full causal layer (ops.attn_fwd(causal=True)) on the same q | k | v.  bf16: its packed
    layout; fp32 (no packed layout): the dense kernels at the pitch max_len with the tails as padded keys -- the same positions,
    the same (b, h, q, k, S_arg) of the keep rule."""
    pad = kp if kp is not None else torch.zeros(lay.T, dtype=torch.uint8)
    if dtype == BF16:
        return ops.attn_fwd(qkv.cuda(), pad.cuda(), lay.B, lay.S_arg, H, dh, lay.cu_d, rate, seed, causal=True)
    S = lay.S_arg
    dense = torch.zeros(lay.B * S, qkv.shape[1], dtype=dtype)
    dpad = torch.ones(lay.B * S, dtype=torch.uint8)
    for b in range(lay.B):
        dense[b * S:b * S + lay.lens[b]] = qkv[lay.cu[b]:lay.cu[b + 1]]
        dpad[b * S:b * S + lay.lens[b]] = pad[lay.cu[b]:lay.cu[b + 1]]
    o, lse = ops.attn_fwd(dense.cuda(), dpad.cuda(), lay.B, S, H, dh, None, rate, seed, causal=True)
    return torch.cat([o[b * S:b * S + lay.lens[b]] for b in range(lay.B)]), lse


def _check(name, got, want, tol, absolute=False):
    e = float((got.double().cpu() - want).abs().max())
    bound = tol if absolute else tol * max(1.0, float(want.abs().max()))
    print('  %s: max error %.3e (bound %.3e)' % (name, e, bound))
    assert e < bound, (name, e, bound)


# ---- 1. float64 parity and the full causal layer ------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad', [None, 'random'])
@pytest.mark.parametrize('name', ['a', 'b'])
@pytest.mark.parametrize('dtype,H,dh', KERNELS)
def test_causal_kernels_match_fp64_and_the_full_layer(ops, dtype, H, dh, name, pad):
    lay = _layout(dtype, name)
    assert any(lay.lens[b] >= 129 and lay.pos[b] and lay.pos[b][-1] <= 31 for b in range(lay.B)) == (name == 'a')
    qkv, q, kv, do = _operands(lay, dtype, H, dh, 100 + H * dh + lay.T)
    kp = _pads(lay, pad)
    ro, rl, rdq, rdkv = _ref(lay, q, kv, do, H, dh, kp)
    o, lse, dq, dkv = _run(ops, lay, q, kv, do, H, dh, kp)
    t = TOL[dtype]
    print('causal mq %s H=%d dh=%d layout %s pad=%s' % (dtype, H, dh, name, pad))
    _check('o', o[:-1], ro, t['o'])
    _check('lse', lse[:-1], rl, t['lse'], absolute=True)
    _check('dq', dq[:-1], rdq, t['g'])
    _check('dkv', dkv, rdkv, t['g'])
    assert not o[-1].any() and not lse[-1].any() and not dq[-1].any()          # the row outside every range
    # the same rows of the full causal layer
    o_full, lse_full = _full_causal(ops, lay, qkv, dtype, H, dh, kp)
    used = torch.from_numpy(lay.q_rows[:-1]).long()
    want_l = torch.stack([lse_full[b, :, p] for b, p in zip(lay.seq_of, lay.qpos)]).double().cpu()
    _check('o against the full layer', o[:-1], o_full.double().cpu()[used], t['o'])
    _check('lse against the full layer', lse[:-1], want_l, t['lse'], absolute=True)
    # it is not the bidirectional function of the same operands
    o_bi = _run(ops, lay, q, kv, do, H, dh, kp, causal=False)[0]
    assert float((o_bi[:-1].double().cpu() - ro).abs().max()) > 10 * t['o'] * max(1.0, float(ro.abs().max()))


@pytest.mark.parametrize('dtype,H,dh', [(F32, 2, 64), (BF16, 2, 64)])
def test_leading_pads_come_out_finite(ops, dtype, H, dh):
    """a query in front of its sequence's first live key sees padded keys only: finite, not otherwise pinned (as in the full
    kernels).  Its dO is zero here, so it adds nothing to dk | dv and every other row keeps its float64 bound."""
    lay = _layout(dtype, 'a')
    qkv, q, kv, do = _operands(lay, dtype, H, dh, 5 + dh)
    kp = _pads(lay, 'leading')
    blind = torch.tensor([bool(kp[int(lay.cu[b]):int(lay.cu[b]) + p + 1].all()) for b, p in zip(lay.seq_of, lay.qpos)] + [False])
    assert 2 <= int(blind.sum()) < lay.R // 2
    do[blind] = 0
    ro, rl, rdq, rdkv = _ref(lay, q, kv, do, H, dh, kp)
    o, lse, dq, dkv = _run(ops, lay, q, kv, do, H, dh, kp)
    for x in (o, lse, dq, dkv):
        assert bool(torch.isfinite(x).all())
    seen = ~blind[:-1]
    t = TOL[dtype]
    _check('o', o[:-1][seen], ro[seen], t['o'])
    _check('lse', lse[:-1][seen], rl[seen], t['lse'], absolute=True)
    _check('dq', dq[:-1][seen], rdq[seen], t['g'])
    _check('dkv', dkv, rdkv, t['g'])


# ---- 2. exact properties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['a', 'b'])
@pytest.mark.parametrize('dtype,H,dh', KERNELS)
def test_prefix_property_bit_for_bit(ops, dtype, H, dh, name):
    lay = _layout(dtype, name, short=True)
    d = H * dh
    _, q, kv, do = _operands(lay, dtype, H, dh, 31 + dh + H)
    kp = _pads(lay, 'random', seed=3)
    base = _run(ops, lay, q, kv, do, H, dh, kp)
    # the k | v rows behind each sequence's last query position: other finite values, 1e3 times larger
    g = torch.Generator().manual_seed(9)
    other = kv.clone()
    changed = 0
    for b in range(lay.B):
        t0, t1 = int(lay.cu[b]) + lay.last(b) + 1, int(lay.cu[b + 1])
        other[t0:t1] = (torch.randn(t1 - t0, 2 * d, generator=g) * 800.0).to(dtype)
        changed += t1 - t0
    assert changed > lay.T // 10
    got = _run(ops, lay, q, other, do, H, dh, kp)
    for nm, a, b_ in zip(('o', 'lse', 'dq'), base, got):
        assert torch.equal(a, b_), nm
    for b in range(lay.B):
        t0, t1 = int(lay.cu[b]), int(lay.cu[b]) + lay.last(b) + 1
        assert torch.equal(base[3][t0:t1], got[3][t0:t1]), b
        assert not got[3][t1:int(lay.cu[b + 1])].any(), b                       # ... and behind it: exact zeros
    # per query: the keys behind IT change nothing in its o / lse row (one launch per step of the positions, forward only)
    for step in (0, 1, 2):
        other = kv.clone()
        rows = []
        for b in range(lay.B):
            if len(lay.pos[b]) > step + 1:
                i = (len(lay.pos[b]) - 1) * step // 3
                t0 = int(lay.cu[b]) + lay.pos[b][i] + 1
                other[t0:int(lay.cu[b + 1])] = (torch.randn(int(lay.cu[b + 1]) - t0, 2 * d, generator=g) * 800.0).to(dtype)
                rows += list(range(int(lay.moff[b]), int(lay.moff[b]) + i + 1))          # the queries at or in front of it
        o2, lse2 = ops.attn_mq_fwd(q.cuda(), other.cuda(), lay.cu_d, lay.moff_d, lay.B, lay.S_arg, H, dh, kp.cuda(), lay.q_rows_d, causal=True)
        assert len(rows) >= 4 and torch.equal(o2[rows], base[0][rows]) and torch.equal(lse2[rows], base[1][rows])
        assert not torch.equal(o2, base[0])


def _raw(ops, lay, dtype, H, dh, name, q, kv, kp, o, lse, do=None, dq=None, dkv=None, tail=(), q_offsets=None):
    """one raw call of b4c_attn_mq_{fwd,bwd}_{drop,ex}; tail = (q_rows, rate, seed[, flags])"""
    from bert4clickpath_amd import _lib as L
    p, st, dt, d = ops._p, ops._st(), ops.dt_code(dtype), H * dh
    head = (p(q), d, p(kv), 2 * d, p(kp), p(lay.cu_d), p(lay.moff_d if q_offsets is None else q_offsets), p(o), d)
    if 'fwd' in name:
        args = head + (p(lse), lay.B, lay.S_arg, H, dh, dt, st)
    else:
        args = head + (p(do), d, p(lse), p(dq), d, p(dkv), 2 * d, lay.B, lay.S_arg, H, dh, dt, st)
    return getattr(L.lib(), name)(*(args + (p(tail[0]),) + tuple(tail[1:])))


def _raw_pair(ops, lay, dtype, H, dh, kind, q, kv, kp, do, tail, q_rows=None, q_offsets=None):
    """forward + backward through the raw entry points, dkv prefilled with NaN"""
    R = q.shape[0]
    o = torch.zeros(R, H * dh, dtype=dtype, device='cuda')
    lse = torch.zeros(R, H, dtype=torch.float32, device='cuda')
    dq, dkv = torch.zeros_like(o), torch.full_like(kv, float('nan'))
    assert _raw(ops, lay, dtype, H, dh, 'b4c_attn_mq_fwd_' + kind, q, kv, kp, o, lse, tail=tail, q_offsets=q_offsets) == 0
    assert _raw(ops, lay, dtype, H, dh, 'b4c_attn_mq_bwd_' + kind, q, kv, kp, o, lse, do, dq, dkv, tail=tail, q_offsets=q_offsets) == 0
    torch.cuda.synchronize()
    return o, lse, dq, dkv


@pytest.mark.parametrize('name', ['a', 'b'])
@pytest.mark.parametrize('dtype,H,dh', KERNELS)
def test_dkv_behind_the_last_query_is_written_as_zeros(ops, dtype, H, dh, name):
    from bert4clickpath_amd import _lib as L
    lay = _layout(dtype, name, short=True)
    _, q, kv, do = _operands(lay, dtype, H, dh, 41 + dh)
    o, lse, dq, dkv = _raw_pair(ops, lay, dtype, H, dh, 'ex', q.cuda(), kv.cuda(), None, do.cuda(), (lay.q_rows_d, 0.0, 0, L.ATTN_CAUSAL))
    assert not bool(torch.isnan(dkv).any()) and not bool(torch.isnan(dq).any())
    zero_rows = 0
    for b in range(lay.B):
        t1 = int(lay.cu[b]) + lay.last(b) + 1                                    # (no query: the whole sequence)
        assert not dkv[t1:int(lay.cu[b + 1])].any(), b
        zero_rows += int(lay.cu[b + 1]) - t1
        if lay.pos[b]:
            assert bool(dkv[int(lay.cu[b]):t1].any())
    assert zero_rows > lay.T // 10 and any(not p for p in lay.pos)


@pytest.mark.parametrize('dtype,H,dh', KERNELS)
def test_slots_without_a_visible_key(ops, dtype, H, dh):
    """q_rows = -1 INSIDE a range, in trailing slots (the padded form of ClickstreamTransformer._forward): o = 0, lse = 0, dq = 0,
    and dk | dv bit-identical to the launch without those slots -- with dO of those rows zero and non-zero"""
    lay = _layout(dtype, 'a')
    d = H * dh
    _, q, kv, do = _operands(lay, dtype, H, dh, 51 + dh)
    base = _run(ops, lay, q, kv, do, H, dh, None)
    # every sequence gets up to 3 trailing slots: (1 query -> 4 slots, 16 -> 19, 17 -> 20, 32 -> 35: a second tile, 0 -> 3: only slots)
    extra = 3
    counts = [len(p) + extra for p in lay.pos]
    moff2 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    R2 = int(moff2[-1]) + 1
    rows2 = np.full(R2, -1, dtype=np.int32)
    src = np.full(R2, -1, dtype=np.int64)                                        # the base row of every kept row
    for b in range(lay.B):
        n = len(lay.pos[b])
        rows2[moff2[b]:moff2[b] + n] = lay.q_rows[lay.moff[b]:lay.moff[b] + n]
        src[moff2[b]:moff2[b] + n] = np.arange(lay.moff[b], lay.moff[b] + n)
    kept = torch.from_numpy(src >= 0)
    g = torch.Generator().manual_seed(4)
    q2 = (torch.randn(R2, d, generator=g) * 0.8).to(dtype)
    q2[kept] = q[torch.from_numpy(src[src >= 0])]
    for nonzero in (False, True):
        do2 = (torch.randn(R2, d, generator=g) if nonzero else torch.zeros(R2, d)).to(dtype)
        do2[kept] = do[torch.from_numpy(src[src >= 0])]
        qd, kvd = q2.cuda(), kv.cuda()
        moff_d, rows_d = torch.from_numpy(moff2).cuda(), torch.from_numpy(rows2).cuda()
        o, lse = ops.attn_mq_fwd(qd, kvd, lay.cu_d, moff_d, lay.B, lay.S_arg, H, dh, None, rows_d, causal=True)
        dq, dkv = ops.attn_mq_bwd(qd, kvd, lay.cu_d, moff_d, o, do2.cuda(), lse, lay.B, lay.S_arg, H, dh, None, rows_d, causal=True)
        for x in (o, lse, dq, dkv):
            assert bool(torch.isfinite(x).all())
        slots = ~kept.cuda()
        assert not o[slots].any() and not lse[slots].any() and not dq[slots].any()
        kd = kept.cuda()
        assert torch.equal(o[kd], base[0][:-1]) and torch.equal(lse[kd], base[1][:-1]) and torch.equal(dq[kd], base[2][:-1])
        assert torch.equal(dkv, base[3]), nonzero


@pytest.mark.parametrize('rate', [0.0, 0.2])
@pytest.mark.parametrize('dtype,H,dh', KERNELS)
def test_flags_zero_is_the_drop_entry_point(ops, dtype, H, dh, rate):
    lay = _layout(dtype, 'b')
    _, q, kv, do = _operands(lay, dtype, H, dh, 61 + dh)
    kp = _pads(lay, 'random', seed=5).cuda()
    q, kv, do = q.cuda(), kv.cuda(), do.cuda()
    old = _raw_pair(ops, lay, dtype, H, dh, 'drop', q, kv, kp, do, (lay.q_rows_d, rate, 77))
    new = _raw_pair(ops, lay, dtype, H, dh, 'ex', q, kv, kp, do, (lay.q_rows_d, rate, 77, 0))
    assert bool(torch.isfinite(old[3]).all())
    for a, b in zip(old, new):
        assert torch.equal(a, b)


@pytest.mark.parametrize('dtype,H,dh', [(F32, 2, 64), (BF16, 2, 64)])
def test_bad_flags_write_nothing(ops, dtype, H, dh):
    from bert4clickpath_amd import _lib as L
    lay = _layout(dtype, 'a')
    _, q, kv, do = _operands(lay, dtype, H, dh, 71)
    q, kv, do = q.cuda(), kv.cuda(), do.cuda()
    o = torch.full((lay.R, H * dh), 7.0, dtype=dtype, device='cuda')
    lse = torch.full((lay.R, H), 7.0, dtype=torch.float32, device='cuda')
    dq, dkv = torch.full_like(o, 7.0), torch.full_like(kv, 7.0)
    for q_rows, rate, flags, what in ((lay.q_rows_d, 0.0, 2, b'flag'), (lay.q_rows_d, 0.2, 3, b'flag'), (None, 0.0, 1, b'q_rows'),
                                      (None, 0.2, 1, b'q_rows')):
        for name in ('b4c_attn_mq_fwd_ex', 'b4c_attn_mq_bwd_ex'):
            rc = _raw(ops, lay, dtype, H, dh, name, q, kv, None, o, lse, do, dq, dkv, tail=(q_rows, rate, 5, flags))
            assert rc == L._C['B4C_EINVAL'] and what in L.lib().b4c_last_error(), (name, flags)
    torch.cuda.synchronize()
    for t in (o, lse, dq, dkv):
        assert bool((t == 7.0).all())


# ---- 3. dropout -----------------------------------------------------------------------------------------------------------------------
_DROP_SPEC = [(70, 33), (7, 0), (33, 10), (1, 1), (40, 17)]          # three key tiles, a one-key sequence, no query, two query passes


@pytest.mark.parametrize('dtype,H,dh', [(BF16, 2, 64), (BF16, 2, 32), (F32, 2, 64)])
def test_kept_set_is_the_full_causal_layers(ops, dtype, H, dh):
    """q = 0: P is uniform over the visible keys.  V row k = one-hot at column k - k0 for the keys k0 .. k0 + dh of a pass, so o of a
    pass IS the keep bits of the visible keys among them (tests/test_gpu_mq_attn_dropout.py::test_outputs_are_the_masks); dO row =
    one-hot at the row's number inside its sequence, so dV is their transpose.  The same operands through the full causal layer
    give what that layer draws at those rows: equal, bit for bit, and equal to b4c_attn_keep for k <= p, nothing for k > p."""
    from bert4clickpath_amd import _lib as L
    lay = Layout(_DROP_SPEC, 3)
    rate, seed = 0.2, 0xCA05A1 + dh
    d, R, T, S_arg = H * dh, lay.R, lay.T, lay.S_arg
    lib = L.lib()
    want = np.zeros((R - 1, H, S_arg), dtype=bool)
    for r, (b, p) in enumerate(zip(lay.seq_of, lay.qpos)):
        for h in range(H):
            for k in range(p + 1):
                want[r, h, k] = bool(lib.b4c_attn_keep(seed, b, h, p, k, H, S_arg, rate))
    q = torch.zeros(R, d, dtype=dtype, device='cuda')
    used = torch.from_numpy(lay.q_rows[:-1]).long()
    got, full = np.zeros_like(want), np.zeros_like(want)
    lse = None
    for k0 in range(0, S_arg, dh):
        kv = torch.zeros(T, 2 * d, dtype=dtype)
        for b in range(lay.B):
            for k in range(k0, min(k0 + dh, lay.lens[b])):
                for h in range(H):
                    kv[lay.cu[b] + k, d + h * dh + k - k0] = 1.0
        o, lse = ops.attn_mq_fwd(q, kv.cuda(), lay.cu_d, lay.moff_d, lay.B, S_arg, H, dh, None, lay.q_rows_d, rate, seed, causal=True)
        n = min(dh, S_arg - k0)
        got[:, :, k0:k0 + n] = (o[:-1].float().cpu().view(R - 1, H, dh) != 0).numpy()[:, :, :n]
        qkv = torch.cat([torch.zeros(T, d, dtype=dtype), kv], 1)
        o_full, _ = _full_causal(ops, lay, qkv, dtype, H, dh, None, rate, seed)
        full[:, :, k0:k0 + n] = (o_full.float().cpu()[used].view(R - 1, H, dh) != 0).numpy()[:, :, :n]
    assert np.array_equal(got, full) and np.array_equal(got, want)
    vis = np.concatenate([want[r, :, :p + 1].ravel() for r, p in enumerate(lay.qpos)])
    assert 0.7 < float(vis.mean()) < 0.9
    for r, p in enumerate(lay.qpos):                          # lse: the undropped softmax over the p + 1 visible keys
        assert float((lse[r].cpu() - np.log(p + 1)).abs().max()) < 1e-4
    # backward: dV[k][c] = P~[query g0 + c of the sequence][k]; dQ and dK are exactly zero (k = 0, and q = 0)
    zkv, zo = torch.zeros(T, 2 * d, dtype=dtype, device='cuda'), torch.zeros(R, d, dtype=dtype, device='cuda')
    gotb = np.zeros_like(want)
    for g0 in range(0, max(len(p) for p in lay.pos), dh):
        do = torch.zeros(R, d, dtype=dtype)
        for r, b in enumerate(lay.seq_of):
            c = r - int(lay.moff[b]) - g0
            if 0 <= c < dh:
                for h in range(H):
                    do[r, h * dh + c] = 1.0
        dq, dkv = ops.attn_mq_bwd(q, zkv, lay.cu_d, lay.moff_d, zo, do.cuda(), lse, lay.B, S_arg, H, dh, None, lay.q_rows_d, rate, seed,
                                  causal=True)
        assert not dq.any() and not dkv[:, :d].any()
        dv = (dkv[:, d:].float().cpu().view(T, H, dh) != 0).numpy()
        for r, b in enumerate(lay.seq_of):
            c = r - int(lay.moff[b]) - g0
            if 0 <= c < dh:
                gotb[r, :, :lay.lens[b]] = dv[lay.cu[b]:lay.cu[b + 1], :, c].T
    assert np.array_equal(gotb, want)


@pytest.mark.parametrize('name', ['a', 'b'])
@pytest.mark.parametrize('dtype,H,dh', KERNELS)
def test_dropout_matches_fp64_with_the_regenerated_mask(ops, dtype, H, dh, name):
    lay = _layout(dtype, name)
    rate, seed = 0.2, 0xFACE + dh + lay.T
    _, q, kv, do = _operands(lay, dtype, H, dh, 11 + dh + lay.T)
    kp = _pads(lay, 'random', seed=7)
    keep = ops.attn_keep_mask(seed, lay.B, H, lay.S_arg, rate)
    ro, rl, rdq, rdkv = _ref(lay, q, kv, do, H, dh, kp, keep, rate)
    o, lse, dq, dkv = _run(ops, lay, q, kv, do, H, dh, kp, rate, seed)
    t = TOL[dtype]
    print('causal mq dropout %s H=%d dh=%d layout %s' % (dtype, H, dh, name))
    _check('o', o[:-1], ro, t['o'])
    _check('lse', lse[:-1], rl, t['lse'], absolute=True)
    _check('dq', dq[:-1], rdq, t['g'])
    _check('dkv', dkv, rdkv, t['g'])
    o0 = ops.attn_mq_fwd(q.cuda(), kv.cuda(), lay.cu_d, lay.moff_d, lay.B, lay.S_arg, H, dh, kp.cuda(), lay.q_rows_d, causal=True)[0]
    assert not torch.equal(o0, o)


# ---- 4. the model ---------------------------------------------------------------------------------------------------------------------
def _build(V, d, L, H, head_dims, dtype, seed, dropout=0.0, **kw):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(seed)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': d}, SoftMaxHead(list(head_dims), V),
                               value_to_head='[MASK]', num_encoder_layers=L, num_attention_heads=H, dropout_rate=dropout,
                               compute_dtype=dtype, **kw)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias') or n.endswith('beta'):
                p.normal_(0, 0.05)
    return m.cuda()


def _batch(B, S, V, seed, min_len=3):
    from bert4clickpath_amd import input_pipeline
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=seed, min_len=min_len)
    ids = torch.from_numpy(b['ids'])
    return b, ids, {'asin': ids[:, 2:S - 1].contiguous().cuda()}, torch.from_numpy(b['labels_padded']).cuda()


class _CountMQ:
    """counts the passes that take the masked-query last layer and notes the trailing argument (tests/test_gpu_causal_model.py)"""

    def __init__(self, ops):
        self.ops, self.calls, self.last = ops, 0, []

    def __enter__(self):
        self._orig = self.ops.MQAttnBlockFn
        rec = self

        class Noting(self._orig):
            @staticmethod
            def apply(*a, **k):
                rec.calls += 1
                rec.last.append(a[-1])
                return rec._orig.apply(*a, **k)
        self.ops.MQAttnBlockFn = Noting
        return self

    def __exit__(self, *exc):
        self.ops.MQAttnBlockFn = self._orig


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


def _clear_rows(model, rows, V, K):
    """the rows whose K + 1 leading reference logits are 1e-3 apart, and their ranking (test_full_last_layer_and_predict_topk)"""
    logits = model.head.logits(rows, out_fp32=True)[:, :V].float().cpu().numpy()
    order = np.argsort(-logits, axis=1, kind='stable')[:, :K + 1]
    top = np.take_along_axis(logits, order, 1)
    return (top[:, :-1] - top[:, 1:] > 1e-3).all(1), order[:, :K]


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
def test_predict_topk_switch_on_equals_switch_off(ops, dtype):
    """the model, seed and batch of tests/test_gpu_causal_model.py::test_full_last_layer_and_predict_topk"""
    V, d, L, H, B, S, K = 40, 64, 2, 2, 6, 12, 5
    model = _build(V, d, L, H, [32], dtype, 9, attention='causal')
    with torch.no_grad():
        model.head.output_layer.kernel.mul_(4.0)
    b, ids, feats, labels = _batch(B, S, V, 7)
    assert not ops.mq_causal
    with _CountMQ(ops) as mq:                                # switch off: the parent's route and result
        off = model.predict_topk(feats, K, labels)
        probs_off = model(feats, training=False)
    assert mq.calls == 0
    with torch.no_grad():
        full = model.transformer({'items': ids.cuda()}, training=False)
        rows = full.reshape(B * S, d)[torch.from_numpy(b['flat_idx']).long().cuda()]
        clear, want = _clear_rows(model, rows, V, K)
    assert clear.mean() > 0.5 and len(set(map(tuple, want[clear]))) > 1
    assert np.array_equal(off[0].cpu().numpy()[clear], want[clear])
    ops.mq_causal = True
    try:
        enc = model.transformer.encoder
        assert enc.rows_route(dtype, False) and not enc.rows_supported(dtype)
        with _CountMQ(ops) as mq:
            on = model.predict_topk(feats, K, labels)
            assert mq.calls == 1 and mq.last == [True]
            probs_on = model(feats, training=False)              # the padded form: unused slots hold -1 inside the ranges
            assert mq.calls == 2
    finally:
        ops.mq_causal = False
    assert np.array_equal(on[0].cpu().numpy()[clear], off[0].cpu().numpy()[clear])
    assert np.array_equal((on[1].cpu().numpy() > 0)[clear], (off[1].cpu().numpy() > 0)[clear])
    # the padded (B, M, V) output ranks the same way (fp32, as in that test: bf16 probabilities 1e-3 apart round to one number)
    assert bool(torch.isfinite(probs_on.float()).all()) and probs_on.shape == probs_off.shape
    valid = (labels[:, :probs_on.shape[1]] != -1).cpu().numpy()
    assert int(valid.sum()) == on[0].shape[0]
    if dtype == F32:
        for probs in (probs_on, probs_off):
            ranked = np.argsort(-probs.detach().float().cpu().numpy()[valid], axis=1, kind='stable')[:, :K]
            assert np.array_equal(ranked[clear], want[clear])
    with _CountMQ(ops) as mq:                                # and off again: nothing stays behind
        again = model.predict_topk(feats, K, labels)
    assert mq.calls == 0 and torch.equal(again[0], off[0])


def _step(model, feats, labels, **kw):
    model.zero_grad()
    loss = model.cloze_loss(feats, labels, training=True, **kw)
    loss.backward()
    return float(loss.detach()), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _same_step(dtype, on, off):
    """bounds of tests/test_gpu_mq.py, masked-query last layer against full layer"""
    (la, ga), (lb, gb) = on, off
    if dtype == F32:
        assert abs(la - lb) < 2e-6 * abs(lb), (la, lb)
        for n in ga:
            assert _rel(ga[n], gb[n]) < 2e-4 or float(gb[n].abs().max()) < 1e-7, n
    else:
        assert abs(la - lb) < 3e-3 * abs(lb), (la, lb)
        for n in ga:
            if float(gb[n].float().norm()) < 1e-9 or n.endswith('mha.wk.bias'):
                continue
            assert _rel(ga[n], gb[n]) < 0.08, n


@pytest.mark.parametrize('dtype,packed', [(F32, False), (BF16, False), (BF16, True)], ids=['fp32-dense', 'bf16-dense', 'bf16-packed'])
def test_cloze_loss_and_gradients_switch_on_against_off(ops, dtype, packed):
    """fp32: the model and batch of test_masked_query_last_layer_fp32_equals_full_layer_and_oracle (L = 2), causal; bf16: those of
    test_masked_query_last_layer_bf16_packed_and_dropout.  Both forms of cloze_loss (the one that reads the row count back and
    max_masked_per_row)."""
    if dtype == F32:
        V, S, B = 90, 40, 7
        model = _build(V, 64, 2, 2, (32, 24), dtype, 3, attention='causal')
        b, ids, feats, labels = _batch(B, S, V, 5)
    else:
        V, S, B = 300, 48, 12
        model = _build(V, 128, 2, 2, (64, 128), dtype, 3, attention='causal')
        b, ids, feats, labels = _batch(B, S, V, 21)
    lay = {'n_real_tokens': int((b['ids'] != 0).sum())} if packed else {'packed': False}
    res = {}
    for on in (False, True):
        ops.mq_causal = on
        try:
            for form in ({}, {'max_masked_per_row': 10}):
                with _CountMQ(ops) as mq:
                    res[(on, bool(form))] = _step(model, feats, labels, **form, **lay)
                assert mq.calls == (1 if on else 0) and (model._packed is not None) == packed
        finally:
            ops.mq_causal = False
    for form in (False, True):
        _same_step(dtype, res[(True, form)], res[(False, form)])


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
def test_training_pass_with_attention_dropout_and_both_switches(ops, dtype):
    """attention_dropout_rate = 0.2, residual dropout 0 (its masks are indexed by the row of the tensor they drop: other draws on the
    two routes): the masked-query kernels draw the full causal layer's masks, so the loss is the switch-off loss"""
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    V, S, B = 500, 32, 8
    model = _build(V, 128, 2, 2, (128, 64), dtype, 3, attention='causal', attention_dropout_rate=0.2)
    b, ids, feats, labels = _batch(B, S, V, 21)
    kw = {'n_real_tokens': int((b['ids'] != 0).sum())} if dtype == BF16 else {}
    res = {}
    prev = (ops.mq_causal, ops.mq_attn_dropout)
    try:
        for causal_on, drop_on, calls in ((False, False, 0), (True, False, 0), (False, True, 0), (True, True, 1)):
            ops.mq_causal, ops.mq_attn_dropout = causal_on, drop_on
            T.set_dropout_seed(5)
            with _CountMQ(ops) as mq:
                res[(causal_on, drop_on)] = _step(model, feats, labels, max_masked_per_row=10, **kw)
            assert mq.calls == calls, (causal_on, drop_on)
    finally:
        ops.mq_causal, ops.mq_attn_dropout = prev
    _same_step(dtype, res[(True, True)], res[(False, False)])
    model0 = _build(V, 128, 2, 2, (128, 64), dtype, 3, attention='causal')
    T.set_dropout_seed(5)
    assert _step(model0, feats, labels, max_masked_per_row=10, **kw)[0] != res[(False, False)][0]       # the masks are in the step


@pytest.mark.parametrize('attention,dtype', [('causal', F32), ('causal', BF16), ('bidirectional', BF16)])
def test_next_item_eval_batch_ranks_at_the_given_rows(ops, attention, dtype):
    """a DeviceCloze next-item evaluation batch: one compact row per sequence at its last input; a sequence with nothing in front of
    its target has none (an empty range).  predict_topk(flat_idx=, row_offsets=, exclude=) takes the masked-query route and ranks
    as the call without row_offsets (full last layer, rows gathered) on the clear rows."""
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    V, K = 60, 5
    g = np.random.default_rng(5)
    lens = np.array([9, 1, 14, 2, 1, 33, 5, 12, 3, 20, 1, 7])                  # 1: only the target, no row
    items = g.integers(0, V, int(lens.sum())).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dc = DeviceCloze(items, offsets, V=V, max_len=16)
    model = _build(V, 64, 2, 2, [32], dtype, 9, attention=attention)
    with torch.no_grad():
        model.head.output_layer.kernel.mul_(4.0)
    causal = attention == 'causal'
    n = 0
    for b in dc.next_item_eval_batches(6, split='test'):
        feats = {'asin': b['items']}
        seen = dc.history(b['target_seq_idx'], 'test')
        off = b['row_offsets'].cpu().numpy()
        assert (np.diff(off) == 0).any() and b['flat_idx'].shape[0] == int(off[-1]) < len(off) - 1
        kw = dict(labels=b['labels'], flat_idx=b['flat_idx'], exclude=seen)
        if dtype == BF16:
            kw['n_real_tokens'] = b['n_real_tokens']
        with _CountMQ(ops) as mq:
            want = model.predict_topk(feats, K, **kw)                            # no row_offsets: as today
            assert mq.calls == 0
            if causal:                                                           # the switch is off: row_offsets changes nothing
                same = model.predict_topk(feats, K, row_offsets=b['row_offsets'], **kw)
                assert mq.calls == 0 and all(torch.equal(x, y) for x, y in zip(same, want))
        prev = ops.mq_causal
        ops.mq_causal = causal
        try:
            with _CountMQ(ops) as mq:
                got = model.predict_topk(feats, K, row_offsets=b['row_offsets'], **kw)
                assert mq.calls == 1 and mq.last == ([True] if causal else [0])
                sc = model.score_candidates(feats, want[0].clamp(min=0), flat_idx=b['flat_idx'], row_offsets=b['row_offsets'],
                                            **({'n_real_tokens': b['n_real_tokens']} if dtype == BF16 else {}))
                assert mq.calls == 2 and bool(torch.isfinite(sc).all())
        finally:
            ops.mq_causal = prev
        # the clear rows, decided on the full-layer route's own rows (the history left out, as the ranking leaves it out)
        with torch.no_grad():
            rows, _ = model._masked_rows(feats, False, b['flat_idx'], pack=model._packed is not None, n_real_tokens=kw.get('n_real_tokens'))
            logits = model.head.logits(rows, out_fp32=True)[:, :V].float().cpu().numpy()
        ex = seen.cpu().numpy()
        for r in range(logits.shape[0]):
            drop = ex[r][(ex[r] >= 0) & (ex[r] != int(b['labels'][r]))]
            logits[r, drop] = -np.inf
        order = np.argsort(-logits, axis=1, kind='stable')[:, :K + 1]
        top = np.take_along_axis(logits, order, 1)
        clear = (top[:, :-1] - top[:, 1:] > 1e-3).all(1)
        assert clear.mean() > 0.5
        assert np.array_equal(want[0].cpu().numpy()[clear], order[:, :K][clear])
        assert np.array_equal(got[0].cpu().numpy()[clear], want[0].cpu().numpy()[clear])
        assert np.array_equal((got[1].cpu().numpy() > 0)[clear], (want[1].cpu().numpy() > 0)[clear])
        n += int(clear.sum())
    assert n > 4
