"""Attention-probability dropout in the masked-query last-layer kernels (b4c_attn_mq_fwd_drop / b4c_attn_mq_bwd_drop) and the
route ops.mq_attn_dropout opens for a model that trains with attention_dropout_rate > 0.

The kernels see R compact query rows; the keep rule of include/b4c.h counts the query inside its sequence, so they take the
token row of every query row (q_rows) and must draw the masks the full layer draws for those rows:
b4c_attn_keep(seed, b, h, q_rows[r] - cu[b], k, H, max_len, rate).

Every kernel-level case runs bf16 with head depth 64 and 32 (the matrix-core kernels) and fp32 with head depth 64 (the VALU
kernels) on two layouts:
  packed  lens [70, 7, 33, 1] (three key tiles, the last partial; a one-key sequence; the pitch is max_len = 70), query counts
          [33, 0, 10, 1] (33: a second query pass of the matrix-core kernels and a third chunk of the VALU ones; 0: an item without
          queries);
  dense   B = 2, S = 40, trailing padded keys (37 and 12 real tokens), query counts [33, 10].
The query positions are not contiguous and include 0 and the last real position; one more query row, outside every
[q_offsets[b], q_offsets[b+1]) range, holds q_rows = -1 (the unused tail of the sync-free form)."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_dropout_ref as ref  # noqa: E402

H = 2
KERNELS = [(torch.bfloat16, 64), (torch.bfloat16, 32), (torch.float32, 64)]
LAYOUTS = ['packed', 'dense']


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops
    return ops


class Layout:
    """host description of one of the two layouts; device copies of the index operands"""

    def __init__(self, kind):
        if kind == 'packed':
            self.pitch = [70, 7, 33, 1]
            self.real = list(self.pitch)
            self.pos = [[0] + list(range(2, 64, 2)) + [69], [], [0, 3, 4, 9, 14, 20, 21, 27, 30, 32], [0]]
            self.S_arg = 70
        else:
            self.pitch = [40, 40]
            self.real = [37, 12]
            self.pos = [[p for p in range(37) if p not in (5, 11, 17, 23)], [0, 2, 3, 5, 6, 7, 8, 9, 10, 11]]
            self.S_arg = 40
        self.packed = kind == 'packed'
        self.B = len(self.pitch)
        self.cu = np.concatenate([[0], np.cumsum(self.pitch)]).astype(np.int32)
        self.counts = [len(p) for p in self.pos]
        assert self.counts == ([33, 0, 10, 1] if self.packed else [33, 10])
        assert all(p[0] == 0 and p[-1] == n - 1 for p, n in zip(self.pos, self.real) if p)
        self.moff = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.T, self.R = int(self.cu[-1]), int(self.moff[-1]) + 1           # + the unused slot
        rows = [int(self.cu[b]) + p for b in range(self.B) for p in self.pos[b]]
        self.q_rows = np.asarray(rows + [-1], dtype=np.int32)
        self.seq_of = [b for b in range(self.B) for _ in self.pos[b]]       # sequence of every used query row
        pad = np.zeros(self.T, dtype=np.uint8)
        for b in range(self.B):
            pad[self.cu[b] + self.real[b]:self.cu[b + 1]] = 1
        self.pad = torch.from_numpy(pad)
        self.cu_d = torch.from_numpy(self.cu).cuda()
        self.moff_d = torch.from_numpy(self.moff).cuda()
        self.q_rows_d = torch.from_numpy(self.q_rows).cuda()
        self.kp_d = None if self.packed else self.pad.cuda()                # packed: every token is real, no key bytes


@pytest.fixture(scope='module')
def layouts(ops):
    return {k: Layout(k) for k in LAYOUTS}


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _operands(lay, dtype, dh, seed):
    """random q | k | v of every token, dO of every query row; q of a query row = the q columns of its token row"""
    g = torch.Generator().manual_seed(seed)
    d = H * dh
    qkv = (torch.randn(lay.T, 3 * d, generator=g) * 0.8).to(dtype)
    do = torch.randn(lay.R, d, generator=g).to(dtype)
    q = qkv[torch.from_numpy(lay.q_rows).long().clamp(min=0), :d].contiguous()        # (the unused slot: any row)
    kv = qkv[:, d:].contiguous()
    return qkv, q, kv, do


# ---- 1. the outputs are the masks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', LAYOUTS)
@pytest.mark.parametrize('dtype,dh', KERNELS)
def test_outputs_are_the_masks(ops, layouts, dtype, dh, kind):
    """q = 0: P is uniform over the real keys.  V row k = one-hot at column k - k0 for the keys k0 .. k0 + dh of a pass, so o of a
    pass IS the keep bits of those keys; dO row = one-hot at the row's number inside its sequence, so dV is their transpose.
    No tolerance: the bits equal b4c_attn_keep(seed, b, h, q_rows[r] - cu[b], k, H, max_len, rate) for every (row, head, key)."""
    from bert4clickpath_amd import _lib as L
    lay = layouts[kind]
    rate, seed = 0.25, 0xA11CE + dh + lay.B
    d, R, T, S_arg = H * dh, lay.R, lay.T, lay.S_arg
    lib = L.lib()
    want = np.zeros((R, H, S_arg), dtype=bool)
    for r, b in enumerate(lay.seq_of):
        qpos = int(lay.q_rows[r] - lay.cu[b])
        for h in range(H):
            for k in range(lay.real[b]):
                want[r, h, k] = bool(lib.b4c_attn_keep(seed, b, h, qpos, k, H, S_arg, rate))
    q = torch.zeros(R, d, dtype=dtype, device='cuda')
    p, st, dt = ops._p, ops._st(), ops.dt_code(dtype)
    got = np.zeros((R, H, S_arg), dtype=bool)
    lse = None
    for k0 in range(0, S_arg, dh):
        kv = torch.zeros(T, 2 * d, dtype=dtype)
        for b in range(lay.B):
            for k in range(k0, min(k0 + dh, lay.pitch[b])):
                for h in range(H):
                    kv[lay.cu[b] + k, d + h * dh + k - k0] = 1.0
        kv = kv.cuda()
        o = torch.zeros(R, d, dtype=dtype, device='cuda')
        lse = torch.zeros(R, H, dtype=torch.float32, device='cuda')
        L.check(lib.b4c_attn_mq_fwd_drop(p(q), d, p(kv), 2 * d, p(lay.kp_d), p(lay.cu_d), p(lay.moff_d), p(o), d, p(lse), lay.B, S_arg,
                                         H, dh, dt, st, p(lay.q_rows_d), rate, seed), 'attn_mq_fwd_drop')
        n = min(dh, S_arg - k0)
        got[:, :, k0:k0 + n] = (o.float().cpu().view(R, H, dh) != 0).numpy()[:, :, :n]
    assert np.array_equal(got, want)
    assert not got[-1].any()                                                  # the unused slot: never written
    kept = np.concatenate([want[r, :, :lay.real[b]].ravel() for r, b in enumerate(lay.seq_of)])
    assert 0.6 < float(kept.mean()) < 0.9                                     # (rate 0.25)
    # lse is that of the undropped softmax: log(number of real keys) for uniform probabilities
    for r, b in enumerate(lay.seq_of):
        assert float((lse[r].cpu() - math.log(lay.real[b])).abs().max()) < 1e-4
    # backward: dV[k][c] = P~[query g0 + c of the sequence][k]; dQ and dK are exactly zero (k = 0, and q = 0)
    zkv = torch.zeros(T, 2 * d, dtype=dtype, device='cuda')
    zo = torch.zeros(R, d, dtype=dtype, device='cuda')
    gotb = np.zeros((R, H, S_arg), dtype=bool)
    for g0 in range(0, max(lay.counts), dh):
        do = torch.zeros(R, d, dtype=dtype)
        for r, b in enumerate(lay.seq_of):
            c = r - int(lay.moff[b]) - g0
            if 0 <= c < dh:
                for h in range(H):
                    do[r, h * dh + c] = 1.0
        dq, dkv = ops.attn_mq_bwd(q, zkv, lay.cu_d, lay.moff_d, zo, do.cuda(), lse, lay.B, S_arg, H, dh, lay.kp_d, lay.q_rows_d, rate, seed)
        assert not dq.any() and not dkv[:, :d].any()
        dv = (dkv[:, d:].float().cpu().view(T, H, dh) != 0).numpy()
        for r, b in enumerate(lay.seq_of):
            c = r - int(lay.moff[b]) - g0
            if 0 <= c < dh:
                gotb[r, :, :lay.pitch[b]] = dv[lay.cu[b]:lay.cu[b + 1], :, c].T
    assert np.array_equal(gotb, want)


# ---- 2. the same masks as the full layer ------------------------------------------------------------------------------------------
def _full_layer(ops, lay, qkv, dtype, dh, rate, seed):
    """o [T, d] and lse [B, H, S_arg] of the full layer's kernels (ops.attn_fwd) on the same q | k | v with the same seed.
    The packed layout of the full layer is bf16 only; in fp32 the packed sequences go through the dense kernels at the pitch
    max_len with their tails as padded keys -- the keep rule sees the same (b, h, q, k, S_arg), a padded key has p = 0 exactly."""
    if lay.packed and dtype == torch.float32:
        S = lay.S_arg
        dense = torch.zeros(lay.B * S, qkv.shape[1], dtype=dtype)
        pad = torch.ones(lay.B * S, dtype=torch.uint8)
        for b in range(lay.B):
            dense[b * S:b * S + lay.pitch[b]] = qkv[lay.cu[b]:lay.cu[b + 1]]
            pad[b * S:b * S + lay.pitch[b]] = 0
        o, lse = ops.attn_fwd(dense.cuda(), pad.cuda(), lay.B, S, H, dh, None, rate, seed)
        return torch.cat([o[b * S:b * S + lay.pitch[b]] for b in range(lay.B)]), lse
    return ops.attn_fwd(qkv.cuda(), lay.pad.cuda(), lay.B, lay.S_arg, H, dh, lay.cu_d if lay.packed else None, rate, seed)


@pytest.mark.parametrize('kind', LAYOUTS)
@pytest.mark.parametrize('dtype,dh', KERNELS)
def test_same_masks_as_the_full_layer(ops, layouts, dtype, dh, kind):
    """ops.attn_mq_fwd(..., q_rows, rate, seed) against the rows q_rows of ops.attn_fwd(..., rate=, seed=) on the same q | k | v.
    Bounds: those tests/test_gpu_mq.py::test_attn_mq_kernels_match_fp64 holds the masked-query kernels to -- o within
    2e-5 (fp32) / 1.5e-2 (bf16) of max(1, max|o|), lse within 1e-4 / 2e-2 -- unwidened.  A mask that differed in one element
    would move o by p / (1 - rate), far outside them.
    Measured (MI355X): bf16, all four cases: o and lse bit-identical (the two kernels share the tile arithmetic); fp32 packed
    max|do| 3.6e-7, max|dlse| 9.5e-7; fp32 dense max|do| 4.8e-7, max|dlse| 9.5e-7."""
    lay = layouts[kind]
    rate, seed = 0.2, 0xD0D0 + dh + lay.T
    qkv, q, kv, _ = _operands(lay, dtype, dh, 7 + dh + lay.T)
    o_full, lse_full = _full_layer(ops, lay, qkv, dtype, dh, rate, seed)
    o, lse = ops.attn_mq_fwd(q.cuda(), kv.cuda(), lay.cu_d, lay.moff_d, lay.B, lay.S_arg, H, dh, lay.kp_d, lay.q_rows_d, rate, seed)
    used = torch.from_numpy(lay.q_rows[:-1]).long()
    want_o = o_full.double().cpu()[used]
    want_l = torch.stack([lse_full[b, :, int(lay.q_rows[r] - lay.cu[b])] for r, b in enumerate(lay.seq_of)]).double().cpu()
    e_o = float((o[:-1].double().cpu() - want_o).abs().max())
    e_l = float((lse[:-1].double().cpu() - want_l).abs().max())
    print('mq attention dropout against the full layer %s dh=%d %s: max|do| %.3e (max|o| %.3f)  max|dlse| %.3e'
          % (dtype, dh, kind, e_o, float(want_o.abs().max()), e_l))
    tol = 2e-5 if dtype == torch.float32 else 1.5e-2
    assert e_o < tol * max(1.0, float(want_o.abs().max()))
    assert e_l < (1e-4 if dtype == torch.float32 else 2e-2)
    assert not o[-1].any() and not lse[-1].any()                              # the unused slot
    # the dropped forward differs from the undropped one; lse does not
    o0, lse0 = ops.attn_mq_fwd(q.cuda(), kv.cuda(), lay.cu_d, lay.moff_d, lay.B, lay.S_arg, H, dh, lay.kp_d)
    assert not torch.equal(o0, o) and torch.equal(lse0, lse)


# ---- 3. float64 parity, forward and backward ------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', LAYOUTS)
@pytest.mark.parametrize('dtype,dh', KERNELS)
def test_matches_fp64_with_the_regenerated_mask(ops, layouts, dtype, dh, kind):
    """bounds: those of tests/test_gpu_attn_dropout.py::test_matches_fp64_with_the_regenerated_mask (o 1.2e-2, gradients 2.5e-2
    relative L2 -- here dq and dkv each --, lse 3e-2), unwidened; the mask is regenerated on the host (ops.attn_keep_mask)"""
    lay = layouts[kind]
    rate, seed = 0.2, 0xFACE + dh + lay.T
    d = H * dh
    _, q, kv, do = _operands(lay, dtype, dh, 11 + dh + lay.T)
    keep = ops.attn_keep_mask(seed, lay.B, H, lay.S_arg, rate)
    q64 = q.double().requires_grad_(True)
    kv64 = kv.double().requires_grad_(True)
    outs, lses = [], []
    for b in range(lay.B):
        if not lay.pos[b]:
            continue
        t0, t1, r0, r1 = int(lay.cu[b]), int(lay.cu[b + 1]), int(lay.moff[b]), int(lay.moff[b + 1])
        n = t1 - t0
        qq = q64[r0:r1].view(r1 - r0, H, dh).permute(1, 0, 2)
        kk = kv64[t0:t1, :d].reshape(n, H, dh).permute(1, 0, 2)
        vv = kv64[t0:t1, d:].reshape(n, H, dh).permute(1, 0, 2)
        neg = lay.pad[t0:t1].double()[None, None, :] * -1e9
        ob, lb = ref.attention(qq, kk, vv, neg, keep[b][:, lay.pos[b], :n], rate)
        outs.append(ob.permute(1, 0, 2).reshape(r1 - r0, d))
        lses.append(lb.t())
    o_ref, lse_ref = torch.cat(outs), torch.cat(lses).detach()
    (o_ref * do[:-1].double()).sum().backward()
    dev = 'cuda'
    qd, kvd, dod = q.to(dev), kv.to(dev), do.to(dev)
    o, lse = ops.attn_mq_fwd(qd, kvd, lay.cu_d, lay.moff_d, lay.B, lay.S_arg, H, dh, lay.kp_d, lay.q_rows_d, rate, seed)
    dq, dkv = ops.attn_mq_bwd(qd, kvd, lay.cu_d, lay.moff_d, o, dod, lse, lay.B, lay.S_arg, H, dh, lay.kp_d, lay.q_rows_d, rate, seed)
    again = ops.attn_mq_bwd(qd, kvd, lay.cu_d, lay.moff_d, o, dod, lse, lay.B, lay.S_arg, H, dh, lay.kp_d, lay.q_rows_d, rate, seed)
    e_o, e_q, e_kv = rel_err(o[:-1], o_ref.detach()), rel_err(dq[:-1], q64.grad[:-1]), rel_err(dkv, kv64.grad)
    e_l = float((lse[:-1].double().cpu() - lse_ref).abs().max())
    print('mq attention dropout against fp64 %s dh=%d %s: rel_err(o) %.3e  rel_err(dq) %.3e  rel_err(dkv) %.3e  |dlse| %.3e'
          % (dtype, dh, kind, e_o, e_q, e_kv, e_l))
    assert e_o < 1.2e-2
    assert e_l < 3e-2
    assert e_q < 2.5e-2 and e_kv < 2.5e-2
    assert torch.equal(again[0], dq) and torch.equal(again[1], dkv)
    assert not dq[-1].any()                                                   # the unused slot
    # a token row that no query reads: exactly zero
    for b in range(lay.B):
        if not lay.pos[b]:
            assert float(dkv[int(lay.cu[b]):int(lay.cu[b + 1])].abs().max()) == 0.0
    if lay.packed:
        assert lay.counts[1] == 0


# ---- 4. rate 0 is the old entry point; 5. bad arguments ----------------------------------------------------------------------------
def _raw(ops, lay, dtype, dh, name, q, kv, o, lse, do=None, dq=None, dkv=None, tail=()):
    """one raw call of b4c_attn_mq_{fwd,bwd}[_drop]; tail = (q_rows, rate, seed) for the _drop form"""
    from bert4clickpath_amd import _lib as L
    p, st, dt, d = ops._p, ops._st(), ops.dt_code(dtype), H * dh
    head = (p(q), d, p(kv), 2 * d, p(lay.kp_d), p(lay.cu_d), p(lay.moff_d), p(o), d)
    if 'fwd' in name:
        args = head + (p(lse), lay.B, lay.S_arg, H, dh, dt, st)
    else:
        args = head + (p(do), d, p(lse), p(dq), d, p(dkv), 2 * d, lay.B, lay.S_arg, H, dh, dt, st)
    if tail:
        args += (p(tail[0]), tail[1], tail[2])
    return getattr(L.lib(), name)(*args)


@pytest.mark.parametrize('kind', LAYOUTS)
@pytest.mark.parametrize('dtype,dh', KERNELS)
def test_rate_zero_is_the_old_entry_point(ops, layouts, dtype, dh, kind):
    lay = layouts[kind]
    _, q, kv, do = _operands(lay, dtype, dh, 23 + dh + lay.T)
    q, kv, do = q.cuda(), kv.cuda(), do.cuda()
    d = H * dh

    def run(fwd, bwd, tail):
        o = torch.zeros(lay.R, d, dtype=dtype, device='cuda')
        lse = torch.zeros(lay.R, H, dtype=torch.float32, device='cuda')
        dq, dkv = torch.zeros_like(o), torch.full_like(kv, float('nan'))
        assert _raw(ops, lay, dtype, dh, fwd, q, kv, o, lse, tail=tail) == 0
        assert _raw(ops, lay, dtype, dh, bwd, q, kv, o, lse, do, dq, dkv, tail=tail) == 0
        torch.cuda.synchronize()
        return o, lse, dq, dkv
    old = run('b4c_attn_mq_fwd', 'b4c_attn_mq_bwd', ())
    assert bool(torch.isfinite(old[3]).all())
    for q_rows in (None, lay.q_rows_d):                   # the seed is ignored at rate 0
        new = run('b4c_attn_mq_fwd_drop', 'b4c_attn_mq_bwd_drop', (q_rows, 0.0, 12345))
        for a, b in zip(old, new):
            assert torch.equal(a, b)


@pytest.mark.parametrize('dtype,dh', KERNELS)
def test_ops_at_rate_zero_is_the_old_entry_point(ops, layouts, dtype, dh):
    """ops.attn_mq_fwd / attn_mq_bwd always call the _drop entry points; at rate 0 (with and without q_rows) their results are, bit
    for bit, those of raw calls of b4c_attn_mq_fwd / b4c_attn_mq_bwd"""
    lay = layouts['packed']
    _, q, kv, do = _operands(lay, dtype, dh, 29 + dh + lay.T)
    q, kv, do = q.cuda(), kv.cuda(), do.cuda()
    o = torch.zeros(lay.R, H * dh, dtype=dtype, device='cuda')
    lse = torch.zeros(lay.R, H, dtype=torch.float32, device='cuda')
    dq, dkv = torch.zeros_like(o), torch.full_like(kv, float('nan'))
    assert _raw(ops, lay, dtype, dh, 'b4c_attn_mq_fwd', q, kv, o, lse) == 0
    assert _raw(ops, lay, dtype, dh, 'b4c_attn_mq_bwd', q, kv, o, lse, do, dq, dkv) == 0
    for q_rows in (None, lay.q_rows_d):
        o1, lse1 = ops.attn_mq_fwd(q, kv, lay.cu_d, lay.moff_d, lay.B, lay.S_arg, H, dh, lay.kp_d, q_rows)
        dq1, dkv1 = ops.attn_mq_bwd(q, kv, lay.cu_d, lay.moff_d, o1, do, lse1, lay.B, lay.S_arg, H, dh, lay.kp_d, q_rows)
        torch.cuda.synchronize()
        for a, b in ((o, o1), (lse, lse1), (dq, dq1), (dkv, dkv1)):
            assert torch.equal(a, b)


@pytest.mark.parametrize('dtype,dh', KERNELS)
def test_bad_arguments_write_nothing(ops, layouts, dtype, dh):
    from bert4clickpath_amd import _lib as L
    lay = layouts['packed']
    _, q, kv, do = _operands(lay, dtype, dh, 31 + dh)
    q, kv, do = q.cuda(), kv.cuda(), do.cuda()
    d = H * dh
    o = torch.full((lay.R, d), 7.0, dtype=dtype, device='cuda')
    lse = torch.full((lay.R, H), 7.0, dtype=torch.float32, device='cuda')
    dq, dkv = torch.full_like(o, 7.0), torch.full_like(kv, 7.0)
    for q_rows, rate, what in ((lay.q_rows_d, 1.0, b'dropout rate'), (lay.q_rows_d, -0.1, b'dropout rate'), (None, 0.2, b'q_rows')):
        for name in ('b4c_attn_mq_fwd_drop', 'b4c_attn_mq_bwd_drop'):
            rc = _raw(ops, lay, dtype, dh, name, q, kv, o, lse, do, dq, dkv, tail=(q_rows, rate, 5))
            assert rc == L._C['B4C_EINVAL'] and what in L.lib().b4c_last_error()
    torch.cuda.synchronize()
    for t in (o, lse, dq, dkv):
        assert bool((t == 7.0).all())


# ---- 6. the model -------------------------------------------------------------------------------------------------------------------
V, D, S, B = 500, 128, 32, 8          # the small model and batch of tests/test_gpu_attn_dropout.py


def _model(dtype, dropout, a_rate=0.2, seed=3):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(seed)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': D}, SoftMaxHead([128, 64], V),
                               value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, dropout_rate=dropout,
                               compute_dtype=dtype, attention_dropout_rate=a_rate)
    return m.cuda()


def _batch(seed=21):
    from bert4clickpath_amd import input_pipeline
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=seed, min_len=3)
    ids = torch.from_numpy(b['ids'])
    return {'asin': ids[:, 2:S - 1].contiguous().cuda()}, torch.from_numpy(b['labels_padded']).cuda(), int((b['ids'] != 0).sum())


class _CountMQ:
    """counts the passes that take the masked-query last layer (the recorder of tests/test_gpu_attn_dropout.py)"""

    def __init__(self, ops):
        self.ops, self.calls, self.rates = ops, 0, []

    def __enter__(self):
        self._orig = self.ops.MQAttnBlockFn
        rec = self

        class Noting(self._orig):
            @staticmethod
            def apply(*a, **k):
                rec.calls += 1
                rec.rates.append(a[-2])
                return rec._orig.apply(*a, **k)
        self.ops.MQAttnBlockFn = Noting
        return self

    def __exit__(self, *exc):
        self.ops.MQAttnBlockFn = self._orig


def _step(model, feats, labels, n_real):
    model.zero_grad()
    kw = {'n_real_tokens': n_real} if n_real is not None else {}
    loss = model.cloze_loss(feats, labels, training=True, max_masked_per_row=10, **kw)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_model_switch_on_against_off(ops, dtype):
    """One training step with attention_dropout_rate = 0.2 and the same seeds, ops.mq_attn_dropout on against off: the last layer at
    the [MASK] rows with the masks of those rows against the full last layer and its gathered rows.  Bounds: those of
    tests/test_gpu_mq.py for "masked-query against full layer" -- fp32 (dense) loss 2e-6, gradients 2e-4 of the largest entry;
    bf16 (packed) loss 3e-3, gradients 0.08 -- unwidened.
    The residual dropout rate is 0 here, as in those tests: the last layer's residual masks are indexed by the row of the tensor
    they drop, R compact rows on one route and T token rows on the other, so with a rate they are different draws on the two
    routes (at every attention rate, 0 included).  The attention masks are indexed by (b, h, q, k) and are the same."""
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    feats, labels, n_real = _batch()
    if dtype == torch.float32:
        n_real = None                                      # fp32: the dense layout
    model = _model(dtype, 0.0)
    res, prev = {}, ops.mq_attn_dropout
    try:
        for on in (True, False):
            ops.mq_attn_dropout = on
            with _CountMQ(ops) as mq:
                T.set_dropout_seed(5)
                res[on] = _step(model, feats, labels, n_real)
                draws = T.dropout_seeds.counter
                assert mq.calls == (1 if on else 0)        # the masked-query block ran in the training pass only with the switch
                assert mq.rates == ([0.2] if on else [])
            res[on] += (draws,)
            assert (model._packed is not None) == (dtype == torch.bfloat16)
    finally:
        ops.mq_attn_dropout = prev
    (la, ga, da), (lb, gb, db) = res[True], res[False]
    assert da == db                                        # the route does not move the seed stream
    print('model %s: loss on %.8f off %.8f' % (dtype, float(la), float(lb)))
    if dtype == torch.float32:
        assert abs(float(la) - float(lb)) < 2e-6 * abs(float(lb))
        for n in ga:
            assert _rel(ga[n], gb[n]) < 2e-4 or float(gb[n].abs().max()) < 1e-7, n
    else:
        assert abs(float(la) - float(lb)) < 3e-3 * abs(float(lb))
        for n in ga:
            if float(gb[n].float().norm()) < 1e-9 or n.endswith('mha.wk.bias'):
                continue
            assert _rel(ga[n], gb[n]) < 0.08, n
    # the attention masks are in the step: rate 0 gives another loss
    model0 = _model(dtype, 0.0, a_rate=0.0)
    T.set_dropout_seed(5)
    assert float(_step(model0, feats, labels, n_real)[0]) != float(la)


def test_model_bf16_packed_checkpoint_resume(ops, tmp_path):
    """two optimizer steps with the switch on, a checkpoint, the third step; a fresh model and optimizer restored from the
    checkpoint repeat the third step bit for bit (residual dropout 0.1, attention dropout 0.2, the packed layout)"""
    from bert4clickpath_amd import checkpoint, optim
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    feats, labels, n_real = _batch()
    prev = ops.mq_attn_dropout
    ops.mq_attn_dropout = True
    try:
        model = _model(torch.bfloat16, 0.1)
        opt = optim.Adam(model.parameters())
        T.set_dropout_seed(31)
        with _CountMQ(ops) as mq:
            for _ in range(2):
                loss, _ = _step(model, feats, labels, n_real)
                opt.step()
            assert mq.calls == 2 and model._packed is not None and bool(torch.isfinite(loss))
        path = checkpoint.save_checkpoint(os.path.join(str(tmp_path), 'ckpt-mq-attn-drop'), model, opt, epoch=1)
        feats3, labels3, n_real3 = _batch(seed=22)
        loss3, grads3 = _step(model, feats3, labels3, n_real3)
        other = _model(torch.bfloat16, 0.1, seed=99)
        opt2 = optim.Adam(other.parameters())
        T.set_dropout_seed(1)
        checkpoint.load_checkpoint(path, other, opt2)
        with _CountMQ(ops) as mq:
            loss3r, grads3r = _step(other, feats3, labels3, n_real3)
            assert mq.calls == 1
        assert torch.equal(loss3, loss3r)
        for n in grads3:
            assert torch.equal(grads3[n], grads3r[n]), n
    finally:
        ops.mq_attn_dropout = prev
