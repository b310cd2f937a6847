"""The id sort, the sorted embedding scatter (both forms) and the batched weight re-pack, through the raw entry points, on the
sizes at which their kernels change path: the sort's 4096-key chunk, its one / two / three 8-bit passes and the scan launch it
takes past 256 chunks; the scatter's 64-entry ranges, its 8-entry batches and its 128-column passes; the re-pack's 64 x 64 tile.
Integer-valued gradients with scale 1 make every correct sum exact, so the scatter is compared with index_add_ bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _lib():
    from bert4clickpath_amd import _lib as LB
    return LB


def _call(name, *args):
    LB = _lib()
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    rc = getattr(LB.lib(), name)(*conv, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, LB.lib().b4c_last_error().decode()


def _dt(dtype):
    LB = _lib()
    return LB.F32 if dtype == F32 else LB.BF16


# ---------------------------------------------------------------------------------------------------------------- sort
def _sort(ids, n_rows):
    n = ids.numel()
    need = int(_lib().lib().b4c_sort_ids_workspace_bytes(n, n_rows))
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    order = torch.full((n,), -7, dtype=torch.int32, device='cuda')
    _call('b4c_sort_ids', ids, n, n_rows, order, ws, need)
    return order


def _id_patterns(n, n_rows, g):
    yield 'all equal', torch.full((n,), n_rows // 2, dtype=torch.int64)
    yield 'all distinct', torch.randperm(n, generator=g)                              # clamped into the table where n > n_rows
    mixed = torch.randint(0, n_rows, (n,), generator=g)
    mixed[::3] = -1 - torch.arange(0, n, 3)                                           # below the table: row 0
    mixed[1::5] = n_rows + torch.arange(0, n - 1, 5) * 1000003                        # past it (and past 2^32): the last row
    yield 'out of range', mixed


# 4095 / 4096 / 8193: around the chunk of one workgroup; 2^20 + 1: the first size with more than 256 chunks (scan launch)
@pytest.mark.parametrize('n_rows', [2, 255, 256, 257, 65536, 65537])
def test_sort_is_the_stable_argsort_of_the_clamped_ids(n_rows):
    g = torch.Generator().manual_seed(n_rows)
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193):
        for what, ids in _id_patterns(n, n_rows, g):
            ids = ids.cuda()
            want = torch.sort(ids.clamp(0, n_rows - 1), stable=True)[1].to(torch.int32)
            assert torch.equal(_sort(ids, n_rows), want), (n, n_rows, what)


@pytest.mark.parametrize('n_rows', [257, 65537])
def test_sort_past_256_chunks(n_rows):
    n = (1 << 20) + 1
    g = torch.Generator().manual_seed(n_rows)
    ids = (torch.exp(torch.rand(n, generator=g) * np.log(n_rows + 1.0)) - 1).long()   # log-uniform: a few very hot rows
    ids[::97] = -5
    ids[1::101] = n_rows + 3
    ids = ids.cuda()
    want = torch.sort(ids.clamp(0, n_rows - 1), stable=True)[1].to(torch.int32)
    assert torch.equal(_sort(ids, n_rows), want)


# ------------------------------------------------------------------------------------------------------------- scatter
def _scatter(form, ids_list, tables, dims, dout, scale, rate, seed, dtype):
    """tables += the sorted scatter of dout (one launch of `form`), in place"""
    n = len(dims)
    T, d = dout.shape
    clamped = [i.clamp(0, t.shape[0] - 1) for i, t in zip(ids_list, tables)]
    order = [torch.sort(c, stable=True)[1].to(torch.int32) for c in clamped]
    ia = (ctypes.c_void_p * n)(*[i.data_ptr() for i in ids_list])
    oa = (ctypes.c_void_p * n)(*[o.data_ptr() for o in order])
    ta = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tables])
    da = (ctypes.c_int * n)(*dims)
    ra = (ctypes.c_int64 * n)(*[t.shape[0] for t in tables])
    if form == 'sorted':
        _call('b4c_embed_concat_pe_bwd_sorted', n, ia, oa, ta, da, ra, scale, dout, d, 1, T, d, rate, seed, _dt(dtype))
    else:
        need = int(_lib().lib().b4c_embed_concat_pe_bwd_sorted_workspace_bytes(n, da, 1, T))
        ws = torch.full((max(need, 1),), 0xFF, dtype=torch.uint8, device='cuda')       # NaN bit patterns: nothing stale may be read
        _call('b4c_embed_concat_pe_bwd_sorted_ws', n, ia, oa, ta, da, ra, scale, dout, d, 1, T, d, rate, seed, ws, need, _dt(dtype))
    return clamped


def _scatter_ids(T, rows, g):
    yield 'one id', torch.full((T,), rows - 2, dtype=torch.int64)                      # fills every 64-entry range
    yield 'all distinct', torch.randperm(rows, generator=g)[:T]
    hot = torch.randperm(rows, generator=g)[:T]                                        # the smallest id, then singletons
    hot[torch.randperm(T, generator=g)[:(2 * T + 2) // 3]] = 0
    yield 'hot id then singletons', hot
    wild = torch.randint(0, rows, (T,), generator=g)
    wild[::2] = -3 - torch.arange(0, T, 2)
    wild[1::4] = rows + torch.arange(0, T - 1, 4) * 7
    yield 'out of range', wild


SCATTER_T = (1, 63, 64, 65, 129, 4097)


@pytest.mark.parametrize('form', ['sorted', 'sorted_ws'])
@pytest.mark.parametrize('dims', [(64, 64), (36,)], ids=['two features of 64', 'one feature of 36'])
def test_scatter_of_integers_is_index_add_exactly(form, dims):
    g = torch.Generator().manual_seed(sum(dims))
    d = sum(dims)
    for T in SCATTER_T:
        rows = T + 5
        for dtype in (F32, BF16):
            dout = torch.randint(-8, 9, (T, d), generator=g).to(dtype).cuda()
            for what, ids0 in _scatter_ids(T, rows, g):
                ids = [ids0.cuda()] + [ids0.flip(0).contiguous().cuda() for _ in dims[1:]]
                start = [torch.randint(-4, 5, (rows, k), generator=g).float().cuda() for k in dims]      # accumulate, not overwrite
                tabs = [s.clone() for s in start]
                clamped = _scatter(form, ids, tabs, dims, dout, 1.0, 0.0, 0, dtype)
                off = 0
                for f, k in enumerate(dims):
                    want = start[f].clone().index_add_(0, clamped[f], dout[:, off:off + k].float())
                    assert torch.equal(tabs[f], want), (form, dims, T, dtype, what, f)
                    off += k
                if form == 'sorted_ws':
                    again = [s.clone() for s in start]
                    _scatter(form, ids, again, dims, dout, 1.0, 0.0, 0, dtype)
                    assert all(torch.equal(a, b) for a, b in zip(again, tabs)), (dims, T, dtype, what)


@pytest.mark.parametrize('form', ['sorted', 'sorted_ws'])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
def test_scatter_dropout_follows_the_keep_mask(form, dtype):
    """rate 0.1: element (t, c) counts iff ops.keep_mask keeps t * d + c, times fp32(1 / (1 - rate)).  The factor is not a power of
    two, so the sums round: a row that n entries reach is n fused multiply-adds (fp32, in one fixed order) and one add into the
    table, each off by at most 2^-24 of a partial sum, and a partial sum is at most the sum of the magnitudes: the bound is
    (n + 2) * 2^-24 * (|start| + sum |g| * mul) per element -- nothing is taken from what the kernel returns."""
    from bert4clickpath_amd import ops
    rate, seed = 0.1, 4242
    mul = float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate)))
    g = torch.Generator().manual_seed(7)
    for dims in ((64, 64), (36,), (6, 10)):       # (6, 10): a feature that starts at column 6 hashes per lane, not per lane pair
        d = sum(dims)
        for T in SCATTER_T:
            rows = T + 5
            keep = torch.from_numpy(ops.keep_mask(seed, T * d, rate).reshape(T, d)).cuda()
            dout = torch.randint(-8, 9, (T, d), generator=g).to(dtype).cuda()
            kept = dout.double() * keep * mul
            for what, ids0 in _scatter_ids(T, rows, g):
                ids = [ids0.cuda()] + [ids0.flip(0).contiguous().cuda() for _ in dims[1:]]
                start = [torch.randint(-4, 5, (rows, k), generator=g).float().cuda() for k in dims]
                tabs = [s.clone() for s in start]
                clamped = _scatter(form, ids, tabs, dims, dout, 1.0, rate, seed, dtype)
                off = 0
                for f, k in enumerate(dims):
                    want = start[f].double().index_add_(0, clamped[f], kept[:, off:off + k])
                    mag = start[f].double().abs().index_add_(0, clamped[f], kept[:, off:off + k].abs())
                    cnt = torch.zeros(rows, dtype=torch.float64, device='cuda').index_add_(0, clamped[f], torch.ones(T, dtype=torch.float64, device='cuda'))
                    bound = (cnt[:, None] + 2) * 2.0 ** -24 * mag
                    err = (tabs[f].double() - want).abs()
                    assert bool((err <= bound).all()), (form, dims, T, what, f, float((err - bound).max()))
                    # a dropped element contributes nothing: rows whose every contribution was dropped keep their start exactly
                    untouched = mag == start[f].double().abs()
                    assert torch.equal(tabs[f][untouched], start[f][untouched])
                    off += k
                if form == 'sorted_ws':
                    again = [s.clone() for s in start]
                    _scatter(form, ids, again, dims, dout, 1.0, rate, seed, dtype)
                    assert all(torch.equal(a, b) for a, b in zip(again, tabs)), (dims, T, what)


# ---------------------------------------------------------------------------------------------------------------- pack
def _desc_tensor(descs):
    LB = _lib()
    arr = (LB.PackDesc * len(descs))(*descs)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()


def _tiles(K, N):
    return ((K + 63) // 64) * ((N + 63) // 64)


def _rup8(x):
    return (x + 7) // 8 * 8


@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('K,N', [(1, 1), (7, 5), (64, 64), (65, 63), (128, 1003)])
def test_pack_is_the_transposed_conversion(K, N, dtype):
    LB = _lib()
    g = torch.Generator().manual_seed(K * 1000 + N)
    w, b = torch.randn(K, N, generator=g).cuda(), torch.randn(N, generator=g).cuda()
    Kp, Np = _rup8(K), _rup8(N)
    wt = torch.zeros(Np, Kp, dtype=dtype, device='cuda')
    wc = torch.zeros(Kp, Np, dtype=dtype, device='cuda')
    bd = torch.zeros(Np, device='cuda')
    dd = _desc_tensor([LB.PackDesc(w.data_ptr(), b.data_ptr(), wt.data_ptr(), wc.data_ptr(), bd.data_ptr(), K, N, Kp, Np, 0, 0)])
    _call('b4c_pack_weights_batched', dd, 1, _tiles(K, N), _dt(dtype))
    want_t = torch.zeros_like(wt)
    want_t[:N, :K] = w.t().contiguous().to(dtype)
    want_c = torch.zeros_like(wc)
    want_c[:K, :N] = w.to(dtype)
    want_b = torch.zeros_like(bd)
    want_b[:N] = b
    assert torch.equal(wt, want_t) and torch.equal(wc, want_c) and torch.equal(bd, want_b)      # padding rows and columns stay zero


@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'fp32'])
def test_pack_three_descriptors_of_unlike_size_and_column_offsets(dtype):
    """One launch: two kernels fused along N into one pair of copies (the second at col_off = 37, neither 4- nor 8-aligned), and a
    third, much larger matrix of its own that has no wc copy."""
    LB = _lib()
    g = torch.Generator().manual_seed(5)
    K, N1, N2 = 65, 37, 70
    w1, w2 = torch.randn(K, N1, generator=g).cuda(), torch.randn(K, N2, generator=g).cuda()
    b1, b2 = torch.randn(N1, generator=g).cuda(), torch.randn(N2, generator=g).cuda()
    Kp, Np = _rup8(K), _rup8(N1 + N2)
    wt = torch.zeros(Np, Kp, dtype=dtype, device='cuda')
    wc = torch.zeros(Kp, Np, dtype=dtype, device='cuda')
    bd = torch.zeros(Np, device='cuda')
    K3, N3 = 128, 1003
    w3, b3 = torch.randn(K3, N3, generator=g).cuda(), torch.randn(N3, generator=g).cuda()
    N3p = _rup8(N3)
    wt3 = torch.zeros(N3p, K3, dtype=dtype, device='cuda')
    bd3 = torch.zeros(N3p, device='cuda')
    descs = [LB.PackDesc(w2.data_ptr(), b2.data_ptr(), wt.data_ptr(), wc.data_ptr(), bd.data_ptr(), K, N2, Kp, Np, N1, 0),
             LB.PackDesc(w3.data_ptr(), b3.data_ptr(), wt3.data_ptr(), None, bd3.data_ptr(), K3, N3, K3, N3p, 0, 0),
             LB.PackDesc(w1.data_ptr(), b1.data_ptr(), wt.data_ptr(), wc.data_ptr(), bd.data_ptr(), K, N1, Kp, Np, 0, 0)]
    dd = _desc_tensor(descs)
    _call('b4c_pack_weights_batched', dd, 3, max(_tiles(K, N2), _tiles(K3, N3), _tiles(K, N1)), _dt(dtype))
    w12, b12 = torch.cat([w1, w2], 1), torch.cat([b1, b2])
    want_t = torch.zeros_like(wt)
    want_t[:N1 + N2, :K] = w12.t().contiguous().to(dtype)
    want_c = torch.zeros_like(wc)
    want_c[:K, :N1 + N2] = w12.to(dtype)
    want_b = torch.zeros_like(bd)
    want_b[:N1 + N2] = b12
    assert torch.equal(wt, want_t) and torch.equal(wc, want_c) and torch.equal(bd, want_b)
    want3 = torch.zeros_like(wt3)
    want3[:N3] = w3.t().contiguous().to(dtype)
    want_b3 = torch.zeros_like(bd3)
    want_b3[:N3] = b3
    assert torch.equal(wt3, want3) and torch.equal(bd3, want_b3)
