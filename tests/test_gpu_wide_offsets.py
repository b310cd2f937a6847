"""The vocabulary-wide kernels and the 2M-row table kernels past 2^31 elements (and 2^32 bytes), through the C ABI.

Every entry point forms addresses as row * ld + col.  Two forms of a case:

PITCH form, where ld is only a pitch (the kernel touches columns [0, width) of a row and nothing between rows): 10 rows at the
pitch LD = 2^29 + 128 elements -- views of one flat allocation (10.7 GB bf16, 21.5 GB fp32, a few KB of it touched).  Row 4
starts past 2^31 elements (bf16: past 2^32 bytes), row 8 past 2^32 elements.  Several operands of one call sit in the same
allocation at different column offsets ("slots").

DENSE form, where the kernel writes or reads the pad columns up to ld (softmax_rows, softmax_rows_bwd, sparse_ce_from_probs_bwd
and softmax_ce_fwd_bwd write zeros there) or has no pitch (the tables): the natural pitch and the smallest R with
R * ld > 2^31 + 64 * ld; tables of 2^23 + 64 rows x 256 fp32 (the byte boundaries 2^31 and 2^32 at rows 2^21 and 2^22, the
element boundary 2^31 at row 2^23).

Each case asserts (1) position independence bit for bit: the same call on a compact copy of the same rows gives torch.equal
outputs; (2) parity of the compact run with float64 within the bound of the entry point's existing parity test (cited at each
use); (3) nothing else moved: outputs start as NaN / -7 and every row is written, and in the pitch form a 4,096-element window
behind every row of every operand keeps its NaN; sampled untouched table rows keep their contents.  In the dense form the rows
compared are the first 64, every 97th, and every row from 64 before the 2^31-element row to the end: a wrapped offset moves
every row past the boundary, and all of those are compared.

b4c_gemm_nt and b4c_gemm_nt_softmax stage A and Bt with 32-bit buffer offsets inside a 128-row tile: a pitch of 2^29 + 128 is
refused there (B4C_EINVAL, include/b4c.h: 128 * ld must span less than 2^30 bytes), and the largest pitch below the limit is run on
a full tile; their C, gate and residual take the pitch."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from candidates_ref import rank_rows, topk_rows  # noqa: E402
from oracle import numpy_ref as nr  # noqa: E402

LD = (1 << 29) + 128        # a multiple of 128: every row 256-B aligned
ROWS = 10
SLOT = 8192                 # elements between two operands of one arena
WIN = 4096                  # sentinel window behind a row
NAN = float('nan')
F32, BF16 = torch.float32, torch.bfloat16
DT = [F32, BF16]


def _ids(dtype):
    return 'f32' if dtype == F32 else 'bf16'


def _need(nbytes):
    free, total = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip('needs %d bytes of device memory, %d free of %d' % (nbytes, free, total))


def _lib():
    from bert4clickpath_amd import _lib as L
    return L


def _call(name, *args):
    from bert4clickpath_amd import ops
    L = _lib()
    L.check(getattr(L.lib(), name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], ops._st()), name)


def _dt(dtype):
    from bert4clickpath_amd import ops
    return ops.dt_code(dtype)


def _rup8(n):
    return (n + 7) // 8 * 8


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device='cuda')


def _full(shape, value, dtype):
    return torch.full(shape, value, dtype=dtype, device='cuda')


def _compact(data, ld=None):
    """data [R][w] on a fresh tensor of pitch ld (default w rounded up to 8), the pad NaN"""
    R, w = data.shape
    t = _full((R, ld or _rup8(w)), NAN, data.dtype)
    t[:, :w] = data
    return t


class _Arena:
    """one flat allocation holding ROWS rows at the pitch LD; operand `slot` starts at column slot * SLOT"""

    def __init__(self, dtype, slots=4):
        n = (ROWS - 1) * LD + slots * SLOT
        _need(n * torch.empty(0, dtype=dtype).element_size() + (1 << 30))
        self.flat = torch.empty(n, dtype=dtype, device='cuda')
        self.used = []

    def rows(self, slot, width):
        return torch.as_strided(self.flat, (ROWS, width), (LD, 1), slot * SLOT)

    def put(self, slot, data):
        """data [ROWS][w] into the slot, NaN in the window behind every row"""
        w = data.shape[1]
        assert w + WIN <= SLOT
        v = self.rows(slot, w + WIN)
        v[:, w:] = NAN
        v[:, :w] = data
        self.used.append((slot, w))
        return self.rows(slot, w)

    def out(self, slot, w):
        """an output operand: NaN everywhere, window included"""
        self.rows(slot, w + WIN).fill_(NAN)
        self.used.append((slot, w))
        return self.rows(slot, w)

    def windows_intact(self):
        return all(bool(torch.isnan(self.rows(s, w + WIN)[:, w:]).all()) for s, w in self.used)


def _free(*tensors):
    """release the storages now -- a plain `del` would leave them to the views that a failed test's traceback keeps, and the
    next test would find the memory taken -- then the cache"""
    for t in tensors:
        if t is not None:
            t.untyped_storage().resize_(0)
    torch.cuda.empty_cache()


def _with_arena(dtype, body, slots=4):
    a = _Arena(dtype, slots)
    try:
        assert a.rows(0, 8)[4:].data_ptr() - a.flat.data_ptr() >= (1 << 31) * a.flat.element_size()
        body(a)
        assert a.windows_intact(), 'a window behind a row lost its sentinel'
    finally:
        _free(a.flat)


def _written(*ts):
    return all(not bool(torch.isnan(t).any()) for t in ts)


# ---------------------------------------------------------------------------------------------------------------------------
# pitch form: softmax and the losses on probabilities
# ---------------------------------------------------------------------------------------------------------------------------
# routes of b4c_softmax_rows (head.hip): bf16 with ld_out <= 65,536 in registers, everything else streaming; the output's pad
# columns are written, so the OUTPUT is compact here (its dense form: test_softmax_rows_dense) and the INPUT has the pitch
@pytest.mark.parametrize('V', [1000, 1003])
@pytest.mark.parametrize('dtype', DT, ids=['stream_f32', 'registers_bf16'])
def test_softmax_rows_pitch(dtype, V):
    def body(a):
        x = (_randn(_gen(V), ROWS, V) * 3).to(dtype)
        outs = []
        for src in (a.put(0, x), _compact(x)):
            y = _full((ROWS, _rup8(V)), NAN, dtype)
            _call('b4c_softmax_rows', src, src.stride(0), y, y.stride(0), ROWS, V, _dt(dtype))
            outs.append(y)
        assert _written(*outs) and torch.equal(outs[0], outs[1])
        assert not bool(outs[0][:, V:].any())                                   # pads are written as 0 (b4c.h)
        p64 = torch.softmax(x.double(), -1)
        # tests/test_gpu_kernels.py:365
        assert float((outs[1][:, :V].double() - p64).abs().max()) < (1e-6 if dtype == F32 else 4e-3)
    _with_arena(dtype, body)


# one kernel per dtype (elemwise.hip); probs and dprobs have the pitch, dlogits (pads written) is compact
@pytest.mark.parametrize('V', [1000, 1003])
@pytest.mark.parametrize('dtype', DT, ids=_ids)
def test_softmax_rows_bwd_pitch(dtype, V):
    def body(a):
        g = _gen(V + 1)
        p = torch.softmax(_randn(g, ROWS, V) * 3, -1).to(dtype)
        w = _randn(g, ROWS, V).to(dtype)
        outs = []
        for ps, ws in ((a.put(0, p), a.put(1, w)), (_compact(p), _compact(w))):
            dx = _full((ROWS, _rup8(V)), NAN, dtype)
            _call('b4c_softmax_rows_bwd', ps, ps.stride(0), ws, ws.stride(0), dx, dx.stride(0), ROWS, V, _dt(dtype))
            outs.append(dx)
        assert _written(*outs) and torch.equal(outs[0], outs[1]) and not bool(outs[0][:, V:].any())
        pd, wd = p.double(), w.double()
        ref = pd * (wd - (pd * wd).sum(-1, keepdim=True))
        # tests/test_gpu_round2.py:115 (1e-6 fp32, 2e-2 bf16, absolute)
        assert float((outs[1][:, :V].double() - ref).abs().max()) < (1e-6 if dtype == F32 else 2e-2)
    _with_arena(dtype, body)


# one kernel per dtype (head.hip), both variants; probs has the pitch
@pytest.mark.parametrize('variant', [0, 1], ids=['tf', 'plain'])
@pytest.mark.parametrize('V', [1000, 1003])
@pytest.mark.parametrize('dtype', DT, ids=_ids)
def test_sparse_ce_from_probs_pitch(dtype, V, variant):
    def body(a):
        g = _gen(V + 2)
        x = _randn(g, ROWS, V) * 3
        x[0, 5] = 40.0                                                        # most of row 0 under the 1e-7 clip
        p = torch.softmax(x, -1).to(dtype)
        labels = torch.randint(0, V, (ROWS,), generator=g, device='cuda')
        labels[0] = 5
        labf = labels.float()
        labf[3] = -1.0
        outs = []
        for ps in (a.put(0, p), _compact(p)):
            item, nval = _full((ROWS,), NAN, F32), torch.zeros(1, device='cuda')
            _call('b4c_sparse_ce_from_probs', ps, ps.stride(0), labf, item, nval, ROWS, V, variant, _dt(dtype))
            assert int(nval) == ROWS - 1
            outs.append(item)
        assert _written(*outs) and torch.equal(outs[0], outs[1])
        want = nr.sparse_categorical_crossentropy(labels.cpu().numpy(), p.double().cpu().numpy(), 'tf' if variant == 0 else 'plain')
        want[3] = 0.0
        # tests/test_gpu_kernels.py:377
        assert float(np.abs(outs[1].double().cpu().numpy() - want).max()) < (2e-5 if dtype == F32 else 2e-2)
    _with_arena(dtype, body)


# one kernel per dtype (elemwise.hip); probs has the pitch, dprobs (pads written) is compact
@pytest.mark.parametrize('variant', [0, 1], ids=['tf', 'plain'])
@pytest.mark.parametrize('dtype', DT, ids=_ids)
def test_sparse_ce_from_probs_bwd_pitch(dtype, variant):
    V = 1003

    def body(a):
        g = _gen(V + 3)
        x = _randn(g, ROWS, V) * 3
        x[0, 5] = 40.0
        p = torch.softmax(x, -1).to(dtype)
        labels = torch.randint(0, V, (ROWS,), generator=g, device='cuda')
        labels[0] = 5
        labf = labels.float()
        labf[3] = -1.0
        gs = torch.tensor([0.37], device='cuda')
        outs = []
        for ps in (a.put(0, p), _compact(p)):
            dp = _full((ROWS, _rup8(V)), NAN, dtype)
            _call('b4c_sparse_ce_from_probs_bwd', ps, ps.stride(0), labf, gs, dp, dp.stride(0), ROWS, V, variant, _dt(dtype))
            outs.append(dp)
        assert _written(*outs) and torch.equal(outs[0], outs[1]) and not bool(outs[0][:, V:].any())
        pd = p.double()
        onehot = torch.zeros_like(pd).scatter_(1, labels[:, None], 1.0)
        py = pd.gather(1, labels[:, None])
        if variant == 0:
            lo, hi = float(np.float32(1e-7)), float(np.float32(1.0) - np.float32(1e-7))      # the clip bounds as the fp32 kernels hold them
            S = pd.clamp(lo, hi).sum(-1, keepdim=True)
            u = ((pd >= lo) & (pd <= hi)).double()
            ref = u * (1.0 / S - onehot / py.clamp(lo, hi))
        else:
            ref = -onehot / py
        ref = ref * float(gs)
        ref[3] = 0.0
        err = float((outs[1][:, :V].double() - ref).abs().max()) / float(ref.abs().max())
        # tests/test_gpu_round2.py:109 for fp32; bf16: the result is rounded once to bf16 (2^-9 relative) behind the same fp32
        # arithmetic: 2^-8 of the largest entry
        assert err < (1e-4 if dtype == F32 else 2.0 ** -8), err
    _with_arena(dtype, body)


# ---------------------------------------------------------------------------------------------------------------------------
# pitch form: ranking on materialised scores (scores are only read: the pitch form throughout; the ids are compact [R][k])
# ---------------------------------------------------------------------------------------------------------------------------
def _topk_inputs(dtype, V, seed):
    g = _gen(seed)
    s = _randn(g, ROWS, V)
    s[1] = torch.randint(0, 4, (V,), generator=g, device='cuda').float()         # heavy ties -> lower index first
    s[9] = 0.5                                                                    # all equal, past 2^32 elements: the list kernel redoes it
    return s.to(dtype), torch.randint(0, V, (ROWS,), generator=g, device='cuda').int()


# routes of b4c_topk_rows_ws (head.hip): redo given -> threshold kernel (fp32: topk_rows_kernel, bf16: the register-resident
# kernel) and the list kernel for flagged rows; redo NULL (b4c_topk_rows) -> list kernel for every row
@pytest.mark.parametrize('V,k', [(1000, 5), (1003, 16)])
@pytest.mark.parametrize('route', ['threshold', 'lists'])
@pytest.mark.parametrize('dtype', DT, ids=_ids)
def test_topk_rows_pitch(dtype, route, V, k):
    def body(a):
        s, labels = _topk_inputs(dtype, V, V + k)
        _, want = nr.top_k(s.float().cpu().numpy(), k)
        labels[4] = int(want[4, min(2, k - 1)])
        outs = []
        for ss in (a.put(0, s), _compact(s)):
            idx, hit, ndcg = _full((ROWS, k), -7, torch.int32), _full((ROWS,), NAN, F32), _full((ROWS,), NAN, F32)
            redo = _full((ROWS,), -7, torch.int32)
            if route == 'threshold':
                _call('b4c_topk_rows_ws', ss, ss.stride(0), ROWS, V, k, idx, labels, hit, ndcg, redo, _dt(dtype))
            else:
                _call('b4c_topk_rows', ss, ss.stride(0), ROWS, V, k, idx, labels, hit, ndcg, _dt(dtype))
            outs.append((idx, hit, ndcg))
        for x, y in zip(*outs):
            assert torch.equal(x, y)
        idx, hit, ndcg = outs[1]
        assert _written(hit, ndcg)
        # tests/test_gpu_kernels.py:415-420: ids and hits exact, ndcg within 1e-6
        assert np.array_equal(idx.cpu().numpy(), want)
        lab = labels.cpu().numpy()
        disc = 1.0 / (np.log(np.arange(2, k + 2, dtype=np.float32)) / np.log(np.float32(2.0)))
        assert np.array_equal(hit.cpu().numpy(), (want == lab[:, None]).any(1).astype(np.float32))
        assert np.allclose(ndcg.cpu().numpy(), ((want == lab[:, None]) * disc[None]).sum(1), atol=1e-6)
    _with_arena(dtype, body)


# b4c_topk_rows_excl: the threshold kernel with exclusion lists for both dtypes (+ the list kernel for row 9), and redo NULL
@pytest.mark.parametrize('route', ['threshold', 'lists'])
@pytest.mark.parametrize('dtype', DT, ids=_ids)
def test_topk_rows_excl_pitch(dtype, route):
    V, k, E = 1003, 10, 24

    def body(a):
        s, _ = _topk_inputs(dtype, V, 77)
        sn = s.float().cpu().numpy()
        _, top = nr.top_k(sn, k)
        rng = np.random.default_rng(5)
        ex = np.full((ROWS, E), -1, np.int32)
        for r in range(ROWS):                        # canonical lists: ascending, no duplicates, then -1; half of the best ids in them
            ids = np.unique(np.concatenate([top[r, ::2], rng.integers(0, V, 12)]))
            ex[r, :ids.size] = ids
            sn[r, ids] = -np.inf
        _, want = nr.top_k(sn, k)
        exd = torch.from_numpy(ex).cuda()
        outs = []
        for ss in (a.put(0, s), _compact(s)):
            idx = _full((ROWS, k), -7, torch.int32)
            redo = _full((ROWS,), -7, torch.int32) if route == 'threshold' else None
            _call('b4c_topk_rows_excl', ss, ss.stride(0), ROWS, V, k, idx, None, None, None, redo, _dt(dtype), exd, E, E)
            outs.append(idx)
        assert torch.equal(outs[0], outs[1])
        assert np.array_equal(outs[1].cpu().numpy(), want)                     # tests/test_gpu_kernels.py:415
    _with_arena(dtype, body)


# b4c_candidate_rank_rows: one kernel per dtype (candidates.hip); the scores have the pitch, the lists are compact
@pytest.mark.parametrize('dtype', DT, ids=_ids)
def test_candidate_rank_rows_pitch(dtype):
    V, C, k = 1003, 33, 10

    def body(a):
        s, labels = _topk_inputs(dtype, V, 91)
        rng = np.random.default_rng(3)
        cand = rng.integers(-2, V + 2, (ROWS, C)).astype(np.int32)              # a few absent entries
        lab = labels.cpu().numpy()
        cand[:, 3] = lab                                                          # the label is listed
        cand[:, 7] = cand[:, 2]                                                   # a duplicate
        cd = torch.from_numpy(cand).cuda()
        outs = []
        for ss in (a.put(0, s), _compact(s)):
            rank, idx = _full((ROWS,), -7, torch.int32), _full((ROWS, k), -7, torch.int32)
            _call('b4c_candidate_rank_rows', ss, ss.stride(0), _dt(dtype), cd, C, ROWS, C, V, labels, rank, k, idx)
            outs.append((rank, idx))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        sn = s.float().cpu().numpy()
        s_list = np.take_along_axis(sn, np.clip(cand, 0, V - 1), 1)
        # tests/test_gpu_candidates.py:138,144: exact on the given scores
        assert np.array_equal(outs[1][1].cpu().numpy(), topk_rows(s_list, cand, V, k))
        assert np.array_equal(outs[1][0].cpu().numpy(), rank_rows(s_list, cand, sn[np.arange(ROWS), lab], lab, V))
    _with_arena(dtype, body)


# b4c_candidate_score: `scores` [R][ld_s] fp32 has the pitch (only the C listed columns are written: the window holds)
@pytest.mark.parametrize('dtype', DT, ids=_ids)
def test_candidate_score_scores_pitch(dtype):
    V, C, K = 1003, 33, 64

    def body(a):
        g = _gen(17)
        h, wt, b = (_randn(g, ROWS, K) * 0.5).to(dtype), (_randn(g, V, K) * 0.5).to(dtype), _randn(g, V)
        cand = torch.randint(0, V, (ROWS, C), generator=g, device='cuda').int()
        outs = []
        for sc in (a.out(0, C), _full((ROWS, C), NAN, F32)):
            _call('b4c_candidate_score', h, K, wt, K, b, cand, C, ROWS, C, V, K, _dt(dtype), None, sc, sc.stride(0), None, 0, None)
            outs.append(sc.clone())
        assert _written(*outs) and torch.equal(outs[0], outs[1])
        prod = h.double()[:, None, :] * wt.double()[cand.long()]
        ref = prod.sum(-1) + b.double()[cand.long()]
        bound = K * 2.0 ** -24 * (prod.abs().sum(-1) + b.double()[cand.long()].abs()) + 1e-30       # tests/test_gpu_candidates.py:131
        assert bool(((outs[1].double() - ref).abs() <= bound).all())
    _with_arena(F32, body)


# ---------------------------------------------------------------------------------------------------------------------------
# pitch form: the projection into the head.  C (and the residual of the generic epilogue) has the pitch; A and Bt cannot
# (32-bit buffer offsets inside a tile: refused, see test_gemm_nt_refuses_an_operand_pitch_past_its_buffer_offsets)
# ---------------------------------------------------------------------------------------------------------------------------
# routes of b4c_gemm_nt (gemm.hip): wide-N (bf16 -> bf16, K <= 128, N >= 2048, plain epilogue); generic with the 16-B epilogue
# (N % 8 == 0) and with the scalar one (N = 1003), bf16 -> bf16, bf16 -> fp32, fp32; generic with a residual
GEMM_ROUTES = [('wide_K64', BF16, BF16, 2056, 64, False), ('wide_K128', BF16, BF16, 2056, 128, False),
               ('generic_bf16', BF16, BF16, 1000, 128, False), ('generic_bf16_scalar_epilogue', BF16, BF16, 1003, 64, False),
               ('generic_bf16_to_f32', BF16, F32, 1000, 64, False), ('generic_f32', F32, F32, 1000, 128, False),
               ('generic_f32_scalar_epilogue', F32, F32, 1003, 64, False), ('generic_bf16_residual', BF16, BF16, 1000, 128, True)]


@pytest.mark.parametrize('route,dtype,out_dtype,N,K,res', GEMM_ROUTES, ids=[r[0] for r in GEMM_ROUTES])
def test_gemm_nt_pitch(route, dtype, out_dtype, N, K, res):
    def body(a):
        g = _gen(N + K)
        # entries of -1, 0, 1 and small integer bias / residual: every sum is exact in fp32 and in bf16 (|sum| <= 136)
        A = torch.randint(-1, 2, (ROWS, K), generator=g, device='cuda').to(dtype)
        Bt = torch.randint(-1, 2, (N, K), generator=g, device='cuda').to(dtype)
        bias = torch.randint(-4, 5, (N,), generator=g, device='cuda').float()
        R_ = torch.randint(-4, 5, (ROWS, N), generator=g, device='cuda').to(dtype) if res else None
        outs = []
        for big in (True, False):
            if big:
                C = a.out(0, N)
                rs = a.put(2, R_) if res else None                               # (a residual is an operand of `dtype`: one arena)
            else:
                C, rs = _full((ROWS, _rup8(N)), NAN, out_dtype), (_compact(R_) if res else None)
            _call('b4c_gemm_nt', A, K, Bt, K, C, C.stride(0), ROWS, N, K, bias, 0, None, 0, rs, rs.stride(0) if res else 0,
                  _dt(dtype), _dt(out_dtype))
            outs.append(C[:, :N].clone())
        assert _written(*outs) and torch.equal(outs[0], outs[1])
        want = A.double() @ Bt.double().T + bias.double() + (R_.double() if res else 0)
        assert torch.equal(outs[1].double(), want)                             # tests/test_gpu_kernels.py:49,62: exact on integers
    _with_arena(out_dtype, body)


@pytest.mark.parametrize('K', [64, 128])
def test_gemm_nt_softmax_pitch(K):
    """the wide-N kernel with the softmax epilogue: probabilities [R][ldc] at the pitch"""
    N = 2056

    def body(a):
        g = _gen(K)
        A = torch.randint(-1, 2, (ROWS, K), generator=g, device='cuda').to(BF16)
        Bt = (torch.randint(-1, 2, (N, K), generator=g, device='cuda') * 0.125).to(BF16)
        bias = torch.randint(-4, 5, (N,), generator=g, device='cuda').float() * 0.25
        x = A.double() @ Bt.double().T + bias.double()                          # exact in fp32: multiples of 1/8
        lse2 = (torch.logsumexp(x, -1) / np.log(2.0)).float()
        outs = []
        for C in (a.out(0, N), _full((ROWS, N), NAN, BF16)):
            _call('b4c_gemm_nt_softmax', A, K, Bt, K, C, C.stride(0), ROWS, N, K, bias, lse2)
            outs.append(C.clone())
        assert _written(*outs) and torch.equal(outs[0], outs[1])
        ref = torch.softmax(x, -1)
        assert float(((outs[1].double() - ref).abs() / (ref + 1e-30)).max()) < 6e-3      # tests/test_gpu_round2.py:682
    _with_arena(BF16, body)


def test_gemm_nt_refuses_an_operand_pitch_past_its_tile_descriptor():
    """A and Bt are staged tile by tile through a buffer descriptor of less than 2^30 bytes, with 32-bit offsets: 128 * ld elements
    must span less than 2^30 bytes (include/b4c.h).  Nothing is launched: the arguments are refused on the host."""
    L = _lib()
    t = torch.zeros(128, 128, dtype=BF16, device='cuda')
    c = torch.zeros(128, 2048, dtype=BF16, device='cuda')
    lse = torch.zeros(128, device='cuda')
    from bert4clickpath_amd import ops
    for N in (128, 2048):                                                        # the generic and the wide-N route
        for lda, ldb in ((LD, 128), (128, LD), (1 << 22, 128), (128, 1 << 22)):  # 2^22 * 128 * 2 B = 2^30 exactly
            rc = L.lib().b4c_gemm_nt(t.data_ptr(), lda, t.data_ptr(), ldb, c.data_ptr(), 2048, 1, N, 128, None, 0, None, 0, None, 0,
                                     L.BF16, L.BF16, ops._st())
            assert rc == -1 and b'2^30 bytes' in L.lib().b4c_last_error()       # B4C_EINVAL
    rc = L.lib().b4c_gemm_nt(t.data_ptr(), 1 << 21, t.data_ptr(), 128, c.data_ptr(), 2048, 1, 128, 128, None, 0, None, 0, None, 0,
                             L.F32, L.F32, ops._st())
    assert rc == -1 and b'2^30 bytes' in L.lib().b4c_last_error()               # fp32: 2^21 * 128 * 4 B
    rc = L.lib().b4c_gemm_nt_softmax(t.data_ptr(), 1 << 22, t.data_ptr(), 128, c.data_ptr(), 2048, 1, 2048, 128, None, lse.data_ptr(),
                                     ops._st())
    assert rc == -1 and b'2^30 bytes' in L.lib().b4c_last_error()


# the accept side: a FULL 128-row tile of A (and of Bt on the generic routes) at the largest pitch the check lets through -- row
# 127 starts 16 bytes short of 2^30 * 127 / 128 -- against the compact operands; exact on integers (tests/test_gpu_kernels.py:49,62)
@pytest.mark.parametrize('route,dtype,N', [('generic_bf16', BF16, 128), ('generic_f32', F32, 128), ('wide_bf16', BF16, 2056)])
def test_gemm_nt_takes_the_largest_operand_pitch(route, dtype, N):
    es = 2 if dtype == BF16 else 4
    ld = (1 << 30) // (128 * es) - (8 if dtype == BF16 else 4)
    M = K = 128
    n = 127 * ld + 2 * SLOT
    _need(n * es + (1 << 30))
    flat = None
    try:
        flat = torch.empty(n, dtype=dtype, device='cuda')
        g = _gen(N)
        A = torch.randint(-1, 2, (M, K), generator=g, device='cuda').to(dtype)
        Bt = torch.randint(-1, 2, (N, K), generator=g, device='cuda').to(dtype)
        bias = torch.randint(-4, 5, (N,), generator=g, device='cuda').float()
        Ab = torch.as_strided(flat, (M, K), (ld, 1), 0)
        Ab.copy_(A)
        Bb = Bt
        if N == 128:
            Bb = torch.as_strided(flat, (N, K), (ld, 1), SLOT)
            Bb.copy_(Bt)
        outs = []
        for a_, b_ in ((Ab, Bb), (A, Bt)):
            C = _full((M, N), NAN, dtype)
            _call('b4c_gemm_nt', a_, a_.stride(0), b_, b_.stride(0), C, N, M, N, K, bias, 0, None, 0, None, 0, _dt(dtype), _dt(dtype))
            outs.append(C)
        assert _written(*outs) and torch.equal(outs[0], outs[1])
        assert torch.equal(outs[1].double(), A.double() @ Bt.double().T + bias.double())
    finally:
        _free(flat)


# ---------------------------------------------------------------------------------------------------------------------------
# pitch form: row gather / scatter on token tensors
# ---------------------------------------------------------------------------------------------------------------------------
# b4c_gather_rows: `in` and `out` have the pitch.  b4c_scatter_rows: `src` has the pitch; dst is zero-filled over n_dst * ld_dst
# (the pad is written: compact)
@pytest.mark.parametrize('dtype', DT, ids=_ids)
def test_gather_and_scatter_rows_pitch(dtype):
    W = 264

    def body(a):
        x = _randn(_gen(4), ROWS, W).to(dtype)
        idx = torch.tensor([9, -1, 4, 0, 8, 3, 9, 5, 7, 1], dtype=torch.int32, device='cuda')
        want = torch.where(idx[:, None] >= 0, x[idx.clamp(min=0).long()], torch.zeros((), dtype=dtype, device='cuda'))
        xs = a.put(0, x)
        for out in (a.out(1, W), _full((ROWS, W), NAN, dtype)):
            _call('b4c_gather_rows', xs, xs.stride(0), idx, out, out.stride(0), ROWS, W, _dt(dtype))
            assert torch.equal(out, want)                                         # a copy: exact (test_mask_positions_and_gather)
        sidx = torch.tensor([11, 2, -1, 7, 0, 5, 13, 3, 9, 1], dtype=torch.int32, device='cuda')      # unique
        want = torch.zeros(14, W, dtype=dtype, device='cuda')
        want[sidx[sidx >= 0].long()] = x[sidx >= 0]
        dst = _full((14, W), NAN, dtype)
        _call('b4c_scatter_rows', xs, xs.stride(0), sidx, dst, W, ROWS, 14, W, _dt(dtype))
        assert torch.equal(dst, want)
    _with_arena(dtype, body)


# ---------------------------------------------------------------------------------------------------------------------------
# dense form
# ---------------------------------------------------------------------------------------------------------------------------
def _dense_shape(V):
    from bert4clickpath_amd import ops
    ld = ops.row_pitch(V)
    return ld, ((1 << 31) + 64 * ld) // ld + 1                                  # the smallest R with R * ld > 2^31 + 64 * ld


def _dense_sample(R, ld):
    b = -(-(1 << 31) // ld)                                                      # the first row that starts at or past 2^31 elements
    rows = list(range(64)) + list(range(64, b - 64, 97)) + list(range(b - 64, R))
    return torch.tensor(rows, device='cuda'), b


def _dense_fill(t, V, seed, scale=3.0, probs=False):
    """N(0, scale) logits (probs: their softmax) in the V columns of every row, in chunks of rows; the pad NaN"""
    g = _gen(seed)
    for r0 in range(0, t.shape[0], 4096):
        c = t[r0:r0 + 4096]
        x = _randn(g, c.shape[0], V) * scale
        c[:, :V] = (torch.softmax(x, -1) if probs else x).to(t.dtype)
        c[:, V:] = NAN


# routes of b4c_softmax_rows: bf16 in registers (ld_out <= 65,536), bf16 streaming (wider), fp32 streaming
@pytest.mark.parametrize('route,dtype,V', [('registers_bf16', BF16, 50000), ('stream_bf16', BF16, 65544), ('stream_f32', F32, 50000)])
def test_softmax_rows_dense(route, dtype, V):
    ld, R = _dense_shape(V)
    es = 2 if dtype == BF16 else 4
    _need(2 * R * ld * es + (2 << 30))
    x = y = None
    try:
        x, y = torch.empty(R, ld, dtype=dtype, device='cuda'), torch.empty(R, ld, dtype=dtype, device='cuda')
        _dense_fill(x, V, V)
        y.fill_(NAN)
        _call('b4c_softmax_rows', x, ld, y, ld, R, V, _dt(dtype))
        sel, b = _dense_sample(R, ld)
        xc = x[sel]
        yc = _full(tuple(xc.shape), NAN, dtype)
        _call('b4c_softmax_rows', xc, ld, yc, ld, sel.numel(), V, _dt(dtype))
        got = y[sel]
        assert _written(got, yc) and torch.equal(got, yc), (sel[(got != yc).any(1)][:6].tolist(), b)
        for r0 in range(0, sel.numel(), 128):                                    # float64 in chunks of rows
            p64 = torch.softmax(xc[r0:r0 + 128, :V].double(), -1)
            # tests/test_gpu_kernels.py:365
            assert float((yc[r0:r0 + 128, :V].double() - p64).abs().max()) < (1e-6 if dtype == F32 else 4e-3)
        assert not bool(yc[:, V:].any())
    finally:
        _free(x, y)


# b4c_softmax_rows_bwd (one kernel per dtype): dlogits, whose pads are written, past 2^31 elements
@pytest.mark.parametrize('dtype', DT, ids=_ids)
def test_softmax_rows_bwd_dense(dtype):
    V = 50000
    ld, R = _dense_shape(V)
    es = 2 if dtype == BF16 else 4
    _need(3 * R * ld * es + (2 << 30))
    p = w = dx = None
    try:
        p, w, dx = (torch.empty(R, ld, dtype=dtype, device='cuda') for _ in range(3))
        _dense_fill(p, V, 41, probs=True)
        _dense_fill(w, V, 42, 1.0)
        dx.fill_(NAN)
        _call('b4c_softmax_rows_bwd', p, ld, w, ld, dx, ld, R, V, _dt(dtype))
        sel, b = _dense_sample(R, ld)
        pc, wc = p[sel], w[sel]
        dxc = _full(tuple(pc.shape), NAN, dtype)
        _call('b4c_softmax_rows_bwd', pc, ld, wc, ld, dxc, ld, sel.numel(), V, _dt(dtype))
        got = dx[sel]
        assert _written(got, dxc) and torch.equal(got, dxc), (sel[(got != dxc).any(1)][:6].tolist(), b)
        assert not bool(dxc[:, V:].any())
        for r0 in range(0, sel.numel(), 128):
            pd, wd = pc[r0:r0 + 128, :V].double(), wc[r0:r0 + 128, :V].double()
            ref = pd * (wd - (pd * wd).sum(-1, keepdim=True))
            # tests/test_gpu_round2.py:115
            assert float((dxc[r0:r0 + 128, :V].double() - ref).abs().max()) < (1e-6 if dtype == F32 else 2e-2)
    finally:
        _free(p, w, dx)


def _sparse_ce_bwd_ref(pd, labf, variant, gs):
    """float64 restatement of b4c_sparse_ce_from_probs_bwd on the stored probabilities pd [n][V]; labf fp32 labels (-1: pad row)"""
    lab = labf.long().clamp(min=0)
    onehot = torch.zeros_like(pd).scatter_(1, lab[:, None], 1.0)
    py = pd.gather(1, lab[:, None])
    if variant == 0:
        lo, hi = float(np.float32(1e-7)), float(np.float32(1.0) - np.float32(1e-7))      # the clip bounds as the fp32 kernels hold them
        S = pd.clamp(lo, hi).sum(-1, keepdim=True)
        ref = ((pd >= lo) & (pd <= hi)).double() * (1.0 / S - onehot / py.clamp(lo, hi))
    else:
        ref = -onehot / py
    ref = ref * gs
    ref[labf == -1.0] = 0.0
    return ref


# b4c_sparse_ce_from_probs_bwd (one kernel per dtype, both variants): dprobs, whose pads are written, past 2^31 elements
@pytest.mark.parametrize('variant', [0, 1], ids=['tf', 'plain'])
@pytest.mark.parametrize('dtype', DT, ids=_ids)
def test_sparse_ce_from_probs_bwd_dense(dtype, variant):
    V = 50000
    ld, R = _dense_shape(V)
    es = 2 if dtype == BF16 else 4
    _need(2 * R * ld * es + (2 << 30))
    p = dp = None
    try:
        p, dp = (torch.empty(R, ld, dtype=dtype, device='cuda') for _ in range(2))
        _dense_fill(p, V, 43, probs=True)
        dp.fill_(NAN)
        labf = torch.randint(0, V, (R,), generator=_gen(44), device='cuda').float()
        labf[::7] = -1.0
        gs = torch.tensor([0.37], device='cuda')
        _call('b4c_sparse_ce_from_probs_bwd', p, ld, labf, gs, dp, ld, R, V, variant, _dt(dtype))
        sel, b = _dense_sample(R, ld)
        pc, lc = p[sel], labf[sel]
        dpc = _full(tuple(pc.shape), NAN, dtype)
        _call('b4c_sparse_ce_from_probs_bwd', pc, ld, lc, gs, dpc, ld, sel.numel(), V, variant, _dt(dtype))
        got = dp[sel]
        assert _written(got, dpc) and torch.equal(got, dpc), (sel[(got != dpc).any(1)][:6].tolist(), b)
        assert not bool(dpc[:, V:].any())
        for r0 in range(0, sel.numel(), 128):
            ref = _sparse_ce_bwd_ref(pc[r0:r0 + 128, :V].double(), lc[r0:r0 + 128], variant, float(gs))
            err = float((dpc[r0:r0 + 128, :V].double() - ref).abs().max()) / float(ref.abs().max())
            # tests/test_gpu_round2.py:109 for fp32; bf16: the result is rounded once to bf16 (2^-9 relative) behind the same fp32
            # arithmetic: 2^-8 of the largest entry
            assert err < (1e-4 if dtype == F32 else 2.0 ** -8), err
    finally:
        _free(p, dp)


# b4c_scatter_rows: dst [2^23 + 64][256] (zero-filled over n_dst * ld_dst, then the named rows) past 2^31 elements; bf16: 2^32 bytes
@pytest.mark.parametrize('dtype', DT, ids=_ids)
def test_scatter_rows_dense(dtype):
    es = 2 if dtype == BF16 else 4
    _need(T_ROWS * T_W * es + (2 << 30))
    dst = None
    try:
        dst = torch.empty(T_ROWS, T_W, dtype=dtype, device='cuda')
        dst.fill_(NAN)
        ids = _table_ids(False)
        uniq, inv = _remap(ids)
        idx, idxc = ids.int(), inv.int()
        idx[5] = idxc[5] = -1                                                    # a skipped source row
        src = _randn(_gen(45), ids.numel(), T_W).to(dtype)
        dstc = _full((uniq.numel(), T_W), NAN, dtype)
        _call('b4c_scatter_rows', src, T_W, idx, dst, T_W, ids.numel(), T_ROWS, T_W, _dt(dtype))
        _call('b4c_scatter_rows', src, T_W, idxc, dstc, T_W, ids.numel(), uniq.numel(), T_W, _dt(dtype))
        want = torch.zeros_like(dstc)
        want[idxc[idxc >= 0].long()] = src[idxc >= 0]
        assert torch.equal(dst[uniq], dstc) and torch.equal(dstc, want)          # a copy: exact
        assert not bool(dst[_untouched(uniq)].any()) and not bool(dst[-48:-16].any())       # the zero fill reached the end
    finally:
        _free(dst)


# routes of b4c_softmax_ce_fwd_bwd: bf16 in registers, fp32 fused (ld <= 65,536), streaming (wider; bf16 and fp32)
@pytest.mark.parametrize('variant', [0, 1], ids=['tf', 'plain'])
@pytest.mark.parametrize('route,dtype,V', [('registers_bf16', BF16, 50000), ('fused_f32', F32, 50000), ('stream_bf16', BF16, 65544),
                                           ('stream_f32', F32, 65544)])
def test_softmax_ce_fwd_bwd_dense(route, dtype, V, variant):
    ld, R = _dense_shape(V)
    es = 2 if dtype == BF16 else 4
    _need(R * ld * es + (3 << 30))
    x = None
    try:
        x = torch.empty(R, ld, dtype=dtype, device='cuda')
        _dense_fill(x, V, V + variant)
        g = _gen(9)
        labels = torch.randint(0, V, (R,), generator=g, device='cuda').int()
        labels[::7] = -1                                                          # ignored rows: zero gradient, loss 0
        sel, b = _dense_sample(R, ld)
        xc, lc = x[sel], labels[sel]                                              # the compact copy, taken before the call (in place)
        x0 = xc.clone()
        gs = torch.tensor([0.5], device='cuda')
        item, itemc = _full((R,), NAN, F32), _full((sel.numel(),), NAN, F32)
        _call('b4c_softmax_ce_fwd_bwd', x, ld, labels, item, gs, R, V, variant, _dt(dtype))
        _call('b4c_softmax_ce_fwd_bwd', xc, ld, lc, itemc, gs, sel.numel(), V, variant, _dt(dtype))
        assert _written(item, itemc, xc)
        got = x[sel]
        assert torch.equal(got, xc) and torch.equal(item[sel], itemc), (sel[(got != xc).any(1)][:6].tolist(), b)
        assert not bool(xc[:, V:].any())                                         # pads are written as 0
        for r0 in range(0, sel.numel(), 128):
            x64 = x0[r0:r0 + 128, :V].double().requires_grad_(True)
            lab = lc[r0:r0 + 128].long()
            valid = lab >= 0
            p = torch.softmax(x64, -1)
            if variant == 0:
                lg = torch.log(torch.clamp(p, 1e-7, 1 - 1e-7))
                item64 = torch.logsumexp(lg, -1) - lg.gather(1, lab.clamp(min=0)[:, None])[:, 0]
            else:
                item64 = -torch.log(p.gather(1, lab.clamp(min=0)[:, None])[:, 0])
            (item64[valid].sum() * 0.5).backward()
            # tests/test_gpu_kernels.py:395-397: loss absolute, gradient relative to its largest entry
            assert float((itemc[r0:r0 + 128].double()[valid] - item64.detach()[valid]).abs().max()) < (2e-5 if dtype == F32 else 2e-2)
            assert float(itemc[r0:r0 + 128][~valid].abs().sum()) == 0.0 and float(xc[r0:r0 + 128][~valid].abs().sum()) == 0.0
            err = float((xc[r0:r0 + 128, :V].double() - x64.grad).abs().max()) / float(x64.grad.abs().max())
            assert err < (2e-5 if dtype == F32 else 1.5e-2), err
    finally:
        _free(x)


# the bf16 threshold routes of b4c_topk_rows_ws on the dense tensor (+ the list kernel for flagged rows): register-resident
# (V <= 65,536) and the re-reading kernel topk_rows_kernel<bf16> that takes the wider rows
@pytest.mark.parametrize('route,V', [('registers_bf16', 50000), ('threshold_bf16', 65544)])
def test_topk_rows_dense(route, V):
    k = 10
    ld, R = _dense_shape(V)
    _need(R * ld * 2 + (2 << 30))
    x = None
    try:
        x = torch.empty(R, ld, dtype=BF16, device='cuda')
        _dense_fill(x, V, 31, 1.0)
        sel, b = _dense_sample(R, ld)
        x[sel[-3], :V] = 0.5                                                      # all equal, past the boundary: redone by the list kernel
        labels = torch.randint(0, V, (R,), generator=_gen(2), device='cuda').int()
        xc = x[sel]
        want = torch.sort(xc[:, :V].float(), dim=1, descending=True, stable=True).indices[:, :k]      # ties -> lower index first
        labels[sel] = want[:, 0].int()                                           # hits on the compared rows
        lc = labels[sel]
        n = sel.numel()
        outs = []
        for s, lab, rows in ((x, labels, R), (xc, lc, n)):
            idx, hit, ndcg = _full((rows, k), -7, torch.int32), _full((rows,), NAN, F32), _full((rows,), NAN, F32)
            redo = _full((rows,), -7, torch.int32)
            _call('b4c_topk_rows_ws', s, ld, rows, V, k, idx, lab, hit, ndcg, redo, _dt(BF16))
            outs.append((idx, hit, ndcg))
        assert _written(outs[0][1], outs[0][2]) and not bool((outs[0][0] == -7).any())        # every row written
        for big, small in zip(*outs):
            assert torch.equal(big[sel], small), b
        assert torch.equal(outs[1][0].long(), want)                            # tests/test_gpu_kernels.py:415: exact
        assert bool((outs[1][1] == 1).all())
    finally:
        _free(x)


# ---------------------------------------------------------------------------------------------------------------------------
# the tables of config 5: 2^23 + 64 rows x 256 fp32 (no pitch: dense form)
# ---------------------------------------------------------------------------------------------------------------------------
T_ROWS, T_W = (1 << 23) + 64, 256
T_BOUNDS = (1 << 21, 1 << 22, 1 << 23)          # rows at 2^31 bytes, 2^32 bytes, 2^31 elements


def _table_ids(repeats):
    """the first 16 and the last 16 rows, 16 on each side of every boundary (~200 ids); with repeats, in a shuffled order"""
    ids = list(range(16)) + list(range(T_ROWS - 16, T_ROWS))
    for b in T_BOUNDS:
        ids += list(range(b - 16, b + 16))
    rng = np.random.default_rng(8)
    if repeats:
        ids = ids + [ids[i] for i in rng.integers(0, len(ids), 40)]
    return torch.from_numpy(rng.permutation(np.array(ids, np.int64))).cuda()


def _remap(ids):
    """-> (unique rows ascending, ids as indices into them): the small table of a compact run"""
    uniq, inv = torch.unique(ids, return_inverse=True)
    return uniq, inv


def _untouched(named):
    """a strided sample of 4,096 rows plus the 64 rows around each boundary, without the named rows"""
    rows = torch.cat([torch.arange(0, T_ROWS, T_ROWS // 4096)[:4096]] + [torch.arange(b - 32, b + 32) for b in T_BOUNDS]).cuda()
    return rows[~torch.isin(rows, named)]


def _zeros_table():
    from bert4clickpath_amd import ops
    return ops.zeros(T_ROWS, T_W, device='cuda')


def test_rows_gather_and_scatter_add_tables():
    """b4c_rows_gather_f32 (ids with repeats) and b4c_rows_scatter_add_f32 -- float atomics: ids WITHOUT repeats, so every sum has
    one term (0 + x) and stays exact"""
    _need(T_ROWS * T_W * 4 + (2 << 30))
    tab = None
    try:
        tab = _zeros_table()
        g = _gen(6)
        ids = _table_ids(True)
        uniq, inv = _remap(ids)
        small = _randn(g, uniq.numel(), T_W)
        tab[uniq] = small
        n = ids.numel()
        out, outc = _full((n, T_W), NAN, F32), _full((n, T_W), NAN, F32)
        _call('b4c_rows_gather_f32', tab, T_W, ids, out, T_W, n, T_W)
        _call('b4c_rows_gather_f32', small, T_W, inv, outc, T_W, n, T_W)
        assert torch.equal(out, outc) and torch.equal(outc, small[inv])         # a copy: exact
        tab[uniq] = 0.0
        ids = _table_ids(False)
        uniq, inv = _remap(ids)
        src = _randn(g, ids.numel(), T_W)
        dstc = torch.zeros(uniq.numel(), T_W, device='cuda')
        _call('b4c_rows_scatter_add_f32', src, T_W, ids, tab, T_W, ids.numel(), T_W)
        _call('b4c_rows_scatter_add_f32', src, T_W, inv, dstc, T_W, ids.numel(), T_W)
        want = torch.zeros_like(dstc)
        want[inv] = src
        assert torch.equal(tab[uniq], dstc) and torch.equal(dstc, want)
        assert not bool(tab[_untouched(uniq)].any())
    finally:
        _free(tab)


HYPER = (0.9, 0.999, 1e-9)


@pytest.mark.parametrize('form', ['ids', 'range'])
@pytest.mark.parametrize('decay', [False, True], ids=['adam', 'adamw'])
@pytest.mark.parametrize('mode', [0, 1], ids=['catch_up', 'step'])
def test_adam_rows_tables(mode, decay, form):
    """b4c_adam_rows / b4c_adamw_rows on four arenas of 8.6 GB: named rows (with repeats) and the range form with row_lo past the
    2^31-element row.  The compact run is bit-identical, and equals the dense kernel's replay (b4c_adam_step / b4c_adamw_step,
    tests/test_gpu_lazy_adam.py:48,67: bit for bit)."""
    _need(4 * T_ROWS * T_W * 4 + (3 << 30))
    P = [None] * 4
    try:
        for i in range(4):
            P[i] = _zeros_table()
        stamp = torch.zeros(T_ROWS, dtype=torch.int32, device='cuda')
        P.append(stamp)
        t, old = 9, 5
        g = _gen(12 + mode)
        lr_hist = (torch.rand(t + 1, generator=g, device='cuda') * 1e-3 + 1e-4)
        d_hist = (torch.rand(t + 1, generator=g, device='cuda') * 1e-2) if decay else None
        if form == 'ids':
            ids = _table_ids(True)
            uniq, inv = _remap(ids)
            n, row_lo, row_lo_c = ids.numel(), 0, 0
        else:
            row_lo, n = (1 << 23) + 8, 40
            uniq = torch.arange(row_lo, row_lo + n, device='cuda')
            ids = inv = None
            row_lo_c = 0
        m = uniq.numel()
        small = [_randn(g, m, T_W) * 0.05, _randn(g, m, T_W), _randn(g, m, T_W) * 0.01, _randn(g, m, T_W).abs() * 1e-4]
        small[2][::3] = 0.0                                                       # rows that never received a gradient: m = v = 0
        small[3][::3] = 0.0
        st_small = torch.full((m,), old, dtype=torch.int32, device='cuda')
        for big, s in zip(P, small):
            big[uniq] = s
        stamp[uniq] = st_small
        ref = [s.clone() for s in small]
        comp = [s.clone() for s in small]
        st_c = st_small.clone()
        b1, b2, eps = HYPER
        gmul = 0.5

        def run(p, gr, mm, vv, st, ids_, lo, rows):
            if decay:
                _call('b4c_adamw_rows', p, gr, mm, vv, st, ids_, n, lo, rows, T_W, lr_hist, d_hist, t, b1, b2, eps, gmul, None, mode)
            else:
                _call('b4c_adam_rows', p, gr, mm, vv, st, ids_, n, lo, rows, T_W, lr_hist, t, b1, b2, eps, gmul, mode)
        run(*P[:4], stamp, ids, row_lo, T_ROWS)
        run(*comp, st_c, inv, row_lo_c, m)
        for big, c in zip(P[:4], comp):
            assert torch.equal(big[uniq], c)
        assert torch.equal(stamp[uniq], st_c) and bool((st_c == t).all())
        # the dense kernel's replay on the compact rows: zero-gradient steps old + 1 .. (t or t - 1), then step t with the gradient
        p, gr, mm, vv = ref
        zero = torch.zeros_like(gr)
        blocks = torch.ones(m * T_W // 64, dtype=torch.uint8, device='cuda')
        lrs, ds = lr_hist.tolist(), d_hist.tolist() if decay else None
        for s in range(old + 1, t + 1):
            gg, mul = (gr, gmul) if (s == t and mode == 1) else (zero, 1.0)
            if decay:
                _call('b4c_adamw_step', p, gg, mm, vv, m * T_W, lrs[s], b1, b2, eps, mul, None, ds[s], blocks)
            else:
                _call('b4c_adam_step', p, gg, mm, vv, m * T_W, lrs[s], b1, b2, eps, mul)
        assert torch.equal(comp[0], p) and torch.equal(comp[2], mm) and torch.equal(comp[3], vv)
        if mode == 1:
            assert not bool(comp[1].any())                                       # the step zeroes the gradient rows it consumed
        else:
            assert torch.equal(comp[1], small[1])
        rest = _untouched(uniq)
        assert not any(bool(big[rest].any()) for big in P)
    finally:
        _free(*P)


@pytest.mark.parametrize('dtype', DT, ids=_ids)
def test_embedding_stage_tables(dtype):
    """b4c_embed_concat_pe_fwd and the three backward forms on a 2^23 + 64 row table.  The atomic form and the sorted form without
    a scratch add through float atomics: ids WITHOUT repeats there, so every sum has one term; the scratch form is deterministic
    and takes the repeats."""
    _need(T_ROWS * T_W * 4 + (2 << 30))
    tab = None
    try:
        tab = _zeros_table()
        g = _gen(21)
        scale, d = 16.0, T_W
        dims = (ctypes.c_int * 1)(d)

        def arrs(ids_t, table):
            c = ctypes
            return ((c.c_void_p * 1)(ids_t.data_ptr()), (c.c_void_p * 1)(table.data_ptr()), (c.c_int64 * 1)(table.shape[0]))

        # forward (ids with repeats, one of them 0: a padded key)
        ids = _table_ids(True)
        uniq, inv = _remap(ids)
        small = _randn(g, uniq.numel(), d) * 0.05
        tab[uniq] = small
        S = ids.numel()
        pe = _randn(g, S, d)
        outs = []
        for ids_t, table in ((ids, tab), (inv, small)):
            out, kp = _full((S, d), NAN, dtype), torch.full((S,), 7, dtype=torch.uint8, device='cuda')
            ia, ta, ra = arrs(ids_t, table)
            _call('b4c_embed_concat_pe_fwd', 1, ia, ta, dims, ra, pe, scale, out, d, kp, 1, S, d, 0.0, 0, _dt(dtype))
            outs.append((out, kp))
        assert _written(outs[0][0]) and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert torch.equal(outs[1][1], (ids == 0).to(torch.uint8))
        want = small.double()[inv] * scale + pe.double()
        err = float((outs[1][0].double() - want).abs().max() / want.abs().max())
        assert err < (1e-6 if dtype == F32 else 6e-3), err                       # tests/test_gpu_kernels.py:130
        tab[uniq] = 0.0

        L = _lib().lib()
        for form, repeats in (('atomic', False), ('sorted', False), ('sorted_ws', True)):
            ids = _table_ids(repeats)
            uniq, inv = _remap(ids)
            S = ids.numel()
            dout = _randn(g, S, d).to(dtype)
            dsm = torch.zeros(uniq.numel(), d, device='cuda')
            for ids_t, table in ((ids, tab), (inv, dsm)):
                ia, ta, ra = arrs(ids_t, table)
                order = torch.argsort(ids_t, stable=True).int()
                oa = (ctypes.c_void_p * 1)(order.data_ptr())
                if form == 'atomic':
                    _call('b4c_embed_concat_pe_bwd', 1, ia, ta, dims, ra, scale, dout, d, 1, S, d, 0.0, 0, _dt(dtype))
                elif form == 'sorted':
                    _call('b4c_embed_concat_pe_bwd_sorted', 1, ia, oa, ta, dims, ra, scale, dout, d, 1, S, d, 0.0, 0, _dt(dtype))
                else:
                    ws = torch.zeros(int(L.b4c_embed_concat_pe_bwd_sorted_workspace_bytes(1, dims, 1, S)), dtype=torch.uint8, device='cuda')
                    _call('b4c_embed_concat_pe_bwd_sorted_ws', 1, ia, oa, ta, dims, ra, scale, dout, d, 1, S, d, 0.0, 0, ws, ws.numel(),
                          _dt(dtype))
            assert torch.equal(tab[uniq], dsm), form
            ref = torch.zeros(uniq.numel(), d, dtype=torch.float64, device='cuda').index_add_(0, inv, dout.double() * scale)
            assert float((dsm.double() - ref).abs().max() / ref.abs().max()) < 1e-5, form      # tests/test_gpu_kernels.py:144
            assert not bool(tab[_untouched(uniq)].any()), form
            tab[uniq] = 0.0
    finally:
        _free(tab)
