"""The weight-gradient GEMMs (b4c_gemm_tn, b4c_gemm_tn_seg, b4c_gemm_tn_group; csrc/gemm.hip, the TN part) against float64 on the
CPU, on every split class, segment layout and operand form (the cases: tests/tn_cases.py; their split plans are pinned without a GPU
by tests/test_tn_plan_cpu.py).

    dW[K, N] += a[:, :K]^T g[:, :N],   db[N] += column sums of g[:, :N]        (fp32 outputs, "add to what is there")

The reference is always a.double().T @ g.double() and g.double().sum(0) of the operands as the kernel reads them (rounded to their
type).  On small integers every product and every partial sum is exact in fp32 in any order, so the integer tests demand equality
bit for bit: they see dropped or doubled rows, wrong tiles, segments and split sets, and a store where an add belongs (the outputs
are pre-filled with random integers and every launch is repeated into the same tensors).  They are blind to a loss of precision,
which the real-valued test bounds element by element."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import local_bounds as lb  # noqa: E402
import tn_cases as T  # noqa: E402

TD = {'bf16': torch.bfloat16, 'f32': torch.float32}
NAN = float('nan')
SENTINEL = 12345.0


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def L(ops):
    from bert4clickpath_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _pitches(K, N, pitch):
    return ((K + 7) // 8 * 8, (N + 7) // 8 * 8) if pitch == 'pad8' else (K, N)


@functools.lru_cache(maxsize=None)
def _int_case(M, K, N, dtype, pitch):
    """-> a, g on the GPU (integers in -2 .. 2, pitches by `pitch`, zeros in the pad), the float64 references of dW and db, and the
    integer prefill of both outputs.  Computed once per case and shared by every test of it: nothing writes to these tensors."""
    g = torch.Generator().manual_seed(M * 131 + K * 7 + N)
    a, gr = _ints(g, (M, K), -2, 2), _ints(g, (M, N), -2, 2)
    lda, ldg = _pitches(K, N, pitch)
    A, G = torch.zeros(M, lda), torch.zeros(M, ldg)
    A[:, :K], G[:, :N] = a, gr
    pre_w, pre_b = _ints(g, (K, N), -8, 8), _ints(g, (N,), -8, 8)
    return A.to(TD[dtype]).cuda(), G.to(TD[dtype]).cuda(), a.double().T @ gr.double(), gr.double().sum(0), pre_w, pre_b


def _sinks(pre_w, pre_b, n_seg):
    w = pre_w.shape[1] // n_seg
    return ([pre_w[:, i * w:(i + 1) * w].contiguous().cuda() for i in range(n_seg)],
            [pre_b[i * w:(i + 1) * w].contiguous().cuda() for i in range(n_seg)])


def _same(got, want, what):
    got = got.cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(x) for x in bad[0])
        raise AssertionError('%s: %d of %d elements differ; first at %s: got %r, want %r'
                             % (what, len(bad), got.numel(), i, float(got[i]), float(want[i])))


# ---------------------------------------------------------------------------------------------------------------------------------
# a. exact on integers, accumulating, through ops.gemm_tn
# ---------------------------------------------------------------------------------------------------------------------------------
def _variants():
    out = []
    for c in T.SINGLE:
        vs = ['into1', 'fresh', 'nobias']
        if c[2] in T.SEGMENTS:
            vs.append('seg')
        if c[5] != 'one':                      # one split adds to dW directly whether a workspace is there or not
            vs.append('atomic')
        out += [pytest.param(c, v, id=T.case_id(c) + '-' + v) for v in vs]
    return out


@pytest.mark.parametrize('case,variant', _variants())
def test_exact_on_integers_accumulating(ops, case, variant):
    """result == prefill + reference bit for bit, and == prefill + 2 x reference after a second launch into the same tensors.
    into1: into= one segment;  seg: into= 3 x 104 / 4 x 192 column segments;  fresh: the zeros ops.gemm_tn allocates;  nobias: db NULL,
    dW as with it;  atomic: ops.tn_deterministic = False (no workspace: float atomics, exact on integers too), segmented where the case
    has segments."""
    M, K, N, dtype, pitch = case[:5]
    A, G, ref_w, ref_b, pre_w, pre_b = _int_case(M, K, N, dtype, pitch)
    if variant == 'fresh':
        dW, db = ops.gemm_tn(A, G, K, N)
        _same(dW, ref_w, 'dW')
        _same(db, ref_b, 'db')
        return
    if variant == 'nobias':
        dW0, _ = ops.gemm_tn(A, G, K, N)
        dW, db = ops.gemm_tn(A, G, K, N, want_bias=False)
        assert db is None and torch.equal(dW, dW0)
        _same(dW, ref_w, 'dW without db')
        return
    n_seg = T.SEGMENTS.get(N, 1) if variant in ('seg', 'atomic') else 1
    dWs, dbs = _sinks(pre_w, pre_b, n_seg)
    det = ops.tn_deterministic
    try:
        ops.tn_deterministic = variant != 'atomic'
        for rep in (1, 2):
            ops.gemm_tn(A, G, K, N, into=(dWs, dbs))
            _same(torch.cat(dWs, 1), pre_w.double() + rep * ref_w, 'dW after launch %d' % rep)
            _same(torch.cat(dbs), pre_b.double() + rep * ref_b, 'db after launch %d' % rep)
    finally:
        ops.tn_deterministic = det


# ---------------------------------------------------------------------------------------------------------------------------------
# b. the ABI's fallbacks and optional arguments (raw calls)
# ---------------------------------------------------------------------------------------------------------------------------------
def _raw_tn(L, A, G, dW_ptr, ldw, db, M, K, N, dtype, ws_ptr, ws_bytes):
    L.check(L.lib().b4c_gemm_tn(A.data_ptr(), A.stride(0), G.data_ptr(), G.stride(0), dW_ptr, ldw, db.data_ptr() if db is not None else None,
                                M, K, N, T.dt_code(L, dtype), ws_ptr, ws_bytes, _st()), 'gemm_tn')


def test_abi_workspace_fallbacks_and_null_db(ops, L):
    """A workspace that is NULL, one byte short or not 16-byte aligned makes b4c_gemm_tn add its partial tiles with float atomics
    (TN_ATOMIC) and still return 0: exact on integers.  Then db NULL with a good workspace (TN_WS without column sums)."""
    M, K, N, dtype = 1000, 104, 312, 'bf16'
    assert T.single_nsplit(L, M, K, N, dtype) > 1
    A, G, ref_w, ref_b, pre_w, pre_b = _int_case(M, K, N, dtype, 'pad8')
    need = int(L.lib().b4c_gemm_tn_workspace_bytes(M, K, N, L.BF16))
    ws = torch.zeros(need + 16, dtype=torch.uint8, device='cuda')
    assert ws.data_ptr() % 16 == 0
    for what, (p, nb) in (('NULL', (None, 0)), ('one byte short', (ws.data_ptr(), need - 1)), ('misaligned', (ws.data_ptr() + 4, need)),
                          ('good', (ws.data_ptr(), need))):
        dW, db = pre_w.cuda(), pre_b.cuda()
        _raw_tn(L, A, G, dW.data_ptr(), N, db, M, K, N, dtype, p, nb)
        _same(dW, pre_w.double() + ref_w, 'dW, workspace ' + what)
        _same(db, pre_b.double() + ref_b, 'db, workspace ' + what)
    for what, (p, nb) in (('good', (ws.data_ptr(), need)), ('NULL', (None, 0))):
        dW = pre_w.cuda()
        _raw_tn(L, A, G, dW.data_ptr(), N, None, M, K, N, dtype, p, nb)
        _same(dW, pre_w.double() + ref_w, 'dW without db, workspace ' + what)


@pytest.mark.parametrize('M,dtype,mode', [(1000, 'bf16', 'ws'), (1000, 'bf16', 'atomic'), (128, 'f32', 'direct'), (2100, 'f32', 'ws')])
def test_dw_as_a_column_slice_leaves_its_neighbours(ops, L, M, dtype, mode):
    """ldw = N + 24: dW is columns 8 .. 8 + N of a wider fp32 matrix filled with a sentinel; the slice receives prefill + reference and
    every other element keeps the sentinel, in each of the three emit paths (the split classes differ: 128 rows direct, 1000 narrow,
    2100 wide)."""
    K, N = 104, 312
    assert (T.single_nsplit(L, M, K, N, dtype) == 1) == (mode == 'direct')
    A, G, ref_w, ref_b, pre_w, pre_b = _int_case(M, K, N, dtype, 'pad8')
    need = int(L.lib().b4c_gemm_tn_workspace_bytes(M, K, N, T.dt_code(L, dtype)))
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device='cuda')
    wide = torch.full((K + 1, N + 24), SENTINEL)
    wide[:K, 8:8 + N] = pre_w
    wide_d, db = wide.cuda(), pre_b.cuda()
    _raw_tn(L, A, G, wide_d.data_ptr() + 8 * 4, N + 24, db, M, K, N, dtype, *((ws.data_ptr(), need) if mode == 'ws' else (None, 0)))
    want = wide.double()
    want[:K, 8:8 + N] += ref_w
    _same(wide_d, want, 'the wider matrix')
    _same(db, pre_b.double() + ref_b, 'db')


# ---------------------------------------------------------------------------------------------------------------------------------
# c. operand forms
# ---------------------------------------------------------------------------------------------------------------------------------
FORMS = ['contiguous', 'padded', 'middle', 'column2', 'pitch+2', 'last']
GENERIC = ('column2', 'pitch+2')           # the forms that no 16-byte load can read


def _form(vals, form, dtype):
    """The [M, w] values as a view of a parent buffer of M + 1 rows whose every other element is NaN (the spare last row too)."""
    M, w = vals.shape
    pitch, c0 = {'contiguous': (w, 0), 'padded': (w + 8, 0), 'middle': (w + 24, 8), 'column2': (w + 8, 2), 'pitch+2': (w + 2, 0),
                 'last': (w + 104, 104)}[form]
    parent = torch.full((M + 1, pitch), NAN)
    parent[:M, c0:c0 + w] = vals
    parent = parent.to(TD[dtype]).cuda()
    view = parent[:M, c0:c0 + w]
    assert view.stride(0) == pitch and view.data_ptr() == parent.data_ptr() + c0 * parent.element_size()
    return view, parent


@pytest.mark.parametrize('form_a', FORMS)
@pytest.mark.parametrize('M', [257, 4200])
@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
def test_operand_forms(ops, dtype, M, form_a):
    """A and G each contiguous, with a padded pitch (112 / 320), cut from the middle of a 16-byte aligned wider buffer, starting at
    column 2 of one (4-byte aligned only), with a pitch of width + 2 (even, no multiple of 8), and as the last column block of a wider
    buffer; everything beside the operand is NaN.  Exact on integers, M = 257 (2 splits) and 4200 (17), K = 104, N = 3 x 104 segments.
    bf16: b4c_gemm_tn takes its 16-byte kernel iff both pitches are multiples of 8 and both pointers 16-byte aligned; that is all that
    is cheaply knowable of the route from here, so it is asserted of the operands: a combination with a 'column2' or 'pitch+2' operand
    must take the generic kernel gemm_tn_kernel<bf16_t>, every other one the 16-byte kernel.
    Every parent has a spare NaN row behind the last token: these tests check values, whatever a loader reads beside them."""
    K, N = 104, 312
    _, _, ref_w, ref_b, pre_w, pre_b = _int_case(M, K, N, dtype, 'pad8')
    g = torch.Generator().manual_seed(M * 131 + K * 7 + N)
    a, gr = _ints(g, (M, K), -2, 2), _ints(g, (M, N), -2, 2)           # the values of _int_case
    A, keep_a = _form(a, form_a, dtype)
    for form_g in FORMS:
        G, keep_g = _form(gr, form_g, dtype)
        if dtype == 'bf16':
            vec16 = all(t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0 for t in (A, G))
            assert vec16 == (form_a not in GENERIC and form_g not in GENERIC), (form_a, form_g)
        for n_seg in (1, 3):
            dWs, dbs = _sinks(pre_w, pre_b, n_seg)
            ops.gemm_tn(A, G, K, N, into=(dWs, dbs))
            _same(torch.cat(dWs, 1), pre_w.double() + ref_w, 'dW, A %s, G %s, %d segments' % (form_a, form_g, n_seg))
            _same(torch.cat(dbs), pre_b.double() + ref_b, 'db, A %s, G %s, %d segments' % (form_a, form_g, n_seg))


# ---------------------------------------------------------------------------------------------------------------------------------
# d. real values
# ---------------------------------------------------------------------------------------------------------------------------------
def _bound(M, nsplit, companion):
    """No bf16 rounding on the path (n = 0 in the terms of local_bounds): exact products of two bf16 (fp32: products rounded once) are
    summed in fp32 in some order -- M terms, the nsplit partial tiles and the prefill: at most M + nsplit + 2 roundings of partial
    sums that the absolute companion dominates."""
    return lb.SECOND_ORDER * (M + nsplit + 2) * lb.U_F32 * companion


@functools.lru_cache(maxsize=None)
def _real_case(M, K, N, dtype):
    g = torch.Generator().manual_seed(M + K + N)
    a = torch.randn(M, K, generator=g).to(TD[dtype])
    gr = (torch.randn(M, N, generator=g) * 0.1).to(TD[dtype])
    pre_w, pre_b = torch.randn(K, N, generator=g), torch.randn(N, generator=g)
    ad, gd = a.double(), gr.double()
    ref = (pre_w.double() + ad.T @ gd, pre_b.double() + gd.sum(0))
    comp = (pre_w.double().abs() + ad.abs().T @ gd.abs(), pre_b.double().abs() + gd.abs().sum(0))
    return a.cuda(), gr.cuda(), pre_w, pre_b, ref, comp


@pytest.mark.parametrize('mode', ['workspace', 'atomic'])
@pytest.mark.parametrize('case', T.REAL, ids=lambda c: '%dx%dx%d-%s' % c)
def test_real_values_within_the_fp32_bound(ops, L, case, mode):
    """randn operands (G scaled by 0.1), randn prefill: every element within
        |got - ref| <= (1 + 2^-6) (M + nsplit + 2) 2^-24 (|a|^T |g| + |prefill|)        (db: sum |g| + |prefill|),
    a bound derived from fp32 summation alone, not measured.  This test is for precision -- a partial tile staged as bf16, a
    product rounded early: errors of 2^-8 relative against a bound that is M 2^-24 of the absolute sum.  Dropped or doubled
    rows are the integer tests' business.  The workspace mode is launched twice on the same inputs and must repeat bit for bit.
    Measured on the MI355X: the worst |err| / bound of any case is 4e-3 (dW of the 257-row case, atomic mode; 1e-4 at 4200 rows and
    less above: the errors of M roundings do not share a sign), and a build that rounds the partial tiles to bf16 on their way into the workspace leaves the bound of the 257-row
    case by 68 x (its 2 partial tiles carry most of their sum; at 4200 rows and more the bound's M 2^-24 has outgrown 2^-9 / sqrt(M))."""
    M, K, N, dtype = case
    a, gr, pre_w, pre_b, ref, comp = _real_case(M, K, N, dtype)
    ns = T.single_nsplit(L, M, K, N, dtype)
    n_seg = T.SEGMENTS.get(N, 1)
    det = ops.tn_deterministic
    runs = []
    try:
        ops.tn_deterministic = mode == 'workspace'
        for _ in range(2 if mode == 'workspace' else 1):
            dWs, dbs = _sinks(pre_w, pre_b, n_seg)
            ops.gemm_tn(a, gr, K, N, into=(dWs, dbs))
            runs.append((torch.cat(dWs, 1), torch.cat(dbs)))
    finally:
        ops.tn_deterministic = det
    for name, got, r, c in zip(('dW', 'db'), runs[0], ref, comp):
        b = _bound(M, ns, c)
        print('%s %s %s: worst |err| / bound = %.3g' % (case, mode, name, lb.worst_ratio(got, r, b)))
        lb.check(name, got, r, b)
    if mode == 'workspace':
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---------------------------------------------------------------------------------------------------------------------------------
# e. grouped launches (raw b4c_gemm_tn_group calls: ops.queue_dw only groups from 4096 rows, the small plans are unreachable there)
# ---------------------------------------------------------------------------------------------------------------------------------
def _group_run(ops, L, M, probs, nodb=(), wide=(), real=False):
    """One b4c_gemm_tn_group launch over bf16 operands -> per problem (got dW, got db or None, reference dW, reference db, companions,
    dW and db of ops.gemm_tn(into=) on the same operands and prefill).  nodb: problems launched with every db NULL;  wide: problems
    whose segments are column slices of one sentinel-filled matrix (ldw > seg_width), checked here."""
    g = torch.Generator().manual_seed(M + len(probs))
    descs = (L.TNDesc * len(probs))()
    keep, out = [], []
    for i, (d, (K, N, n_seg)) in enumerate(zip(descs, probs)):
        if real:
            a, gr = torch.randn(M, K, generator=g).bfloat16(), (torch.randn(M, N, generator=g) * 0.1).bfloat16()
            pre_w, pre_b = torch.randn(K, N, generator=g), torch.randn(N, generator=g)
        else:
            a, gr = _ints(g, (M, K), -2, 2).bfloat16(), _ints(g, (M, N), -2, 2).bfloat16()
            pre_w, pre_b = _ints(g, (K, N), -8, 8), _ints(g, (N,), -8, 8)
        assert K % 8 == 0 and N % 8 == 0
        A, G = a.cuda(), gr.cuda()
        w = N // n_seg
        dWs, dbs = _sinks(pre_w, pre_b, n_seg)
        ldw, parent = w, None
        if i in wide:
            ldw = n_seg * (w + 8) + 24
            parent = torch.full((K + 1, ldw), SENTINEL)
            for s in range(n_seg):
                parent[:K, 8 + s * (w + 8):8 + s * (w + 8) + w] = pre_w[:, s * w:(s + 1) * w]
            parent_d = parent.cuda()
            dWs = [parent_d[:K, 8 + s * (w + 8):8 + s * (w + 8) + w] for s in range(n_seg)]
            keep.append(parent_d)
        d.A, d.G, d.lda, d.ldg, d.K = A.data_ptr(), G.data_ptr(), A.stride(0), G.stride(0), K
        d.n_seg, d.seg_width, d.ldw = n_seg, w, ldw
        for s in range(n_seg):
            d.dW[s] = dWs[s].data_ptr()
            d.db[s] = None if i in nodb else dbs[s].data_ptr()
        ad, gd = a.double(), gr.double()
        out.append(dict(K=K, N=N, n_seg=n_seg, A=A, G=G, dWs=dWs, dbs=None if i in nodb else dbs, pre_w=pre_w, pre_b=pre_b,
                        ref_w=pre_w.double() + ad.T @ gd, ref_b=pre_b.double() + gd.sum(0), parent=parent,
                        parent_d=keep[-1] if i in wide else None,
                        comp_w=pre_w.double().abs() + ad.abs().T @ gd.abs(), comp_b=pre_b.double().abs() + gd.abs().sum(0)))
    need = int(L.lib().b4c_gemm_tn_group_workspace_bytes(descs, len(probs), M))
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    L.check(L.lib().b4c_gemm_tn_group(descs, len(probs), M, L.BF16, ws.data_ptr(), need, _st()), 'gemm_tn_group')
    torch.cuda.synchronize()
    for p in out:
        p['got_w'] = torch.cat([t.contiguous() for t in p['dWs']], 1)
        p['got_b'] = torch.cat(p['dbs']) if p['dbs'] is not None else None
        if p['parent'] is not None:                          # the sentinels around the segments
            w = p['N'] // p['n_seg']
            want = p['parent'].double()
            for s in range(p['n_seg']):
                want[:p['K'], 8 + s * (w + 8):8 + s * (w + 8) + w] = p['ref_w'][:, s * w:(s + 1) * w]
            _same(p['parent_d'], want, 'the wider matrix of a %d x %d problem' % (p['K'], p['N']))
        sW, sb = _sinks(p['pre_w'], p['pre_b'], p['n_seg'])
        ops.gemm_tn(p['A'], p['G'], p['K'], p['N'], into=(sW, sb))
        p['single_w'], p['single_b'] = torch.cat(sW, 1), torch.cat(sb)
    return out


def _group_exact(out, what):
    for i, p in enumerate(out):
        name = '%s, problem %d (%d x %d, %d segments)' % (what, i, p['K'], p['N'], p['n_seg'])
        _same(p['got_w'], p['ref_w'], 'dW of ' + name)
        assert torch.equal(p['got_w'], p['single_w']), 'dW differs from the single launch: ' + name
        if p['got_b'] is not None:
            _same(p['got_b'], p['ref_b'], 'db of ' + name)
            assert torch.equal(p['got_b'], p['single_b']), 'db differs from the single launch: ' + name


@pytest.mark.parametrize('case', T.GROUP, ids=T.group_id)
def test_group_exact_on_integers(ops, L, case):
    """Every grouped plan: integer operands, random-integer prefill; == prefill + float64 reference bit for bit and == what
    ops.gemm_tn(into=) gives on the same operands."""
    M, probs = case[:2]
    _group_exact(_group_run(ops, L, M, probs), T.group_id(case))


@pytest.mark.parametrize('case', [T.GROUP[0], T.GROUP[1], T.GROUP[5]], ids=T.group_id)
def test_group_null_db_and_sliced_dw(ops, L, case):
    """One problem without column sums (every db NULL), another whose dW segments are column slices of a sentinel-filled wider matrix
    (ldw > seg_width, sentinels untouched) -- with one split, a narrow and a wide reduction."""
    M, probs = case[:2]
    out = _group_run(ops, L, M, probs, nodb=(1,), wide=(0, 3))
    assert out[1]['got_b'] is None
    _group_exact(out, T.group_id(case))


def test_group_real_values_within_the_fp32_bound(ops, L):
    """The straddling-segment group on real data under the bound of test_real_values_within_the_fp32_bound."""
    M, probs = T.GROUP_REAL[:2]
    ns = T.group_nsplit(L, M, probs)
    for i, p in enumerate(_group_run(ops, L, M, probs, real=True)):
        for name, got, r, c in (('dW', p['got_w'], p['ref_w'], p['comp_w']), ('db', p['got_b'], p['ref_b'], p['comp_b'])):
            b = _bound(M, ns, c)
            print('group problem %d %s: worst |err| / bound = %.3g' % (i, name, lb.worst_ratio(got, r, b)))
            lb.check('%s of problem %d' % (name, i), got, r, b)
