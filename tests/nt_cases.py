"""The committed cases of the forward GEMM b4c_gemm_nt / b4c_gemm_nt_act (csrc/gemm.hip, the NT part), a restatement of its host
dispatch, a bit-exact CPU emulation of what each route stores, and an element-wise bound for the forms that cannot be emulated bit
for bit.  No tests here: tests/test_nt_cases_cpu.py checks the case lists against route() and feeds the checkers deliberately wrong
variants (no GPU), tests/test_gpu_gemm_nt.py runs the kernels.

Routes (route(), from b4c_gemm_nt_act, gemm.hip:829-872)

    'wide'    gemm_nt_wide2_kernel<false>: bf16 in and out, K <= 128, N >= 2048, bias as the only epilogue operand, N % 8 == 0,
              ldc % 8 == 0, C and bias 16-byte aligned (gemm.hip:830-831, vec_ok_wide :778-780).  mt x chunks workgroups, each walks
              tiles_per_chunk N tiles (:832-837) with the next W tile prefetched into registers (:723).
    'vec'     gemm_nt_kernel, OutT = bf16 and vec_ok (:851-855, `vec` at :171): the 16-byte epilogue behind the LDS transpose.
    'scalar'  gemm_nt_kernel otherwise (fp32 output, N % 8 != 0, a pitch that is no multiple of 8, a misaligned C / gate / residual /
              pre / bias): the element loop at the bottom of the kernel (:289-312).
    The instantiation of gemm_nt_kernel is (T, OutT, EPI, ACTX): T / OutT from the types (:870-872), EPI = gate or residual (:867),
    ACTX = pre, a GELU activation or a GELU gate (:869).  xcd_map = 1 for 2 .. 8 N tiles (:844): the M tiles are rounded up to a
    multiple of 8 (:845) and the surplus workgroups return at :170.

Where each route rounds (acc = the fp32 MFMA accumulator; bf16(.) = round to nearest even; "out" = the stored C)

    route             pre                                     C                                                 roundings of acc
    ----------------  --------------------------------------  ------------------------------------------------  ----------------
    vec               bf16(f32(bf16(acc)) + bias)             bf16(gate(act(f32(bf16(acc)) + bias)) + residual)  1, then out
                      acc -> bf16: gemm.hip:240; + bias in    act :257-263, gate :264-272, residual :273-283,
                      fp32 :255; pre stored :256              stored :284
    scalar, bf16 out  bf16(acc + bias)   :298-299             bf16(gate(act(acc + bias)) + residual)            0, then out
                                                              :298-308: one rounding, at the store :308
    scalar, fp32 out  (T)(acc + bias)    :299                 the fp32 value itself :308                        0, none
                      (bf16 inputs: one rounding; fp32: none)
    wide              --                                      bf16(acc + bias)   gemm.hip:753-754               0, then out

    Order inside every route: + bias, store pre, activation, gate (ReLU gate: gate > 0 ? v : +0, so a gate of +0.0 or -0.0 closes),
    + residual, store.  gemm_nt_ln_kernel and the persistent feed-forward kernels re-create the vec route's bf16(f32(bf16(acc)) + bias)
    (gemm.hip:421, :579); the fused kernels' tests compare with ops.gemm_nt bit for bit, so the table above is what they are pinned to.

Exact cases (EXACT): operands are small integers and the bias half-integers, every partial sum stays below 2^24, so all fp32 work is
exact and the only inexact steps are the bf16 conversions of the table: emulate() reproduces C and pre bit for bit with torch.bfloat16
on the CPU.  Operand ranges (operand_range): K <= 8: integers in [-15, 15]; 8 < K <= 64: [-10, 10]; K >= 72: [-7, 7]; bias: multiples
of 0.5 in [-2.5, 2.5]; residual: integers in [-64, 64]; ReLU gates: integers in [-2, 2], half of the zeros stored as -0.0.  With these
|acc| passes 256 often enough that the vec route's two roundings and a single rounding of the same inputs part on some percent of the
elements WHEREVER a bias or a residual stands between them (without either the second rounding finds a bf16 number and both routes
store the same bits): a case on the wrong route cannot pass (test_nt_cases_cpu.py asserts >= 1 % on every such case, counting the
elements that a ReLU or a closed gate has not set to zero, and bit equality on the others).

Real-valued cases (REAL): GELU / GELU-tanh activation, GELU gates, `pre` beside them.  bound() / real_ref() is element-wise, local_bounds.py style:
with v = acc + bias (float64), Aabs = |A| |Bt|^T, y the float64 result,

    dv    = n 2^-8 |acc| + K 2^-24 Aabs + 2^-24 |v|                  n: roundings of acc (table: 1 on vec, 0 elsewhere); the last term
                                                                     is the fp32 addition of the bias
    |C - y| <= (1 + 2^-6) (LIP dv + EVAL 2^-24 (|v| + |y| + 1) + u_out |y|) + 2^-109

    LIP: the factor by which the epilogue stretches an error of v.  Activation: |gelu(v + d) - gelu(v)| <= sup |gelu'| |d|.  Gate: the
    output is v g'(u) with u read from memory (exact), so the factor is |g'(u)| <= sup |g'|: the same supremum, as act_gelu_grad IS
    gelu'.  erf form: g'(u) = Phi(u) + u phi(u), g''(u) = phi(u) (2 - u^2) = 0 at u = +-sqrt 2, g' in [-0.128904, 1.128904] and
    -> 0 / 1 at -+ infinity: LIP = Phi(sqrt 2) + sqrt 2 phi(sqrt 2) = 1.128904.  tanh form: no closed form; lipschitz() takes the
    supremum over a float64 grid of spacing 2^-12 on [-12, 12] (beyond it g' is 0 or 1 to 1e-30) plus the grid's own error
    sup |g'''| h^2 / 8 < 1e-7: 1.128993.  test_nt_cases_cpu.py asserts both numbers.
    EVAL: the fp32 evaluation of act_gelu / act_gelu_grad (common.h:237-250: erff / tanhf / __expf, whose device accuracy is
    documented nowhere) and the fp32 product around it.  MEASURED on the MI355X on the fp32 K = 8 cases of REAL (where K 2^-24 Aabs is
    a few 2^-24) as max |got - ref| / (2^-24 (|v| + |ref| + 1)), v the accumulator plus bias of both forms:
        EVAL_MEASURED = 4.55  (GELU 2.33, GELU-tanh 2.46, GELU gate 2.62, GELU-tanh gate 4.55; the figure takes in the few 2^-24 of
                               the other terms at K = 8, so it overstates the evaluation alone)
        EVAL          = 9.1   (factor 2 margin)
    No other term is fitted to a kernel result.  The test prints this measure for every real-valued case.
"""
import itertools
import math

import torch

F32, BF16 = torch.float32, torch.bfloat16
DT = {'f32': F32, 'bf16': BF16}
ES = {'f32': 4, 'bf16': 2}
TILE = 128
CANARY = -24832.0          # -97 * 256: a bf16 number no case can produce (|acc| <= 104 * 49 + 2.5 + 64)
TAIL = 64                  # canary / NaN elements behind every buffer
EXTRA_ROWS = 2             # canary rows of C and pre beyond M
U_BF16, U_F32 = 2.0 ** -8, 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -6
UNDERFLOW = 2.0 ** -109
EVAL_MEASURED = 4.55
EVAL = 2.0 * EVAL_MEASURED
ACT_CODE = {'none': 0, 'relu': 1, 'gelu': 2, 'gelu_tanh': 3}          # B4C_ACT_* of include/b4c.h


def ceil_div(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
def case(why, M, N, K, types='bf16/bf16', bias=False, act='none', gate=None, residual=False, pre=False, expect=None, real=False, **geom):
    """One launch.  types 'T/OutT'; gate None | 'relu' | 'gelu' | 'gelu_tanh'; geom: the pitches lda ldb ldc ldg ldr ldp (default: tight),
    bt_rows (rows of the Bt buffer, default N), and element offsets c_off bias_off gate_off res_off pre_off of the views into their
    buffers (default 0: 16-byte aligned).  expect: (kernel, instantiation or None, xcd_map, tiles_per_chunk or None)."""
    dtype, out = types.split('/')
    c = dict(why=why, M=M, N=N, K=K, dtype=dtype, out=out, bias=bias, act=act, gate=gate, residual=residual, pre=pre, real=real,
             lda=K, ldb=K, ldc=N, ldg=N, ldr=N, ldp=N, bt_rows=N, c_off=0, bias_off=0, gate_off=0, res_off=0, pre_off=0, expect=expect)
    unknown = set(geom) - set(c)
    assert not unknown, unknown
    c.update(geom)
    return c


def case_id(c):
    epi = '+'.join([n for n, on in (('bias', c['bias']), (c['act'], c['act'] != 'none'), ('gate_' + str(c['gate']), c['gate']),
                                    ('res', c['residual']), ('pre', c['pre'])) if on]) or 'plain'
    geom = ','.join('%s=%d' % (k, c[k]) for k, d in (('lda', c['K']), ('ldb', c['K']), ('ldc', c['N']), ('ldg', c['N']), ('ldr', c['N']),
                                                      ('ldp', c['N']), ('bt_rows', c['N']), ('c_off', 0), ('bias_off', 0), ('gate_off', 0),
                                                      ('res_off', 0), ('pre_off', 0)) if c[k] != d)
    return '%dx%dx%d-%s.%s-%s%s' % (c['M'], c['N'], c['K'], c['dtype'], c['out'], epi, '-' + geom if geom else '')


def inst(types, epi, actx):
    t, o = types.split('/')
    return (t, o, bool(epi), bool(actx))


TYPE_PAIRS = ('f32/f32', 'bf16/f32', 'bf16/bf16')
FULL = dict(bias=True, act='relu', gate='relu', residual=True, pre=True)


def _generic(types, epi, actx, xcd, vec=None):
    kernel = ('vec' if types == 'bf16/bf16' else 'scalar') if vec is None else ('vec' if vec else 'scalar')
    return (kernel, inst(types, epi, actx), xcd, None)


def _exact_cases():
    out = []
    # ---- shapes and tile maps
    for t in TYPE_PAIRS:
        out.append(case('one 8-column chunk of one row', 1, 8, 8, t, expect=_generic(t, 0, 0, 0)))
        out.append(case('one chunk, ReLU gate alone', 1, 8, 8, t, gate='relu', expect=_generic(t, 1, 0, 0)))
    out += [
        case('one full tile, one K stage: the gate prefetch is issued in the first and only iteration', 128, 128, 64,
             bias=True, gate='relu', expect=_generic('bf16/bf16', 1, 0, 0)),
        case('the same with the residual as the prefetched operand', 128, 128, 64, bias=True, residual=True,
             expect=_generic('bf16/bf16', 1, 0, 0)),
        case('XCD map: 9 M tiles rounded to 16, the surplus workgroups return early', 1025, 136, 8, **FULL,
             expect=_generic('bf16/bf16', 1, 1, 1)),
        case('XCD map, fp32 output', 1025, 136, 8, 'bf16/f32', bias=True, residual=True, expect=_generic('bf16/f32', 1, 0, 1)),
        case('9 N tiles: no XCD map, ragged M and N', 129, 1032, 72, **FULL, expect=_generic('bf16/bf16', 1, 1, 0)),
        case('fp32: K below one MFMA pair', 129, 136, 4, 'f32/f32', bias=True, act='relu', expect=_generic('f32/f32', 0, 0, 1)),
        case('fp32: exactly one K stage', 129, 136, 32, 'f32/f32', bias=True, gate='relu', expect=_generic('f32/f32', 1, 0, 1)),
        case('fp32: a 4-element tail in the second stage', 129, 136, 36, 'f32/f32', **FULL, expect=_generic('f32/f32', 1, 1, 1)),
    ]
    # ---- every epilogue form on the ragged shape (K: an 8-element tail in the second stage); reaches all 12 instantiations
    for t in TYPE_PAIRS:
        for bias, act, gate, res, pre in itertools.product((False, True), ('none', 'relu'), (None, 'relu'), (False, True), (False, True)):
            out.append(case('epilogue product', 129, 136, 72, t, bias=bias, act=act, gate=gate, residual=res, pre=pre,
                            expect=_generic(t, gate or res, pre, 1)))
    # ---- pitched operands: every operand a view into a larger buffer (NaN around the inputs, a canary around C and pre)
    for t, p in (('bf16/bf16', 8), ('bf16/f32', 8), ('f32/f32', 4)):
        out.append(case('every pitch different, Bt with 5 NaN rows beyond N', 129, 136, 72, t, **FULL, lda=72 + p, ldb=72 + 2 * p,
                        ldc=144, ldg=152, ldr=160, ldp=168, bt_rows=141, expect=_generic(t, 1, 1, 1)))
    out += [
        case('pitched gate alone: the prefetch halves walk ldg', 129, 136, 72, gate='relu', lda=80, ldc=144, ldg=152,
             expect=_generic('bf16/bf16', 1, 0, 1)),
        case('pitched residual alone: the prefetch halves walk ldr', 129, 136, 72, residual=True, ldb=88, ldc=144, ldr=160,
             expect=_generic('bf16/bf16', 1, 0, 1)),
    ]
    # ---- the scalar epilogue with bf16 output
    sc = _generic('bf16/bf16', 1, 1, 1, vec=False)
    out += [
        case('scalar: N % 8 != 0', 129, 50, 72, **FULL, expect=('scalar', inst('bf16/bf16', 1, 1), 0, None)),
        case('scalar: ldc % 8 != 0', 129, 136, 72, **FULL, ldc=140, expect=sc),
        case('scalar: C offset by 2 elements', 129, 136, 72, **FULL, c_off=2, expect=sc),
        case('scalar: bias offset by one float', 129, 136, 72, **FULL, bias_off=1, expect=sc),
        case('scalar: ldg % 8 != 0', 129, 136, 72, **FULL, ldg=140, expect=sc),
        case('scalar: residual offset by 2 elements', 129, 136, 72, **FULL, res_off=2, expect=sc),
        case('scalar: ldp % 8 != 0', 129, 136, 72, **FULL, ldp=140, expect=sc),
        case('scalar: gate offset by 4 elements', 129, 136, 72, **FULL, gate_off=4, expect=sc),
        case('N >= 2048 with a misaligned bias: falls from the wide kernel to the generic one', 129, 2048, 8, bias=True, bias_off=1,
             expect=('scalar', inst('bf16/bf16', 0, 0), 0, None)),
    ]
    # ---- the wide kernel (C on the ops.row_pitch pitch)
    out += [
        case('wide: one tile per chunk', 129, 2048, 8, bias=True, expect=('wide', None, 0, 1)),
        case('wide: 66 x 41 tiles, 21 chunks of 2 tiles, the last holds one; last N tile 8 columns wide', 8321, 5128, 104, bias=True,
             ldc=5248, expect=('wide', None, 0, 2)),
        case('wide: 100 x 53 tiles, 18 chunks of 3 tiles, the last holds two', 12673, 6664, 8, bias=True, ldc=6784,
             expect=('wide', None, 0, 3)),
    ]
    return out


REAL_FORMS = (dict(bias=True, act='gelu'), dict(bias=True, act='gelu_tanh'), dict(gate='gelu'), dict(gate='gelu_tanh'))


def _real_cases():
    """every form with `pre` (the GPU test launches it again without); 'bf16/bf16' twice: on the vec route and, with ldc % 8 != 0, on
    the scalar one.  The fp32 K = 8 cases are the ones EVAL was measured on."""
    out = []
    for M, N, K in ((129, 136, 72), (37, 104, 128)):
        for form in REAL_FORMS:
            epi = form.get('gate') is not None
            out.append(case('real, vec', M, N, K, 'bf16/bf16', pre=True, real=True, expect=('vec', inst('bf16/bf16', epi, 1), N > 128, None), **form))
            out.append(case('real, bf16 output forced onto the scalar route', M, N, K, 'bf16/bf16', pre=True, real=True, ldc=N + 4,
                            expect=('scalar', inst('bf16/bf16', epi, 1), N > 128, None), **form))
            for t in ('bf16/f32', 'f32/f32'):
                out.append(case('real', M, N, K, t, pre=True, real=True, expect=('scalar', inst(t, epi, 1), N > 128, None), **form))
    for form in REAL_FORMS:
        out.append(case('real, fp32 K = 8: the evaluation term dominates', 129, 136, 8, 'f32/f32', pre=True, real=True,
                        expect=('scalar', inst('f32/f32', form.get('gate') is not None, 1), 1, None), **form))
    return out


EXACT = _exact_cases()
REAL = _real_cases()
# the two cases above a few MB: compared in row blocks
BLOCK_ROWS = 2048


# ------------------------------------------------------------------------------------------------------------------
# the host's dispatch, restated
# ------------------------------------------------------------------------------------------------------------------
def route(c):
    """What b4c_gemm_nt_act launches for this case (gemm.hip:829-872): {'kernel', 'inst', 'xcd_map', 'blocks'} and for 'wide' also
    'mt', 'chunks', 'tiles_per_chunk'."""
    M, N, K = c['M'], c['N'], c['K']
    bf_in, bf_out = c['dtype'] == 'bf16', c['out'] == 'bf16'
    gate, res, pre, bias = c['gate'] is not None, c['residual'], c['pre'], c['bias']

    def aligned(off, es):
        return (off * es) % 16 == 0
    c_al, bias_al = aligned(c['c_off'], ES[c['out']]), aligned(c['bias_off'], 4)
    # vec_ok_wide, gemm.hip:778-780
    wide_ok = N % 8 == 0 and c['ldc'] % 8 == 0 and c_al and (not bias or bias_al)
    if bf_in and bf_out and K <= 128 and N >= 2048 and c['act'] == 'none' and not gate and not res and not pre and wide_ok:   # :830-831
        mt, ntn = ceil_div(M, TILE), ceil_div(N, TILE)                                                                     # :832
        chunks = max(1, min(ceil_div(512 * 5, mt), ntn))                                                                  # :833-835
        tpc = ceil_div(ntn, chunks)                                                                                       # :836
        chunks = ceil_div(ntn, tpc)                                                                                       # :837
        return dict(kernel='wide', inst=None, xcd_map=0, mt=mt, chunks=chunks, tiles_per_chunk=tpc, blocks=mt * chunks)   # :840
    mt_n, nt_n = ceil_div(M, TILE), ceil_div(N, TILE)                                                                     # :843
    xcd = 1 if 1 < nt_n <= 8 else 0                                                                                       # :844
    blocks = (ceil_div(mt_n, 8) * 8 if xcd else mt_n) * nt_n                                                              # :845
    es = ES[c['dtype']]
    vec_ok = (N % 8 == 0 and c['ldc'] % 8 == 0 and c_al and                                                               # :851
              (not gate or (c['ldg'] % 8 == 0 and aligned(c['gate_off'], es))) and                                        # :852
              (not res or (c['ldr'] % 8 == 0 and aligned(c['res_off'], es))) and                                          # :853
              (not bias or bias_al) and                                                                                   # :854
              (not pre or (c['ldp'] % 8 == 0 and aligned(c['pre_off'], es))))                                             # :855
    epi = gate or res                                                                                                     # :867
    actx = pre or c['act'] in ('gelu', 'gelu_tanh') or (gate and c['gate'] != 'relu')                                     # :869
    out_t = 'f32' if not bf_in else c['out']                                                                              # :870-872
    kernel = 'vec' if (out_t == 'bf16' and vec_ok) else 'scalar'                                                          # :171
    return dict(kernel=kernel, inst=(c['dtype'], out_t, bool(epi), bool(actx)), xcd_map=xcd, blocks=blocks)


def expected_route(c):
    """route() in the form of a case's `expect`"""
    r = route(c)
    return (r['kernel'], r['inst'], r['xcd_map'], r.get('tiles_per_chunk'))


def rounding(c):
    """'double' (vec), 'single' (one bf16 rounding: scalar with bf16 output, wide) or 'none' (fp32 output): the table's last column"""
    r = route(c)
    if c['out'] == 'f32':
        return 'none'
    return 'double' if r['kernel'] == 'vec' else 'single'


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def operand_range(K):
    return 15 if K <= 8 else 10 if K <= 64 else 7


def _gen(c, salt=0):
    s = 0
    for k in (c['M'], c['N'], c['K'], ES[c['dtype']], ES[c['out']], int(c['bias']), ACT_CODE[c['act']], ACT_CODE[c['gate'] or 'none'],
              int(c['residual']), int(c['pre']), c['ldc'], c['c_off'], salt):
        s = (s * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _pitched(x, ld, off, rows_alloc, fill, dtype):
    """x [rows, width] inside a `fill`-filled flat buffer: element (r, j) at off + r * ld + j; rows_alloc >= rows; TAIL behind"""
    rows, width = x.shape
    buf = torch.full((off + rows_alloc * ld + TAIL,), fill, dtype=dtype)
    torch.as_strided(buf, (rows, width), (ld, 1), off).copy_(x.to(dtype))
    return buf


def view(c, name, buf, rows=None):
    """the [rows, width] view of operand `name` ('A' 'Bt' 'C' 'gate' 'res' 'pre' 'bias') into its flat buffer, on buf's device"""
    M, N, K = c['M'], c['N'], c['K']
    if name == 'bias':
        return buf[c['bias_off']:c['bias_off'] + N]
    ld, off, r, w = {'A': (c['lda'], 0, M, K), 'Bt': (c['ldb'], 0, c['bt_rows'], K), 'C': (c['ldc'], c['c_off'], M, N),
                     'gate': (c['ldg'], c['gate_off'], M, N), 'res': (c['ldr'], c['res_off'], M, N),
                     'pre': (c['ldp'], c['pre_off'], M, N)}[name]
    return torch.as_strided(buf, (r if rows is None else rows, w), (ld, 1), off)


def out_buffer(c, name):
    """the canary-filled flat buffer of 'C' or 'pre' (M + EXTRA_ROWS rows and a TAIL)"""
    ld, off, dt = (c['ldc'], c['c_off'], DT[c['out']]) if name == 'C' else (c['ldp'], c['pre_off'], DT[c['dtype']])
    return torch.full((off + (c['M'] + EXTRA_ROWS) * ld + TAIL,), CANARY, dtype=dt)


def inputs(c):
    """The flat CPU buffers of the launch's inputs, {'A', 'Bt', 'bias', 'gate', 'res'} (None where the case has none), in the storage
    types.  Around every view the buffers hold NaN; Bt's rows beyond N are NaN.  Exact cases: integers / half-integers (module
    docstring); real cases: the distribution of tests/test_gpu_gelu.py (acc + bias and the gate span about [-4, 4])."""
    M, N, K, T = c['M'], c['N'], c['K'], DT[c['dtype']]
    g = _gen(c)
    nan = float('nan')
    if c['real']:
        a = torch.randn(M, K, generator=g)
        bt = torch.randn(N, K, generator=g) * (1.55 / K ** 0.5)
        bias = torch.randn(N, generator=g) * 0.4
        gate = torch.randn(M, N, generator=g) * 1.6
        res = torch.randn(M, N, generator=g)
    else:
        r = operand_range(K)
        a = torch.randint(-r, r + 1, (M, K), generator=g).float()
        bt = torch.randint(-r, r + 1, (N, K), generator=g).float()
        bias = torch.randint(-5, 6, (N,), generator=g).float() * 0.5
        gate = torch.randint(-2, 3, (M, N), generator=g).float()
        neg0 = (gate == 0) & (torch.rand(M, N, generator=g) < 0.5)
        gate = torch.where(neg0, torch.full((), -0.0), gate)
        gate[0, :8] = torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, -0.0, 0.0])      # planted: the one-chunk cases see every kind
        res = torch.randint(-64, 65, (M, N), generator=g).float()
    btf = torch.full((c['bt_rows'], K), nan)
    btf[:N] = bt
    out = {'A': _pitched(a, c['lda'], 0, M, nan, T), 'Bt': _pitched(btf, c['ldb'], 0, c['bt_rows'], nan, T),
           'bias': None, 'gate': None, 'res': None}
    if c['bias']:
        out['bias'] = torch.full((c['bias_off'] + N + TAIL,), nan)
        out['bias'][c['bias_off']:c['bias_off'] + N] = bias
    if c['gate'] is not None:
        out['gate'] = _pitched(gate, c['ldg'], c['gate_off'], M, nan, T)
    if c['residual']:
        out['res'] = _pitched(res, c['ldr'], c['res_off'], M, nan, T)
    return out


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def bf16r(x):
    return x.to(BF16).to(x.dtype)


# ------------------------------------------------------------------------------------------------------------------
# exact emulation
# ------------------------------------------------------------------------------------------------------------------
WRONG = ('rounding', 'gate_ge', 'bias_after_act', 'res_before_gate', 'pre_after_act')        # arithmetic mutants of emulate()
WRONG_BUFFER = ('row_from_next_tile', 'chunk_shifted', 'canary')                             # mutants of the stored buffers


def applies(c, wrong):
    """whether the mutant changes what this case stores"""
    return {'rounding': c['out'] == 'bf16' and (c['bias'] or c['residual']),
            'gate_ge': c['gate'] == 'relu',
            'bias_after_act': c['bias'] and c['act'] == 'relu',
            'res_before_gate': c['gate'] == 'relu' and c['residual'],
            'pre_after_act': c['pre'] and c['act'] == 'relu',
            'row_from_next_tile': c['M'] > TILE,
            'chunk_shifted': c['N'] >= 16,
            'canary': True}[wrong]


def emulate(c, inp, r0=0, r1=None, wrong=None, kind=None):
    """Rows r0 .. r1 of what the launch stores: {'C': [rows, N] OutT, 'pre': [rows, N] T or None}, bit for bit for the exact cases (act none
    / ReLU, ReLU gate).  kind: the rounding order ('double' | 'single' | 'none'), default the case's route's.  wrong: one of WRONG."""
    assert not c['real'] and c['act'] in ('none', 'relu') and c['gate'] in (None, 'relu') and wrong in (None,) + WRONG
    M, N, K = c['M'], c['N'], c['K']
    r1 = M if r1 is None else min(r1, M)
    kind = kind or rounding(c)
    if wrong == 'rounding':
        kind = {'double': 'single', 'single': 'double'}[kind]
    a = view(c, 'A', inp['A'])[r0:r1].float()
    bt = view(c, 'Bt', inp['Bt'])[:N].float()
    # every product and every partial sum is an integer below 2^24: exact in fp32 in any summation order
    assert K * float(a.abs().max()) * float(bt.abs().max()) < 2.0 ** 24 and bool((a == a.round()).all()) and bool((bt == bt.round()).all())
    acc = a @ bt.T
    bias = view(c, 'bias', inp['bias']) if c['bias'] else torch.zeros(N)
    if kind == 'double':
        acc = bf16r(acc)                                           # gemm.hip:240
    v = acc if wrong == 'bias_after_act' else acc + bias           # :255 / :298 / :753
    pre = v
    if c['act'] == 'relu':
        v = torch.clamp_min(v, 0.0)                                # :257-259 / :300
    if wrong == 'bias_after_act':
        v = v + bias
    if wrong == 'pre_after_act':
        pre = v
    res = view(c, 'res', inp['res'])[r0:r1].float() if c['residual'] else None
    if wrong == 'res_before_gate' and res is not None:
        v = v + res
    if c['gate'] is not None:
        g = view(c, 'gate', inp['gate'])[r0:r1].float()
        v = torch.where((g >= 0) if wrong == 'gate_ge' else (g > 0), v, torch.zeros(()))      # :271 / :305
    if res is not None and wrong != 'res_before_gate':
        v = v + res                                                # :277 / :282 / :307
    return {'C': v.to(DT[c['out']]), 'pre': pre.to(DT[c['dtype']]) if c['pre'] else None}


def row_blocks(c):
    big = c['M'] * c['N'] > (1 << 22)
    step = BLOCK_ROWS if big else c['M']
    return [(r0, min(r0 + step, c['M'])) for r0 in range(0, c['M'], step)]


def emulate_buffers(c, inp, wrong=None):
    """the flat buffers the launch leaves ({'C', 'pre'}: canary everywhere outside [M, N]); wrong: WRONG or WRONG_BUFFER"""
    bufs = {'C': out_buffer(c, 'C'), 'pre': out_buffer(c, 'pre') if c['pre'] else None}
    arith = wrong if wrong in WRONG else None
    for r0, r1 in row_blocks(c):
        e = emulate(c, inp, r0, r1, wrong=arith)
        for n in ('C', 'pre'):
            if bufs[n] is not None:
                view(c, n, bufs[n])[r0:r1] = e[n]
    for n in ('C', 'pre'):
        if bufs[n] is None:
            continue
        v = view(c, n, bufs[n])
        if wrong == 'row_from_next_tile':          # the last row of the first M tile holds the last row of the second
            v[TILE - 1] = v[min(2 * TILE - 1, c['M'] - 1)].clone()
        elif wrong == 'chunk_shifted':             # the second 8-column chunk of the last row holds the first
            v[c['M'] - 1, 8:16] = v[c['M'] - 1, 0:8].clone()
        elif wrong == 'canary':                    # the element behind the last stored one: a pad column, or row M on a tight pitch
            ld, off = (c['ldc'], c['c_off']) if n == 'C' else (c['ldp'], c['pre_off'])
            bufs[n][off + (c['M'] - 1) * ld + c['N']] = 1.0
    return bufs


def check_canary(c, name, buf):
    """nothing outside [M, N] of the view was written: the offset in front, the pad columns of every row, every row beyond M, the tail.
    Runs on buf's device."""
    ld, off = (c['ldc'], c['c_off']) if name == 'C' else (c['ldp'], c['pre_off'])
    M, N = c['M'], c['N']
    want = int(bits(torch.full((1,), CANARY, dtype=buf.dtype))[0])
    b = bits(buf)
    assert bool((b[:off] == want).all()), '%s of %s: wrote in front of the view' % (name, case_id(c))
    if ld > N:
        pad = torch.as_strided(b, (M, ld - N), (ld, 1), off + N)
        assert bool((pad == want).all()), '%s of %s: wrote into the pad columns (first at %s)' % (name, case_id(c), (pad != want).nonzero()[0].tolist())
    assert bool((b[off + M * ld:] == want).all()), '%s of %s: wrote beyond row M' % (name, case_id(c))


def check_exact(c, inp, got):
    """THE exact comparison.  got: {'C': flat buffer, 'pre': flat buffer or None} as the launch left them (any device): the [M, N] views
    equal emulate() bit for bit (fp32 output: also the float64 reference), everything else still holds the canary."""
    names = ['C'] + (['pre'] if c['pre'] else [])
    for n in names:
        check_canary(c, n, got[n])
    for r0, r1 in row_blocks(c):
        e = emulate(c, inp, r0, r1)
        for n in names:
            g = view(c, n, got[n])[r0:r1].cpu()
            same = bits(g) == bits(e[n])
            if not bool(same.all()):
                bad = (~same).nonzero()
                i, j = int(bad[0][0]), int(bad[0][1])
                raise AssertionError('%s of %s (%s): %d of %d elements differ from the emulation, first at (%d, %d): got %r, want %r' %
                                     (n, case_id(c), route(c)['kernel'], len(bad), same.numel(), r0 + i, j, float(g[i, j]), float(e[n][i, j])))
        if c['out'] == 'f32':
            ref = exact_ref64(c, inp, r0, r1)
            assert torch.equal(view(c, 'C', got['C'])[r0:r1].cpu().double(), ref), 'C of %s: differs from the float64 reference' % case_id(c)


def exact_ref64(c, inp, r0, r1):
    """the float64 reference of C for an exact case (no rounding anywhere)"""
    a = view(c, 'A', inp['A'])[r0:r1].double()
    bt = view(c, 'Bt', inp['Bt'])[:c['N']].double()
    v = a @ bt.T
    if c['bias']:
        v = v + view(c, 'bias', inp['bias']).double()
    if c['act'] == 'relu':
        v = torch.relu(v)
    if c['gate'] is not None:
        v = torch.where(view(c, 'gate', inp['gate'])[r0:r1].double() > 0, v, torch.zeros((), dtype=torch.float64))
    if c['residual']:
        v = v + view(c, 'res', inp['res'])[r0:r1].double()
    return v


# ------------------------------------------------------------------------------------------------------------------
# real-valued cases: float64 reference and element-wise bound
# ------------------------------------------------------------------------------------------------------------------
def gelu64(name, z):
    return torch.nn.functional.gelu(z, approximate={'gelu': 'none', 'gelu_tanh': 'tanh'}[name])


def gelu_grad64(name, u):
    """d gelu / d u in closed form (float64): what act_gelu_grad (common.h:242-249) evaluates in fp32"""
    if name == 'gelu':
        return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    k = math.sqrt(2 / math.pi)
    t = torch.tanh(k * (u + 0.044715 * u ** 3))
    return 0.5 * (1 + t) + 0.5 * u * (1 - t * t) * k * (1 + 3 * 0.044715 * u * u)


_LIP = {}


def lipschitz(name):
    """sup |gelu'| (module docstring): the closed form for the erf form, a float64 grid for the tanh form"""
    if name not in _LIP:
        if name == 'gelu':
            s2 = math.sqrt(2.0)
            _LIP[name] = 0.5 * (1 + math.erf(1.0)) + s2 * math.exp(-1.0) / math.sqrt(2 * math.pi)
        else:
            u = torch.arange(-12 * 4096, 12 * 4096 + 1, dtype=torch.float64) / 4096
            _LIP[name] = float(gelu_grad64(name, u).abs().max()) + 1e-7
    return _LIP[name]


def real_ref(c, inp):
    """-> {'v': acc + bias, 'C': reference, 'bound': per element, 'n': roundings of acc}, float64"""
    assert c['real'] and not c['residual']
    a = view(c, 'A', inp['A']).double()
    bt = view(c, 'Bt', inp['Bt'])[:c['N']].double()
    acc = a @ bt.T
    aabs = a.abs() @ bt.abs().T
    v = acc + (view(c, 'bias', inp['bias']).double() if c['bias'] else 0.0)
    n = 1 if rounding(c) == 'double' else 0
    dv = n * U_BF16 * acc.abs() + c['K'] * U_F32 * aabs + U_F32 * v.abs()
    if c['gate'] is not None:
        y = v * gelu_grad64(c['gate'], view(c, 'gate', inp['gate']).double())
        lip = lipschitz(c['gate'])
    else:
        y = gelu64(c['act'], v)
        lip = lipschitz(c['act'])
    u_out = U_BF16 if c['out'] == 'bf16' else U_F32
    b = lip * dv + EVAL * U_F32 * (v.abs() + y.abs() + 1.0) + u_out * y.abs()
    return {'v': v, 'C': y, 'bound': b * SECOND_ORDER + UNDERFLOW, 'n': n}


def eval_ratio(got, ref):
    """the measure EVAL was taken with: max |got - ref| / (2^-24 (|v| + |ref| + 1))"""
    return float(((got.double() - ref['C']).abs() / (U_F32 * (ref['v'].abs() + ref['C'].abs() + 1.0))).max())


def real_emulate(c, inp):
    """the kernel's rounding steps in float32 torch math: the bf16 conversions where the table has them, the activation in fp32"""
    a = view(c, 'A', inp['A']).float()
    bt = view(c, 'Bt', inp['Bt'])[:c['N']].float()
    acc = a @ bt.T
    if rounding(c) == 'double':
        acc = bf16r(acc)
    v = acc + view(c, 'bias', inp['bias']) if c['bias'] else acc
    pre = v.to(DT[c['dtype']])
    if c['gate'] is not None:
        y = v * gelu_grad64(c['gate'], view(c, 'gate', inp['gate']).float())
    else:
        y = gelu64(c['act'], v)
    assert y.dtype == F32
    return {'C': y.to(DT[c['out']]), 'pre': pre}


def bound(c, inp=None):
    """the element-wise bound of a real-valued case's C (real_ref's, for the case's committed inputs unless others are given)"""
    return real_ref(c, inputs(c) if inp is None else inp)['bound']
