"""The candidate-list losses of include/b4c.h restated in numpy, their derived fp32 error bounds, and the committed
cases of the GPU tests (shared with the CPU tests: same seeds, same inputs).

restate(...) evaluates the definition -- scores, per-row loss, coefficients g, dh, dW, db -- in float64, or (dtype=np.float32) with
EVERY intermediate rounded to float32: sequential sums, one rounding per operation.  The float32 mode is not the kernel; it is a
second, independent fp32 evaluation, and its distance from float64 measures what the derived bound below leaves out (the
transcendental functions and the few roundings around them).

Derived bound, per element, u = 2^-24, gamma_n = n u / (1 - n u) (the style of tests/local_bounds.py; bf16 operands are exact in
fp32 and so are their products, so only the fp32 sums round):
    score   ds_c   = gamma_{K+1} (sum_k |h_k w_ck| + |b_c|)
    bce     dl     = sum_{present c} ds_c + gamma_{C+8} sum_c |term_c|          softplus is 1-Lipschitz
            dg_c   = ds_c / 4 + 8 u |g_c|                                       sigma is 1/4-Lipschitz
    softmax dl     = 2 max_c ds_c + 8 u (|m - s_0| + |log sum| + |l|)
            dg_c   = 2 max_c ds_c + u p_c (|s_c - m| + 8) + 8 u |g_c|          (the exponent's argument is rounded before exp)
    dh      gs (sum_c dg_c |w_ck| + gamma_{C+2} sum_c |g_c w_ck|)   [+ 2^-8 |dh| for the one bf16 rounding of the stored value]
    dW      gs sum_{(r,c) -> v} dg |h_rk| + gamma_{n_v+3} (|G0| + gs sum |g h_rk|),   n_v adds into row v; db alike
An element whose bound is 0 (ignored rows, absent entries, rows no list names) must be exact.  The GATE of the GPU tests is this
bound times max(2, 2 x MEASURED_RATIO), MEASURED_RATIO = the worst |float32 mode - float64| / bound over the committed cases,
measured on the CPU (tests/test_candidate_loss_cpu.py::test_measured_ratio_is_current recomputes it)."""
import numpy as np

U_F32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
KINDS = ('bce', 'softmax')
# worst |float32 mode - float64| in units of the derived bound over CASES x KINDS x dtypes x row_off (measured on the CPU; see above)
MEASURED_RATIO = 0.063       # (case (1, 1, 8, 5): 0.0626; every other case below 0.02) -> the gate is 2 x the derived bound


def gamma(n):
    return n * U_F32 / (1.0 - n * U_F32)


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1, e) / (1 + e)


def restate(h, W, b, cand, kind, gscale=None, G0=None, dtype=np.float64):
    """h [R, K], W [V, K] (the table rows row_off .. row_off + V, already rounded to the compute dtype), b [V], cand int [R, C].
    -> dict: present [R, C], valid [R], s [R, C] (0 where absent), item [R], g [R, C], loss, gs, dh [R, K], dW [V, K], db [V]
    (dW / db on top of G0 = (dW0, db0) when given).  gscale None: 1 / max(#valid rows, 1)."""
    f = dtype
    h, W, b = np.asarray(h, f), np.asarray(W, f), np.asarray(b, f)
    cand = np.asarray(cand)
    R, K = h.shape
    V = W.shape[0]
    C = cand.shape[1]
    present = (cand >= 0) & (cand < V)
    valid = present[:, 0]
    present = present & valid[:, None]
    ids = np.where(present, cand, 0)
    Wc = W[ids]                                            # [R, C, K]
    s = np.zeros((R, C), f)
    for k in range(K):                                     # sequential: every partial sum is rounded to `dtype`
        s = s + h[:, k, None] * Wc[:, :, k]
    s = np.where(present, s + b[ids], f(0))
    first = np.zeros((R, C), bool)
    first[:, 0] = True
    if kind == 'bce':
        x = np.where(first, -s, s)
        term = np.where(present, _softplus(x).astype(f), f(0))
        g = np.where(present, np.where(first, -1, 1) * _sigmoid(x), 0).astype(f)
        m = lse = None
    else:
        sm = np.where(present, s, -np.inf)
        m = np.where(valid, sm.max(1), f(0)).astype(f)
        e = np.where(present, np.exp((s - m[:, None]).astype(f)), f(0)).astype(f)
        tot = np.zeros(R, f)
        for c in range(C):
            tot = tot + e[:, c]
        tot = np.where(valid, tot, f(1))
        lse = np.log(tot).astype(f)
        p = (e / tot[:, None]).astype(f)
        g = np.where(present, p - first, 0).astype(f)
        term = np.where(first & present, ((m - s[:, 0]) + lse)[:, None], f(0)).astype(f)
    item = np.zeros(R, f)
    for c in range(C):
        item = item + term[:, c]
    nvalid = int(valid.sum())
    gs = f(1.0 / max(nvalid, 1) if gscale is None else gscale)
    loss = f(0)
    for r in range(R):
        loss = f(loss + item[r])
    loss = f(loss * gs)
    gg = (gs * g).astype(f)
    dh = np.zeros((R, K), f)
    for c in range(C):
        dh = dh + gg[:, c, None] * Wc[:, c, :]
    dW = np.zeros((V, K), f) if G0 is None else np.array(G0[0], f)
    db = np.zeros(V, f) if G0 is None else np.array(G0[1], f)
    rr, cc = np.nonzero(present)
    np.add.at(dW, ids[rr, cc], (gg[rr, cc, None] * h[rr]).astype(f))
    np.add.at(db, ids[rr, cc], gg[rr, cc])
    return dict(present=present, valid=valid, ids=ids, s=s, item=item, g=g, loss=loss, gs=gs, dh=dh, dW=dW, db=db, m=m, lse=lse)


def bounds(h, W, b, ref, kind, G0=None, bf16=False):
    """the derived bound (module docstring) of every output of restate(..., dtype=float64) = ref -> dict like ref's"""
    h, W, b = np.asarray(h, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    present, ids, s, g, gs = ref['present'], ref['ids'], ref['s'], ref['g'], float(ref['gs'])
    R, K = h.shape
    V = W.shape[0]
    C = present.shape[1]
    Wa = np.abs(W)[ids] * present[:, :, None]              # [R, C, K], 0 where absent
    ha = np.abs(h)
    ds = gamma(K + 1) * (np.einsum('rk,rck->rc', ha, Wa) + np.abs(b)[ids]) * present
    if kind == 'bce':
        first = np.zeros((R, C), bool)
        first[:, 0] = True
        term = _softplus(np.where(first, -s, s)) * present
        d_item = ds.sum(1) + gamma(C + 8) * term.sum(1)
        dg = (ds / 4 + 8 * U_F32 * np.abs(g)) * present
    else:
        dmax = ds.max(1)
        m, lse = ref['m'], ref['lse']
        d_item = (2 * dmax + 8 * U_F32 * (np.abs(m - s[:, 0]) + np.abs(lse) + np.abs(ref['item']))) * ref['valid']
        if C == 1:
            d_item = d_item * 0                            # the definition: exactly 0
        p = g + (np.arange(C) == 0)[None, :]
        dg = (2 * dmax[:, None] + U_F32 * p * (np.abs(s - m[:, None]) + 8) + 8 * U_F32 * np.abs(g)) * present
        if C == 1:
            dg = dg * 0
    d_loss = gs * d_item.sum() + gamma(R + 2) * gs * np.abs(ref['item']).sum()
    ga = np.abs(g)
    d_dh = gs * (np.einsum('rc,rck->rk', dg, Wa) + gamma(C + 2) * np.einsum('rc,rck->rk', ga, Wa))
    if bf16:
        d_dh = d_dh + U_BF16 * np.abs(ref['dh'])
    rr, cc = np.nonzero(present & (ga + dg > 0))
    n_v = np.zeros(V)
    np.add.at(n_v, ids[rr, cc], 1.0)
    eW, aW = np.zeros((V, K)), np.zeros((V, K)) if G0 is None else np.abs(np.asarray(G0[0], np.float64))
    eb, ab = np.zeros(V), np.zeros(V) if G0 is None else np.abs(np.asarray(G0[1], np.float64))
    np.add.at(eW, ids[rr, cc], gs * dg[rr, cc, None] * ha[rr])
    np.add.at(aW, ids[rr, cc], gs * ga[rr, cc, None] * ha[rr])
    np.add.at(eb, ids[rr, cc], gs * dg[rr, cc])
    np.add.at(ab, ids[rr, cc], gs * ga[rr, cc])
    touched = n_v > 0
    d_dW = (eW + gamma(n_v + 3)[:, None] * aW) * touched[:, None]
    d_db = (eb + gamma(n_v + 3) * ab) * touched
    return dict(s=ds, item=d_item, g=dg, loss=d_loss, dh=d_dh, dW=d_dW, db=d_db)


# ---- the committed cases ------------------------------------------------------------------------------------------------------
# (R, C, K, V, operand scale); every size at which the kernels take another lane layout (K / 8 chunks: 1, 8, 16, 17 -> 32 lanes, 128
# -> two chunks per lane), one row, rows that are no multiple of anything, C below / above one wave's positions and at B4C_MAX_CAND.
# (67, 101, 128, 50): every item is listed many times -- the atomic collision case.  The last case: |s| about 100.
CASES = [(1, 1, 8, 5, 0.5), (5, 2, 64, 50, 0.5), (67, 101, 128, 50, 0.3), (300, 7, 136, 1000, 0.3), (3, 1024, 1024, 2000, 0.1),
         (5, 2, 64, 50, 3.5)]
ROW_OFFS = (0, 10)


def inputs(R, C, K, V, scale, bf16, seed=0):
    """-> h [R, K], table [V + 13, K], b [V] (fp32; h bf16-representable when bf16), cand int32 [R, C]: column 0 the target, rows with
    an invalid target (-1 and V + 3), absent entries in the middle of a list and a repeated id, where the shape has room"""
    rng = np.random.default_rng(1000 * R + C + K + seed)
    h = (rng.standard_normal((R, K)) * scale).astype(np.float32)
    table = (rng.standard_normal((V + 13, K)) * scale).astype(np.float32)
    b = (rng.standard_normal(V) * 0.5).astype(np.float32)
    cand = rng.integers(0, V, size=(R, C)).astype(np.int32)
    if R >= 3:
        cand[1, 0] = -1
        cand[R - 1, 0] = V + 3
    if C >= 3:
        cand[0, C // 2] = -1
        cand[R // 2, 1] = V
        cand[0, C - 1] = cand[0, 0]                        # the target once more, as a negative
    if C >= 4:
        cand[R // 2, 3] = cand[R // 2, 2]
    if bf16:
        import torch
        h = torch.from_numpy(h).bfloat16().float().numpy()
    return h, table, b, cand


def operand_rows(table, row_off, V, bf16):
    """the rows the kernel reads as items 0 .. V - 1, as the products see them (rounded to bf16 for a bf16 h)"""
    W = table[row_off:row_off + V]
    if bf16:
        import torch
        W = torch.from_numpy(np.ascontiguousarray(W)).bfloat16().float().numpy()
    return W


def measured_ratio(cases=None):
    """worst |float32 mode - float64| / derived bound over the committed cases (CPU only; a few seconds)"""
    worst = 0.0
    for R, C, K, V, scale in (cases or CASES):
        for bf16 in (False, True):
            for off in ROW_OFFS:
                h, table, b, cand = inputs(R, C, K, V, scale, bf16)
                W = operand_rows(table, off, V, bf16)
                for kind in KINDS:
                    r64 = restate(h, W, b, cand, kind)
                    r32 = restate(h, W, b, cand, kind, dtype=np.float32)
                    bd = bounds(h, W, b, r64, kind)
                    for name in ('item', 'g', 'dh', 'dW', 'db'):
                        err = np.abs(np.asarray(r32[name], np.float64) - r64[name])
                        pos = bd[name] > 0
                        assert not err[~pos].any(), (name, 'not exact where the bound is 0')
                        if pos.any():
                            worst = max(worst, float((err[pos] / bd[name][pos]).max()))
    return worst
