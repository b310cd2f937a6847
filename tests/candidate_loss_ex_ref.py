"""The extended candidate-list losses of include/b4c.h restated in numpy -- BPR, the weighted binary cross-entropy
(gBCE) and the per-item score correction (logQ) --, their derived fp32 error bounds, and the settings of the GPU tests.  The
inputs, the committed shapes and the helpers are those of tests/candidate_loss_ref.py (same seeds, same cases); this module adds
the correction vector of a case, generated from a seed.

restate(...) evaluates the definition in float64, or (dtype=np.float32) with EVERY intermediate rounded to float32: sequential
sums, one rounding per operation.  As in candidate_loss_ref the float32 mode is not the kernel; it is a second, independent fp32
evaluation, and its distance from float64 measures what the derived bound leaves out (the transcendental functions and the few
roundings around them).

Derived bound, per element, u = 2^-24, gamma_n as there.  ds_c is candidate_loss_ref's bound of a score.  corr is an exact fp32
input, so the corrected score z_c = s_c - corr[id_c] carries one more rounding:
    z       dz_c   = ds_c + u |z_c| where corrected, ds_c elsewhere
    bce     the bound of candidate_loss_ref over z, with beta on the target's term and on its bound:
            dl     = beta dz_0 + sum_{c >= 1} dz_c + gamma_{C+8} sum_c |term_c|          term_0 = beta softplus(-z_0)
            dg_0   = beta dz_0 / 4 + 8 u |g_0|,   dg_c = dz_c / 4 + 8 u |g_c|
    softmax the bound of candidate_loss_ref with z for s and dz for ds
    bpr     x_c = z_c - z_0:   dx_c = dz_c + dz_0 + u |x_c|
            dl     = sum_c dx_c + gamma_{C+8} sum_c |term_c|                               softplus is 1-Lipschitz
            dg_c   = dx_c / 4 + 8 u |g_c|                                                  sigma is 1/4-Lipschitz
            dg_0   = sum_c dg_c + gamma_C sum_c |g_c|                                      the sum of the C - 1 coefficients
            (a row without a present negative: every bound 0 -- loss and coefficients are exactly 0)
    scores  ds_c: `scores` holds the uncorrected s
    dh, dW, db, loss: candidate_loss_ref's, from dg and g (b4c_candidate_loss_bwd is unchanged)
An element whose bound is 0 must be exact.  The GATE of the GPU tests is this bound times max(2, 2 x MEASURED_RATIO_EX),
MEASURED_RATIO_EX = the worst |float32 mode - float64| / bound over CASES x ROW_OFFS x dtypes x SETTINGS, measured on the CPU
(tests/test_candidate_loss_ex_cpu.py::test_measured_ratio_ex_is_current recomputes it: the constant is at least the recomputed
value and within 10 % of it)."""
import numpy as np

from candidate_loss_ref import CASES, ROW_OFFS, U_BF16, U_F32, _sigmoid, _softplus, gamma, inputs, operand_rows  # noqa: F401

KINDS = ('bce', 'softmax', 'bpr')
# (kind, beta, with corr, correct_target): the settings of the GPU grid
SETTINGS = (('bpr', 1.0, False, False), ('bpr', 1.0, True, False), ('bce', 0.37, True, False), ('softmax', 1.0, True, False),
            ('softmax', 1.0, True, True))
# worst |float32 mode - float64| in units of the derived bound over CASES x ROW_OFFS x dtypes x SETTINGS (measured on the CPU; see above)
MEASURED_RATIO_EX = 0.056      # (case (1, 1, 8, 5), weighted bce with corr: 0.0552; every other below 0.035) -> the gate is 2 x the bound


def setting_id(setting):
    kind, beta, with_corr, target = setting
    return kind + ('' if beta == 1.0 else '-beta%g' % beta) + ('-corr' if with_corr else '') + ('-target' if target else '')


def gbce_beta(N, V, t):
    """gSASRec: beta = alpha (t (1 - 1 / alpha) + 1 / alpha), alpha = N / (V - 1)"""
    alpha = N / (V - 1.0)
    return alpha * (t * (1.0 - 1.0 / alpha) + 1.0 / alpha)


def item_counts(V, seed=0):
    """Zipf-like integer counts of V items in a seeded order, about a tenth of the items at count 0 (at least one item counted)"""
    rng = np.random.default_rng(77 + seed)
    cnt = np.floor(3000.0 / np.arange(1, V + 1) ** 1.1).astype(np.int64) + rng.integers(0, 3, size=V)
    cnt[rng.random(V) < 0.1] = 0
    cnt = cnt[rng.permutation(V)]
    if not cnt.any():
        cnt[0] = 1
    return cnt


def log_expected_count(cnt, N):
    """log(N count_v / total) in fp32, 0 where the count is 0: what cloze.log_expected_count returns"""
    cnt = np.asarray(cnt, np.float64)
    q = cnt * (float(N) / cnt.sum())
    return np.where(cnt > 0, np.log(np.where(cnt > 0, q, 1.0)), 0.0).astype(np.float32)


def corr_for(C, V, seed=0):
    """the correction of a committed case: log(N q) of item_counts(V, seed) with N = max(C - 1, 1)"""
    return log_expected_count(item_counts(V, seed), max(C - 1, 1))


def restate(h, W, b, cand, kind, beta=1.0, corr=None, correct_target=False, gscale=None, G0=None, dtype=np.float64):
    """h [R, K], W [V, K] (rows row_off .. row_off + V of the table as the products see them), b [V], cand int [R, C], corr [V] or None.
    -> dict like candidate_loss_ref.restate's, with z [R, C] the corrected scores (s: the uncorrected ones; both 0 where absent)."""
    f = dtype
    h, W, b = np.asarray(h, f), np.asarray(W, f), np.asarray(b, f)
    cand = np.asarray(cand)
    beta = f(beta)
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
    corrected = np.zeros((R, C), bool)
    z = s
    if corr is not None:
        corrected = present & (~first | bool(correct_target))
        z = np.where(corrected, s - np.asarray(corr, f)[ids], s).astype(f)
    elif correct_target:
        raise ValueError('correct_target without corr')
    m = lse = x = None
    if kind == 'bce':
        x = np.where(first, -z, z)
        sp, sg = _softplus(x).astype(f), _sigmoid(x).astype(f)
        term = np.where(present, np.where(first, beta * sp, sp), f(0)).astype(f)
        g = np.where(present, np.where(first, -(beta * sg), sg), f(0)).astype(f)
    elif kind == 'softmax':
        zm = np.where(present, z, -np.inf)
        m = np.where(valid, zm.max(1), f(0)).astype(f)
        e = np.where(present, np.exp((z - m[:, None]).astype(f)), f(0)).astype(f)
        tot = np.zeros(R, f)
        for c in range(C):
            tot = tot + e[:, c]
        tot = np.where(valid, tot, f(1))
        lse = np.log(tot).astype(f)
        p = (e / tot[:, None]).astype(f)
        g = np.where(present, p - first, 0).astype(f)
        term = np.where(first & present, ((m - z[:, 0]) + lse)[:, None], f(0)).astype(f)
    elif kind == 'bpr':
        neg = present & ~first
        x = np.where(neg, z - z[:, :1], f(0)).astype(f)
        term = np.where(neg, _softplus(x), f(0)).astype(f)
        g = np.where(neg, _sigmoid(x), f(0)).astype(f)
        tot = np.zeros(R, f)
        for c in range(1, C):
            tot = tot + g[:, c]
        g[:, 0] = f(0) - tot
    else:
        raise ValueError(kind)
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
    return dict(present=present, valid=valid, ids=ids, s=s, z=z, x=x, corrected=corrected, term=term, item=item, g=g, loss=loss, gs=gs,
                dh=dh, dW=dW, db=db, m=m, lse=lse, beta=float(beta))


def bounds(h, W, b, ref, kind, G0=None, bf16=False):
    """the derived bound (module docstring) of every output of restate(..., dtype=float64) = ref -> dict like ref's"""
    h, W, b = np.asarray(h, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    present, ids, s, z, g, gs, beta = ref['present'], ref['ids'], ref['s'], ref['z'], ref['g'], float(ref['gs']), ref['beta']
    R, K = h.shape
    V = W.shape[0]
    C = present.shape[1]
    first = np.zeros((R, C), bool)
    first[:, 0] = True
    Wa = np.abs(W)[ids] * present[:, :, None]              # [R, C, K], 0 where absent
    ha = np.abs(h)
    ds = gamma(K + 1) * (np.einsum('rk,rck->rc', ha, Wa) + np.abs(b)[ids]) * present
    dz = ds + U_F32 * np.abs(z) * ref['corrected']
    term = np.abs(ref['term'])
    if kind == 'bce':
        w = np.where(first, beta, 1.0)
        d_item = (w * dz).sum(1) + gamma(C + 8) * term.sum(1)
        dg = (w * dz / 4 + 8 * U_F32 * np.abs(g)) * present
    elif kind == 'softmax':
        dmax = dz.max(1)
        m, lse = ref['m'], ref['lse']
        d_item = (2 * dmax + 8 * U_F32 * (np.abs(m - z[:, 0]) + np.abs(lse) + np.abs(ref['item']))) * ref['valid']
        p = g + (np.arange(C) == 0)[None, :]
        dg = (2 * dmax[:, None] + U_F32 * p * (np.abs(z - m[:, None]) + 8) + 8 * U_F32 * np.abs(g)) * present
        if C == 1:                                         # the definition: exactly 0
            d_item, dg = d_item * 0, dg * 0
    else:
        neg = present & ~first
        dx = (dz + dz[:, :1] + U_F32 * np.abs(ref['x'])) * neg
        d_item = dx.sum(1) + gamma(C + 8) * term.sum(1)
        dg = (dx / 4 + 8 * U_F32 * np.abs(g)) * neg
        dg[:, 0] = dg.sum(1) + gamma(C) * (np.abs(g) * neg).sum(1)
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
    return dict(s=ds, z=dz, item=d_item, g=dg, loss=d_loss, dh=d_dh, dW=d_dW, db=d_db)


def measured_ratio(cases=None, settings=None):
    """worst |float32 mode - float64| / derived bound over the committed cases and settings (CPU only)"""
    worst = 0.0
    for R, C, K, V, scale in (cases or CASES):
        corr = corr_for(C, V)
        for bf16 in (False, True):
            for off in ROW_OFFS:
                h, table, b, cand = inputs(R, C, K, V, scale, bf16)
                W = operand_rows(table, off, V, bf16)
                for kind, beta, with_corr, target in (settings or SETTINGS):
                    kw = dict(beta=beta, corr=corr if with_corr else None, correct_target=target)
                    r64 = restate(h, W, b, cand, kind, **kw)
                    r32 = restate(h, W, b, cand, kind, dtype=np.float32, **kw)
                    bd = bounds(h, W, b, r64, kind)
                    for name in ('item', 'g', 'dh', 'dW', 'db'):
                        err = np.abs(np.asarray(r32[name], np.float64) - r64[name])
                        pos = bd[name] > 0
                        assert not err[~pos].any(), (name, 'not exact where the bound is 0')
                        if pos.any():
                            worst = max(worst, float((err[pos] / bd[name][pos]).max()))
    return worst
