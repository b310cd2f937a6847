"""The in-batch contrastive loss of include/b4c.h restated in numpy from that header's comment, its derived fp32 error bounds, and
the committed cases of the GPU tests (shared with the CPU tests: same seeds, same inputs).

restate(...) evaluates the definition -- rnorm, scores, keys, lse, item_loss, the coefficients G, dz -- in float64, or
(dtype=np.float32) with EVERY intermediate rounded to float32: sequential sums, one rounding per operation.  The float32 mode is not
the kernel; it is a second, independent fp32 evaluation, and its distance from float64 measures what the derived bound leaves out.

Derived bound, per element, u = 2^-24, gamma_n = n u / (1 - n u) (the style of tests/candidate_loss_ref.py; bf16 operands are exact
in fp32 and so are their products, so only the fp32 sums round).  A_ij = sum_k |z_ik z_jk|, it = inv_temp, n_i = keys of row i,
nb = ceil(N / 32) + 2 (the rescalings of a running max-shifted sum that is carried block by block):
    rnorm   e_rn   = gamma_{K+4} relative (sum of squares, sqrt, max, reciprocal); 0 without the cosine flag
    score   ds_ij  = it rn_i rn_j gamma_{K+1} A_ij + |s_ij| (2 e_rn + 3 u)
    lse     dl_i   = max_{j key} ds_ij + gamma_{n_i + nb + 8} + u (R_i + 4) + 2 u (|m_i| + |lse_i|)     log-sum-exp is 1-Lipschitz in the
                     max norm; R_i = the spread of the row's key scores: an exponent's argument x is rounded before exp (u |x|)
                     n_i = 1: lse_i is the one score, dl_i = ds_{i, pos_i}
    item    di_i   = dl_i + ds_{i, pos_i} + u |item_i|;   n_i = 1: exactly 0
    P       dP_ij  = P_ij (ds_ij + dl_i + u (2 |s_ij - lse_i| + 4));   n_i = 1: exactly 0 (P = exp(0))
    G       dG_ij  = dP_ij + u |G_ij|
    coeff   dC_ij  = (dG_ij + dG_ji + u |W_ij|) rn_j + |C_ij| (e_rn + u)  [+ 2^-8 |C_ij|: bf16, the operand of the second product]
    dzh     dh_id  = gs it (sum_j dC_ij |z_jd| + gamma_{N+1} sum_j |C_ij z_jd|) + 3 u |dzh_id|
    dz      dot:   dd_i = sum_d (|zh_id| dh_id + e |zh_id dzh_id|) + gamma_{K+1} sum_d |zh_id dzh_id|,  e = e_rn + u
            cos:   rn_i (dh_id + |zh_id| dd_i + e |zh_id dot_i| + 2 u |zh_id dot_i| + u |dzh_id - zh_id dot_i|) + e |dz_id|
            dot:   dh_id                                                  [+ 2^-8 |dz_id|: the one bf16 rounding of the stored value]
An element whose bound is 0 (ignored rows; a batch where every live row's only key is its positive) must be exact.  The GATE of the
GPU tests is this bound times max(2, 2 x MEASURED_RATIO), MEASURED_RATIO = the worst |float32 mode - float64| / bound over the
committed cases, measured on the CPU (tests/test_nce_cpu.py::test_measured_ratio_is_current recomputes it)."""
import numpy as np

U_F32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
# worst |float32 mode - float64| in units of the derived bound over CASES x dtypes (measured on the CPU; see above)
MEASURED_RATIO = 0.127       # (case (6, 128, 0, deadpos, None, dot, 0.07): 0.1262; every other case below 0.09) -> the gate is 2 x the derived bound


def gamma(n):
    return n * U_F32 / (1.0 - n * U_F32)


def inv_temp(temperature):
    """the float the entry point receives"""
    return float(np.float32(1.0 / temperature))


def gate_factor():
    return max(2.0, 2.0 * MEASURED_RATIO)


def structure(pos, group, N):
    """-> live [N], p [N] (pos where live, else -1), ispos [N, N], key [N, N] of the definition"""
    pos = np.asarray(pos, np.int64)
    idx = np.arange(N)
    live = (pos >= 0) & (pos < N) & (pos != idx)
    p = np.where(live, pos, -1)
    g = np.full(N, -1, np.int64) if group is None else np.asarray(group, np.int64)
    gok = (g[:, None] < 0) | (g[None, :] < 0) | (g[:, None] != g[None, :])
    ispos = live[:, None] & (idx[None, :] == p[:, None])
    key = (idx[:, None] != idx[None, :]) & live[:, None] & (ispos | (live[None, :] & gok))
    return live, p, ispos, key


def restate(z, pos, group, inv_temp, cosine, gscale=None, dtype=np.float64):
    """z [N, K] (already rounded to the compute dtype), pos int [N], group int [N] or None -> dict: live, key, ispos, rn [N], s [N, N],
    m, lse, item [N], loss, gs, P, G, W, C [N, N], dzh, dz [N, K].  gscale None: 1 / max(#live rows, 1).  The bf16 rounding of the
    coefficient C is not applied: the bound carries it."""
    f = dtype
    z = np.asarray(z, f)
    N, K = z.shape
    idx = np.arange(N)
    live, p, ispos, key = structure(pos, group, N)
    it = f(inv_temp)
    if cosine:
        ss = np.zeros(N, f)
        for k in range(K):
            ss = ss + z[:, k] * z[:, k]
        rn = (f(1) / np.maximum(np.sqrt(ss).astype(f), f(1e-12))).astype(f)
    else:
        rn = np.ones(N, f)
    raw = np.zeros((N, N), f)
    for k in range(K):                                     # sequential: every partial sum is rounded to `dtype`
        raw = raw + z[:, k, None] * z[None, :, k]
    s = ((raw * (rn[:, None] * rn[None, :]).astype(f)).astype(f) * it).astype(f)
    sm = np.where(key, s, -np.inf)
    m = np.where(live, sm.max(1, initial=-np.inf), 0).astype(f)
    m = np.where(np.isfinite(m), m, 0).astype(f)
    e = np.where(key, np.exp((np.where(key, s, 0) - m[:, None]).astype(f)), f(0)).astype(f)
    tot = np.zeros(N, f)
    for j in range(N):
        tot = tot + e[:, j]
    tot = np.where(live, tot, f(1)).astype(f)
    lse = np.where(live, m + np.log(tot).astype(f), f(0)).astype(f)
    spos = s[idx, np.where(live, p, 0)]
    item = np.where(live, lse - spos, f(0)).astype(f)
    nlive = int(live.sum())
    gs = f(1.0 / max(nlive, 1) if gscale is None else gscale)
    loss = f(0)
    for i in range(N):
        loss = f(loss + item[i])
    loss = f(loss * gs)
    P = np.where(key, np.exp((np.where(key, s, 0) - lse[:, None]).astype(f)), f(0)).astype(f)
    G = (P - ispos.astype(f)).astype(f)
    W = (G + G.T).astype(f)
    C = (W * rn[None, :]).astype(f)
    acc = np.zeros((N, K), f)
    for j in range(N):
        acc = acc + C[:, j, None] * z[None, j, :]
    dzh = (acc * f(gs * it)).astype(f)
    if cosine:
        zh = (z * rn[:, None]).astype(f)
        dot = np.zeros(N, f)
        for k in range(K):
            dot = dot + zh[:, k] * dzh[:, k]
        dz = (rn[:, None] * (dzh - (zh * dot[:, None]).astype(f)).astype(f)).astype(f)
    else:
        zh, dot, dz = z, np.zeros(N, f), dzh
    return dict(live=live, key=key, ispos=ispos, p=p, rn=rn, s=s, m=m, lse=lse, item=item, loss=loss, gs=gs, P=P, G=G, W=W, C=C, dzh=dzh,
                zh=zh, dot=dot, dz=dz)


def bounds(z, ref, inv_temp, cosine, bf16=False):
    """the derived bound (module docstring) of lse, item, dz of restate(..., dtype=float64) = ref -> dict like ref's"""
    z = np.asarray(z, np.float64)
    N, K = z.shape
    u = U_F32
    it, gs = float(inv_temp), float(ref['gs'])
    live, key, p, rn, s = ref['live'], ref['key'], ref['p'], ref['rn'], ref['s']
    idx = np.arange(N)
    za = np.abs(z)
    A = za @ za.T
    e_rn = gamma(K + 4) if cosine else 0.0
    ds = it * rn[:, None] * rn[None, :] * gamma(K + 1) * A + np.abs(s) * (2 * e_rn + 3 * u)
    nk = key.sum(1)
    nb = (N + 31) // 32 + 2
    ds_pos = ds[idx, np.where(live, p, 0)] * live
    dmax = np.where(key, ds, 0).max(1, initial=0.0)
    smax = np.where(key, s, -np.inf).max(1, initial=-np.inf)
    smin = np.where(key, s, np.inf).min(1, initial=np.inf)
    spread = np.where(nk > 0, smax - smin, 0.0)
    d_lse = dmax + gamma(nk + nb + 8) + u * (spread + 4) + 2 * u * (np.abs(ref['m']) + np.abs(ref['lse']))
    d_lse = np.where(nk == 1, ds_pos, d_lse) * live
    d_item = np.where(nk == 1, 0.0, d_lse + ds_pos + u * np.abs(ref['item'])) * live
    P, G, W, C = ref['P'], ref['G'], ref['W'], ref['C']
    dP = P * (ds + d_lse[:, None] + u * (2 * np.abs(np.where(key, s - ref['lse'][:, None], 0)) + 4)) * key
    dP = np.where((nk == 1)[:, None], 0.0, dP)
    dG = dP + u * np.abs(G)
    e = e_rn + u
    dC = (dG + dG.T + u * np.abs(W)) * rn[None, :] + np.abs(C) * e
    if bf16:
        dC = dC + U_BF16 * np.abs(C)
    d_dzh = gs * it * (dC @ za + gamma(N + 1) * (np.abs(C) @ za)) + 3 * u * np.abs(ref['dzh'])
    if cosine:
        zh, dzh, dot = np.abs(ref['zh']), np.abs(ref['dzh']), np.abs(ref['dot'])
        d_dot = (zh * d_dzh + e * zh * dzh).sum(1) + gamma(K + 1) * (zh * dzh).sum(1)
        inner = np.abs(ref['dzh'] - ref['zh'] * ref['dot'][:, None])
        d_dz = rn[:, None] * (d_dzh + zh * d_dot[:, None] + (e + 2 * u) * zh * dot[:, None] + u * inner) + e * np.abs(ref['dz'])
    else:
        d_dz = d_dzh
    if bf16:
        d_dz = d_dz + U_BF16 * np.abs(ref['dz'])
    return dict(lse=d_lse, item=d_item, dz=d_dz)


def dense_loss(z, pos, group, inv_temp, cosine):
    """the definition as dense torch operations (autograd supplies the gradient) -> the mean item loss over the live rows"""
    import torch
    N = z.shape[0]
    live, p, ispos, key = structure(pos, group, N)
    zh = z / z.norm(dim=1, keepdim=True).clamp(min=1e-12) if cosine else z
    s = (zh @ zh.T) * inv_temp
    keyt = torch.from_numpy(key).to(z.device)
    livet = torch.from_numpy(live).to(z.device)
    lse = torch.logsumexp(torch.where(keyt, s, torch.full_like(s, -float('inf')))[livet], dim=1)
    spos = s[livet][torch.arange(int(live.sum()), device=z.device), torch.from_numpy(p[live]).to(z.device)]
    return (lse - spos).sum() / max(int(live.sum()), 1)


# ---- the committed cases ------------------------------------------------------------------------------------------------------
# (N, K, pitch - K, pos pattern, group kind, similarity, temperature).  N: one and several 128-row tiles on both sides with remainders
# (2, 6, 127 | 130, 258, 385), K: one 16-byte chunk, the two tile widths, and widths that are no multiple of a k-step (24, 72) or of
# a 32-column block (72, 120).  (2, ..) and (6, 64, .., 'same'): every live row's only key is its positive -- item_loss and dz exactly 0.
CASES = [
    (2, 8, 0, 'paired', None, 'dot', 1.0),
    (2, 64, 8, 'paired', None, 'cos', 0.07),
    (6, 8, 8, 'holes', 'neg', 'cos', 1.0),
    (6, 64, 0, 'paired', 'same', 'dot', 1.0),
    (6, 128, 0, 'deadpos', None, 'dot', 0.07),
    (127, 64, 0, 'cycle', 'repeat', 'cos', 0.07),
    (127, 128, 8, 'holes', None, 'dot', 1.0),
    (127, 120, 8, 'paired', 'neg', 'cos', 1.0),
    (130, 8, 0, 'paired', 'repeat', 'dot', 1.0),
    (130, 24, 8, 'cycle', None, 'dot', 0.07),
    (130, 128, 0, 'deadpos', 'neg', 'cos', 1.0),
    (258, 64, 8, 'paired', 'repeat', 'cos', 0.07),
    (258, 72, 0, 'holes', 'repeat', 'dot', 1.0),
    (258, 128, 0, 'cycle', 'neg', 'dot', 0.07),
    (385, 8, 0, 'holes', 'repeat', 'cos', 1.0),
    (385, 64, 0, 'deadpos', None, 'dot', 1.0),
    (385, 128, 16, 'paired', 'repeat', 'cos', 0.07),
]


def case_id(case):
    return '-'.join(str(x) for x in case)


def make_pos(N, pattern):
    """paired: the two halves name each other (an odd N: the last row names nobody); holes: paired with rows that name -1, N + 3 or
    themselves; cycle: a non-involutive map (i -> i + 7 mod N, i + 2 for N = 6, the swap for N = 2); deadpos: paired, but row 0
    names row 1 and row 1 names nobody: a positive that is not live (N > 200: one more, in another tile)."""
    h = N // 2
    pos = np.full(N, -1, np.int32)
    pos[:h] = np.arange(h) + h
    pos[h:2 * h] = np.arange(h)
    if pattern == 'paired':
        return pos
    if pattern == 'holes':
        pos[0] = -1
        if N > 4:
            pos[3] = N + 3
            pos[N - 2] = N - 2
            pos[N // 3] = -5
        return pos
    if pattern == 'cycle':
        step = 7 if N > 8 else (2 if N > 2 else 1)
        return ((np.arange(N) + step) % N).astype(np.int32)
    if pattern == 'deadpos':
        pos[0] = 1
        pos[1] = -1
        if N > 200:
            pos[N - 1] = 140          # a positive in another tile ...
            pos[140] = N + 1          # ... that is not live
        return pos
    raise ValueError(pattern)


def make_group(N, kind, seed):
    if kind is None:
        return None
    if kind == 'same':
        return np.full(N, 3, np.int32)
    rng = np.random.default_rng(77 + seed)
    g = (np.arange(N) % 37).astype(np.int32)               # row i and rows i + 37, i + 74, ..: repeats inside and across the 128-row tiles
    if N > 128:
        g[N - 1] = g[0]
        g[129] = g[5]
    if kind == 'neg':
        g[rng.random(N) < 0.3] = -1
        g[0] = -7
    return g


def inputs(case, bf16, seed=0):
    """-> z [N, ld] fp32 (bf16-representable when bf16; the columns behind K hold NaN: nobody may read them as data), pos, group"""
    N, K, pad, pattern, gkind, sim, temp = case
    rng = np.random.default_rng(1000 * N + K + seed)
    scale = 0.3 if sim == 'dot' else 1.0
    z = (rng.standard_normal((N, K)) * scale).astype(np.float32)
    if bf16:
        import torch
        z = torch.from_numpy(z).bfloat16().float().numpy()
    full = np.full((N, K + pad), np.nan, np.float32)
    full[:, :K] = z
    return full, make_pos(N, pattern), make_group(N, gkind, N + K)


def measured_ratio(cases=None):
    """worst |float32 mode - float64| / derived bound over the committed cases (CPU only; a few seconds)"""
    worst = 0.0
    for case in (cases or CASES):
        N, K, pad, pattern, gkind, sim, temp = case
        for bf16 in (False, True):
            zf, pos, group = inputs(case, bf16)
            z = zf[:, :K]
            it = inv_temp(temp)
            r64 = restate(z, pos, group, it, sim == 'cos')
            r32 = restate(z, pos, group, it, sim == 'cos', dtype=np.float32)
            bd = bounds(z, r64, it, sim == 'cos')
            for name in ('lse', 'item', 'dz'):
                err = np.abs(np.asarray(r32[name], np.float64) - r64[name])
                ok = bd[name] > 0
                assert not err[~ok].any(), (case, name, 'not exact where the bound is 0')
                if ok.any():
                    worst = max(worst, float((err[ok] / bd[name][ok]).max()))
    return worst
