"""Element-wise, derived error bounds for the bf16 / fp32 attention kernels and the logits-free vocabulary head.

Every kernel output X checked here is a contraction of factors of which some were rounded.  From the same inputs this module
computes, in float64,

    X_ref    the reference, and
    A_X      its absolute companion: the same formula with every factor replaced by its absolute value and every
             subtraction by an addition,

and bounds each ELEMENT on its own (no tensor-wide scale anywhere):

    |X_gpu - X_ref| <= (1 + 2^-6) * ( n u A_X  +  u_out |X_ref|  +  fp32 term )  +  2^-109 (underflow; only where the rest is > 0)

u = 2^-8 for bf16, 2^-24 for fp32: the unit roundoff of round-to-nearest with p significand bits is 2^-p (half the spacing
2^(1-p) of the numbers just above a power of two), and bf16 has 8 (7 stored and the hidden one): x = 1 + 2^-8 - 2^-12 rounds to
1, a relative error of 0.94 * 2^-8.  (2^-9 is the AVERAGE size of such a rounding, not its bound: with it the kernels' own
rounding steps, emulated on the CPU, leave the bound by up to 1.5 x on the six-live-key sequences, where one rounding is not
averaged with others; tests/test_local_bounds_cpu.py pins both facts.)  n counts the bf16 roundings on the output's path
inside the kernel (table below, read from the kernel source); u_out |X_ref| is the rounding of the stored output; the fp32
term carries (a) the fp32 accumulation, length * 2^-24 * A_X, and (b) the fp32 error of the exponent of every probability:
p = exp(s - lse) with s an fp32 dot product of `depth` exact bf16 products, so |delta p| / p <= |delta s| + |delta lse| <=
E[q, k] = 2^-24 (depth + 8) (sum_j |q_j||k_j| / sqrt(dh) + max_k' sum_j |q_j||k'_j| / sqrt(dh) + 1 + log S)   (the "+ 8" covers
the scale, the log2(e) product and the 1-ulp hardware exp / log), which enters the companions as a per-(q, k) weight beside
n u.  The factor 1 + 2^-6 covers the second-order products of these first-order terms (n u <= 2^-7 each).

Where the bound of an element is exactly 0 (padded keys' dK / dV, ignored rows, sequences without dO), the comparison demands an
exact 0.

Roundings per output and route (file:line of the instruction that rounds; "out" = rounding of the stored output)

  route        kernels                                   output  n   where
  -----------  ----------------------------------------  ------  --  -----------------------------------------------------------
  mfma         attn_fwd_mfma_kernel                      o       1   P -> bf16 in front of P V: attn_mfma.hip:212 pack8(pv); out :240
               (dense + packed, bf16, dh 32 / 64)        lse     0   logits are fp32 sums of exact bf16 products, the scale is
                                                                     applied in fp32 (attn_mfma.hip:174); stored fp32 (:250)
               attn_bwd_resident_kernel (S <= 256)       dv      1   P -> bf16: attn_mfma.hip:670 (key blocks: :405); out :717 (:462)
               attn_bwd_mfma_kernel (key blocks, S>256)  dq, dk  1   dS -> bf16: attn_mfma.hip:666 / :671 (key blocks: :401 / :406);
                                                                     out: dq :694 (key blocks :444, once, after the fp32 sum of the
                                                                     block partials), dk :716 (:461)
                                                         delta   -   delta = sum dO o reads the FORWARD's stored bf16 o
                                                                     (attn_mfma.hip:320-322 / :575): it carries o's whole bound
                                                                     (n = 1 and out), |delta delta_q| <= sum_j |dO_qj| bound_o[q, j]
  mq_mfma      attn_mq_fwd_mfma_kernel                   o       1   attn_mq.hip:475 pack8(pv); out :495
               attn_mq_bwd_mfma_kernel                   lse     0   as above
               (bf16, dh 32 / 64)                        dv      1   P -> bf16 attn_mq.hip:664; out :706, once per pass of 32 queries
                                                         dq, dk  1   dS -> bf16 attn_mq.hip:654 / :665; out: dq :722, dk :705 once
                                                                     per pass of 32 queries (a pass reads the stored bf16 row back
                                                                     and adds: ceil(queries / 32) - 1 further roundings of a partial
                                                                     sum, each bounded by u A)
  row_f32      attn.hip / attn_mq.hip fp32 kernels       all     0   plain fp32 VALU arithmetic, fp32 outputs (u_out = 2^-24)

  vce          vce_token_kernel<K,1> / <K,2> + combine   dh      1   P' -> bf16 in front of U = P' W: vocab_ce.hip:338 pack8(p);
                                                                     out :507
               vce_dw_kernel (atomic, deterministic,     dW      1   dlogit -> bf16 in front of h^T dlogit: vocab_ce.hip:667; the label
               foreground and background sweeps) + the               term -yd h_row is added in fp32; fp32 output
               label kernels                             db      0   column sums of the UNROUNDED fp32 dlogit (vocab_ce.hip:651 / :662)
               vce_lse_kernel / rowscal[:, 0]            lse     0   fp32 sums of exact bf16 products

The attention companions (c = 1 / sqrt(dh), w = n u + E + length 2^-24):
    o      A = sum_k P |V|                    (+ |o| sum_k P (E + S 2^-24) for the normaliser l, which sums the unrounded P)
    lse    |delta lse| <= max_k |delta s|     = 2^-24 (dh + 8) (max_k sum_j |q_j||k_j| c + 1 + log S) + 2^-24 (S + 8) + 2^-24 |lse|
    dV     A = sum_q P |dO|
    dS     |delta dS| <= |dS| (n u + 2 E) + P T 2 (dh + 8) 2^-24 + P delta_delta,   T[q, k] = sum_j |dO_qj||V_kj| + sum_j |dO_qj||O_qj|
           (|dS| = P |dP - delta| <= P T: the rounding of dS and the error of P are relative to dS itself, which is tighter than P T)
    dQ     bound = c sum_k |delta dS| |K| + fp32 sum over A = c sum_k P T |K|,   dK: the transpose form with |Q|
The vocabulary-head companions, with D = |dlogit_ref| + grad_scale onehot(label) on valid rows (the p_y - 1 cancellation:
p_y went through the rounding, the 1 did not):
    dh     A = D |W|,   dW: A = |h|^T D,   db: A = sum_r D
TF clip variant: a row that leaves [1e-7, 1 - 1e-7] gets U and Ud (the part outside the range) from two sweeps with two
roundings of the same p, so D gains 2 gs p / S on the entries outside the range; and the row's coefficients gs (1 / S - G) and
-gs G, G = Pu / S - yd, are fp32 differences of O(1) numbers (vocab_ce.hip:498, :513): D gains 8 * 2^-24 gs p on every entry of
such a row (on a confidently wrong row the exact coefficient gs Pc / S is smaller than that error: the MI355X run showed the
dominant entries' dW off by their own size, 3e-10 against gradients of 1e-3, until this term was counted).  The kernels decide the clipping on fp32
probabilities: an entry with |log(p_ref / 1e-7)| <= E[r, v] (E as above with depth K and the logits' sum_j |h_j||w_j| + |b|),
or a row whose mass beside its dominant entry is within the row's largest E (+ V 2^-24) of 1e-7, is UNDECIDED; it is not
excluded: its full contribution gs p / S (a whole undecided row: |dlogit| + gs p / S) is added to the bound of the dh row and
the dW / db column it feeds.  `slack_share` reports which fraction of the checked elements received such slack; the tests
assert < 5 % on the reference before any GPU comparison.
"""
import math

import numpy as np
import torch

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -6
EPS_TF = 1e-7
SLACK_CAP = 0.05
# roundings behind a clipped row's coefficients: Pu = 1 - Pc, S = Pu + ..., invS = 1 / S, Pu * invS, - yd, gs *, gs *, ra - rb
COEF_ULPS = 8
# fp32 (and bf16: same exponent range) flush what falls under the smallest normal number 2^-126: up to 2^13 such terms times factors
# of at most 2^4 can be missing from a sum.  Added to every POSITIVE bound (a bound of 0 stays an exact-zero demand).
UNDERFLOW = 2.0 ** -109


def _finish(b):
    return torch.where(b > 0, b * SECOND_ORDER + UNDERFLOW, torch.zeros_like(b))

# n per output and route: the table of the module docstring
ROUTES = {
    'mfma': dict(u=U_BF16, u_out=U_BF16, n_o=1, n_lse=0, n_dv=1, n_ds=1, pass_rows=0),
    'mq_mfma': dict(u=U_BF16, u_out=U_BF16, n_o=1, n_lse=0, n_dv=1, n_ds=1, pass_rows=32),
    'row_f32': dict(u=U_F32, u_out=U_F32, n_o=0, n_lse=0, n_dv=0, n_ds=0, pass_rows=0),
}
VCE = dict(u=U_BF16, n_dh=1, n_dw=1, n_db=0, n_lse=0)


def bf16r(x):
    """round to bf16 and back (the kernels' (bf16_t) conversions), any float dtype"""
    return x.to(torch.bfloat16).to(x.dtype)


# ------------------------------------------------------------------------------------------------------------------
# the comparator
# ------------------------------------------------------------------------------------------------------------------
def violations(got, ref, bound):
    got, ref, bound = [torch.as_tensor(t).detach().double().cpu() for t in (got, ref, bound)]
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    return (got - ref).abs() > bound


def worst_ratio(got, ref, bound):
    """max |error| / bound over the elements with a positive bound (0.0 if there is none)"""
    got, ref, bound = [torch.as_tensor(t).detach().double().cpu() for t in (got, ref, bound)]
    pos = bound > 0
    if not bool(pos.any()):
        return 0.0
    return float(((got - ref).abs()[pos] / bound[pos]).max())


def accepts(got, ref, bound):
    return not bool(violations(got, ref, bound).any())


def check(name, got, ref, bound, record=None):
    """Assert |got - ref| <= bound for every element (an element with bound 0 must be exact); returns the worst ratio."""
    got64 = torch.as_tensor(got).detach().double().cpu()
    ref, bound = torch.as_tensor(ref).double(), torch.as_tensor(bound).double()
    assert bool(torch.isfinite(got64).all()), '%s: non-finite values' % name
    bad = violations(got64, ref, bound)
    ratio = worst_ratio(got64, ref, bound)
    if record is not None:
        record[name] = max(record.get(name, 0.0), ratio)
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError('%s: %d of %d elements outside their bound, worst |err| / bound = %.3g; first at %s: got %.6g, ref %.6g, '
                             'bound %.3g' % (name, int(bad.sum()), bad.numel(), ratio, idx, float(got64[idx]), float(ref[idx]),
                                             float(bound[idx])))
    return ratio


# ------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------
def _attn_item(q, k, v, do, live, r, dh):
    """N (sequence, head) items of one shape: q, do [N, M, dh]; k, v [N, S, dh]; live [N, S] bool.
    -> {name: (ref, bound)} for o, dq [N, M, dh], lse [N, M], dk, dv [N, S, dh]."""
    M, S = q.shape[1], k.shape[1]
    u, uo, e32 = r['u'], r['u_out'], U_F32
    c = 1.0 / float(np.sqrt(np.float32(dh)))
    t = lambda x: x.transpose(-1, -2)      # noqa: E731
    lv = live.double()[:, None, :]
    s = (q @ t(k)) * c + (1.0 - lv) * -1e9
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    o = P @ v
    qa, ka, va, ga = q.abs(), k.abs(), v.abs(), do.abs()
    sabs = (qa @ t(ka)) * c
    smax = (sabs * lv).max(-1).values                  # over the live keys (the others' p is an exact 0)
    logS = 1.0 + math.log(max(S, 2))
    E = e32 * (dh + 8) * (sabs + smax[..., None] + logS)
    b_lse = r['n_lse'] * u * smax + e32 * (dh + 8) * (smax + logS) + e32 * (S + 8) + e32 * lse.abs()
    wl = E + e32 * (S + 8)
    b_o = (P * (r['n_o'] * u + wl)) @ va + o.abs() * (P * wl).sum(-1, keepdim=True) + uo * o.abs()
    # backward: P from the forward's lse (its error and the logit's own: 2 E); delta from the forward's stored o
    dP = do @ t(v)
    delta = (do * o).sum(-1)
    dS = P * (dP - delta[..., None])
    dq, dk, dv = (dS @ k) * c, (t(dS) @ q) * c, t(P) @ do
    T2 = (ga * o.abs()).sum(-1)
    T = ga @ t(va) + T2[..., None]
    d_delta = (ga * b_o).sum(-1) + e32 * (dh + 8) * T2
    PT = P * T
    # the rounding of dS and the error of P are relative to dS itself (|dS| <= P T); T is needed for the fp32 sums behind dP only
    b_dS = dS.abs() * (r['n_ds'] * u + 2 * E) + PT * (e32 * 2 * (dh + 8)) + P * d_delta[..., None]
    passes = max(1, -(-M // r['pass_rows'])) if r['pass_rows'] else 1       # stored-row read-modify-write passes (dk / dv)
    A_dk, A_dv = (t(PT) @ qa) * c, t(P) @ ga
    b_dq = (b_dS @ ka) * c + e32 * (S + 8) * (PT @ ka) * c + uo * dq.abs()
    b_dk = (t(b_dS) @ qa) * c + e32 * (M + 8) * A_dk + uo * dk.abs() + (passes - 1) * uo * A_dk
    b_dv = t(P * (r['n_dv'] * u + 2 * E + e32 * (M + 8))) @ ga + uo * dv.abs() + (passes - 1) * uo * A_dv
    out = {'o': (o, b_o), 'lse': (lse, b_lse), 'dq': (dq, b_dq), 'dk': (dk, b_dk), 'dv': (dv, b_dv)}
    return {n: (a, _finish(b)) for n, (a, b) in out.items()}


def attn_batch(q, k, v, do, items, live, H, dh, route):
    """q, do [Rq, H*dh]; k, v [T, H*dh] (float64, the values the kernel reads); items: (q0, q1, t0, t1) per sequence; live [T] bool.
    -> {name: (ref, bound)}: o, dq [Rq, H*dh]; lse [Rq, H]; dk, dv [T, H*dh].  Rows outside every item: ref 0, bound 0."""
    r = ROUTES[route]
    q, k, v, do = [torch.as_tensor(t).detach().double().cpu() for t in (q, k, v, do)]
    live = torch.as_tensor(live).bool().cpu()
    Rq, T, d = q.shape[0], k.shape[0], H * dh
    shapes = {'o': (Rq, d), 'lse': (Rq, H), 'dq': (Rq, d), 'dk': (T, d), 'dv': (T, d)}
    res = {n: (torch.zeros(sh, dtype=torch.float64), torch.zeros(sh, dtype=torch.float64)) for n, sh in shapes.items()}
    groups = {}                                              # sequences of one shape go through the formulas together
    for it in items:
        if it[1] > it[0] and it[3] > it[2]:
            groups.setdefault((it[1] - it[0], it[3] - it[2]), []).append(it)
    heads = lambda x, a, b: x[a:b].reshape(b - a, H, dh).permute(1, 0, 2)      # noqa: E731  -> [H, rows, dh]
    for (M, S), its in groups.items():
        qq, gg = [torch.cat([heads(x, a, b) for a, b, _, _ in its]) for x in (q, do)]
        kk, vv = [torch.cat([heads(x, a, b) for _, _, a, b in its]) for x in (k, v)]
        lv = torch.cat([live[a:b][None, :].expand(H, -1) for _, _, a, b in its])
        got = _attn_item(qq, kk, vv, gg, lv, r, dh)
        for i, (q0, q1, t0, t1) in enumerate(its):
            for n, (a, b) in got.items():
                rows = slice(q0, q1) if n in ('o', 'lse', 'dq') else slice(t0, t1)
                for j, x in enumerate((a, b)):
                    blk = x[i * H:(i + 1) * H]
                    res[n][j][rows] = blk.T if n == 'lse' else blk.permute(1, 0, 2).reshape(-1, d)
    return res


def attn_dense(qkv, pad, do, B, S, H, dh, route):
    """The dense layout of ops.attn_fwd / attn_bwd: qkv [B*S, 3 H dh], pad [B, S] (1 = padded key).  lse comes back as [B, H, S]."""
    d = H * dh
    qkv = torch.as_tensor(qkv).detach().double().cpu()
    items = [(b * S, (b + 1) * S, b * S, (b + 1) * S) for b in range(B)]
    res = attn_batch(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], do, items, ~torch.as_tensor(pad).bool().reshape(-1).cpu(), H, dh, route)
    res['lse'] = tuple(t.reshape(B, S, H).permute(0, 2, 1).contiguous() for t in res['lse'])
    return res


def attn_packed(qkv, cu, do, H, dh, route, key_pad=None):
    """The packed layout (cu [B+1] row offsets).  lse stays [T, H]: the kernel's lse[b, h, :len_b] is row cu[b] + i of it."""
    d = H * dh
    qkv = torch.as_tensor(qkv).detach().double().cpu()
    cu = [int(c) for c in cu]
    items = [(cu[b], cu[b + 1], cu[b], cu[b + 1]) for b in range(len(cu) - 1)]
    live = torch.ones(qkv.shape[0], dtype=torch.bool) if key_pad is None else ~torch.as_tensor(key_pad).bool().cpu()
    return attn_batch(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], do, items, live, H, dh, route)


def packed_lse(lse_bhs, cu):
    """the kernel's lse [B, H, S_max] -> [T, H] rows in packed order"""
    cu = [int(c) for c in cu]
    return torch.cat([lse_bhs[b, :, :cu[b + 1] - cu[b]].T for b in range(len(cu) - 1)], 0)


def attn_mq(q, kv, cu, moff, do, H, dh, route, key_pad=None):
    """The masked-query kernels: q, do [R, H dh]; kv [T, 2 H dh]; sequence b: token rows cu[b]..cu[b+1], query rows moff[b]..moff[b+1]."""
    d = H * dh
    kv = torch.as_tensor(kv).detach().double().cpu()
    cu, moff = [int(c) for c in cu], [int(m) for m in moff]
    items = [(moff[b], moff[b + 1], cu[b], cu[b + 1]) for b in range(len(cu) - 1)]
    live = torch.ones(kv.shape[0], dtype=torch.bool) if key_pad is None else ~torch.as_tensor(key_pad).bool().cpu()
    return attn_batch(q, kv[:, :d], kv[:, d:], do, items, live, H, dh, route)


def attn_emulate(q, k, v, do, items, live, H, dh, route):
    """The kernels' arithmetic restated with their rounding steps (table above): fp32 sums, P / dS / o / the outputs rounded where the
    route rounds them.  What `check` must accept without a GPU."""
    r = ROUTES[route]
    rnd = bf16r if r['u'] == U_BF16 else (lambda t: t)
    q, k, v, do = [torch.as_tensor(t).detach().float().cpu() for t in (q, k, v, do)]
    live = torch.as_tensor(live).bool().cpu()
    Rq, T, d = q.shape[0], k.shape[0], H * dh
    out = {'o': torch.zeros(Rq, d), 'lse': torch.zeros(Rq, H), 'dq': torch.zeros(Rq, d), 'dk': torch.zeros(T, d), 'dv': torch.zeros(T, d)}
    c = float(np.float32(1.0) / np.sqrt(np.float32(dh)))
    for q0, q1, t0, t1 in items:
        if q1 <= q0 or t1 <= t0:
            continue
        for h in range(H):
            cs = slice(h * dh, (h + 1) * dh)
            qq, kk, vv, gg, lv = q[q0:q1, cs], k[t0:t1, cs], v[t0:t1, cs], do[q0:q1, cs], live[t0:t1]
            s = (qq @ kk.T) * c + (~lv).float()[None, :] * -1e9
            m = s.max(1, keepdim=True).values
            p = torch.exp(s - m)
            l = p.sum(1, keepdim=True)
            o = rnd((rnd(p) @ vv) / l)
            lse = (m + torch.log(l))[:, 0]
            P = torch.exp(s - lse[:, None])
            delta = (gg * o).sum(1, keepdim=True)
            dS = P * (gg @ vv.T - delta)
            out['o'][q0:q1, cs], out['lse'][q0:q1, h] = o, lse
            out['dq'][q0:q1, cs] = rnd((rnd(dS) @ kk) * c)
            step = r['pass_rows'] or (q1 - q0)
            dk, dv = torch.zeros_like(kk), torch.zeros_like(vv)
            for a in range(0, q1 - q0, step):                      # a pass adds to the stored (rounded) rows
                dk = rnd(dk + (rnd(dS[a:a + step]).T @ qq[a:a + step]) * c)
                dv = rnd(dv + rnd(P[a:a + step]).T @ gg[a:a + step])
            out['dk'][t0:t1, cs], out['dv'][t0:t1, cs] = dk, dv
    return out


# ------------------------------------------------------------------------------------------------------------------
# vocabulary head
# ------------------------------------------------------------------------------------------------------------------
def vocab_ref(h, W, b, y, variant):
    """float64 reference of the logits-free head (softmax -> TF's clipped sparse CE / plain CE, mean over the valid rows) with the
    gradient of the logits retained, and the element-wise bounds of dh [R, K], dW [K, V], db [V] and lse [R].
    h [R, K], W [V, K], b [V]: the values the kernels read; y [R] (< 0: ignored)."""
    ht = torch.tensor(np.asarray(h), dtype=torch.float64, requires_grad=True)
    Wt = torch.tensor(np.asarray(W), dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(np.asarray(b), dtype=torch.float64, requires_grad=True)
    y = np.asarray(y)
    R, K = ht.shape
    V = Wt.shape[0]
    valid = torch.tensor(y >= 0)
    yl = torch.tensor(np.where(y >= 0, y, 0).astype(np.int64))
    logits = ht @ Wt.T + bt
    logits.retain_grad()
    if variant == 'tf':
        lg = torch.log(torch.clamp(torch.softmax(logits, -1), EPS_TF, 1.0 - EPS_TF))
        item = torch.logsumexp(lg, -1) - lg.gather(1, yl[:, None])[:, 0]
    else:
        item = -torch.log_softmax(logits, -1).gather(1, yl[:, None])[:, 0]
    item = item * valid.double()
    gs = 1.0 / max(int(valid.sum()), 1)
    (item.sum() * gs).backward()
    with torch.no_grad():
        dlogit = logits.grad
        lse = torch.logsumexp(logits, -1)
        p = torch.softmax(logits, -1)
        onehot = torch.zeros(R, V, dtype=torch.float64)
        onehot[torch.arange(R), yl] = 1.0
        onehot *= valid.double()[:, None]
        habs, Wabs = ht.abs(), Wt.abs()
        xabs = habs @ Wabs.T + bt.abs()[None, :]
        xm = xabs.max(1).values
        logV = 1.0 + math.log(max(V, 2))
        E = U_F32 * (K + 8) * (xabs + xm[:, None] + logV)
        D = dlogit.abs() + gs * onehot
        slack = torch.zeros(R, V, dtype=torch.float64)
        coef = torch.zeros(R, V, dtype=torch.float64)
        if variant == 'tf':
            outside = (p < EPS_TF) | (p > 1.0 - EPS_TF)
            clipped = outside.any(1) & valid
            S = torch.clamp(p, EPS_TF, 1.0 - EPS_TF).sum(1)
            unit = gs * p / S[:, None]                                     # an entry's contribution when it counts as inside
            D = D + (outside & clipped[:, None]).double() * 2.0 * unit
            # the row's two coefficients (inside the range: gs (1 / S - G), outside: -gs G, G = Pu / S - yd) are fp32 DIFFERENCES of
            # O(1) numbers (vocab_ce.hip:498 G = Pu * invS - yd, :513 ra - rb): an absolute error of up to COEF_ULPS 2^-24 gs each, whatever
            # is left of them after the cancellation (a confidently wrong row: gs Pc / S with Pc the mass beside its dominant entry)
            coef = clipped[:, None].double() * (COEF_ULPS * U_F32 * gs) * p            # absolute: not scaled by n u
            und = (torch.log(p.clamp_min(1e-300) / EPS_TF).abs() <= E) & valid[:, None]
            slack = und.double() * unit
            pmax = p.max(1)
            rest = p.clone()
            rest[torch.arange(R), pmax.indices] = 0.0
            others = rest.sum(1).clamp_min(1e-300)                          # the mass beside the row's largest entry
            row_und = (torch.log(others / EPS_TF).abs() <= E.max(1).values + U_F32 * (V + 8)) & valid & (pmax.values > 0.5)
            slack = torch.where(row_und[:, None], dlogit.abs() + unit, slack)
        u = VCE['u']
        dh, dW, db = ht.grad, Wt.grad.T.contiguous(), bt.grad
        has = slack > 0
        slack = slack + coef
        b_dh = (D * (VCE['n_dh'] * u + E + U_F32 * (V + 8)) + slack) @ Wabs + u * dh.abs()
        b_dW = habs.T @ (D * (VCE['n_dw'] * u + E + U_F32 * (R + 8)) + slack) + U_F32 * dW.abs()
        b_db = (D * (VCE['n_db'] * u + E + U_F32 * (R + 8)) + slack).sum(0) + U_F32 * db.abs()
        b_lse = U_F32 * (K + 8) * (xm + logV) + U_F32 * (V + 8) + U_F32 * lse.abs()
        share = {'dh': float(has.any(1).double().mean()), 'dW': float(has.any(0).double().mean()), 'db': float(has.any(0).double().mean())}
    return {'item': item.detach(), 'loss': float(item.detach().sum()) * gs, 'gs': gs, 'dlogit': dlogit, 'p': p, 'lse': (lse, _finish(b_lse)),
            'dh': (dh, _finish(b_dh)), 'dW': (dW, _finish(b_dW)), 'db': (db, _finish(b_db)), 'slack_share': share,
            'onehot': onehot}


def vocab_emulate(h, W, b, y, variant, ref):
    """The head's arithmetic with its rounding steps: bf16 P in front of P W, bf16 dlogit in front of h^T dlogit (the label term added
    in fp32), db from the unrounded dlogit, dh stored in bf16; fp32 sums."""
    ht, Wt = torch.tensor(np.asarray(h)).float(), torch.tensor(np.asarray(W)).float()
    p, dlogit, onehot, gs = ref['p'], ref['dlogit'], ref['onehot'], ref['gs']
    # dlogit = p coef - gs yd onehot: the sweeps see p coef, the label kernels the rest
    yd = onehot * ((dlogit.abs().sum(1, keepdim=True) > 0) & ((p >= EPS_TF) | (variant != 'tf'))).double()
    sweep = (dlogit + gs * yd).float()                # fp32 dlogit without the label term
    coef = torch.where(p > 0, sweep.double() / p.clamp_min(1e-300), torch.zeros_like(p))
    dh = bf16r(((bf16r(p.float()).double() * coef).float() @ Wt) - (gs * yd).float() @ Wt)
    dW = ht.T @ bf16r(sweep) - ht.T @ (gs * yd).float()
    db = sweep.sum(0) - (gs * yd).float().sum(0)
    return {'dh': dh, 'dW': dW, 'db': db}


def edge_report(ref, V, R):
    """max |reference gradient| of each named kernel edge over the median of its peers (the condition of the edge cases: >= 0.1).
    Edges: last vocabulary column, last 128-column tile, columns 127 and 128, last token row, last 128-row token tile."""
    dW, db, dh = ref['dW'][0].abs(), ref['db'][0].abs(), ref['dh'][0].abs()
    colw, colb = dW.max(0).values, db                         # per vocabulary column
    rowh = dh.max(1).values                                   # per token row
    rep = {}

    def rel(vals, idx, name):
        idx = [i for i in idx if 0 <= i < len(vals)]
        peers = np.setdiff1d(np.arange(len(vals)), idx)
        if not idx or len(peers) == 0:
            return
        med = float(np.median(vals[peers]))
        rep[name] = float(vals[idx].min()) / med if med > 0 else float('inf')

    def tiles(vals):
        n = (len(vals) + 127) // 128
        return np.array([float(vals[t * 128:(t + 1) * 128].max()) for t in range(n)])
    cw, cb, rh = colw.numpy(), colb.numpy(), rowh.numpy()
    for tag, vals in (('dW', cw), ('db', cb)):
        rel(vals, [V - 1], tag + ' last column')
        rel(vals, [127], tag + ' column 127')
        rel(vals, [128], tag + ' column 128')
        t = tiles(vals)
        rel(t, [len(t) - 1], tag + ' last vocabulary tile')
    live = rh > 0                                             # ignored rows are exact zeros: no peers, and no edge to weigh
    if live[R - 1] and live[:R - 1].any():
        rep['dh last row'] = float(rh[R - 1]) / float(np.median(rh[:R - 1][live[:R - 1]]))
    t = tiles(rh)
    rel(t, [len(t) - 1], 'dh last token tile')
    return rep


# the metrics the suite used before this module (kept for the record: the CPU tests show what they let through)
def old_rel_max(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def old_rel_l2(got, ref, floor=0.0):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).norm() / max(float(ref.norm()), floor))


# ------------------------------------------------------------------------------------------------------------------
# the committed cases (shared by the CPU tests of this module and the GPU tests: same seeds, same inputs)
# ------------------------------------------------------------------------------------------------------------------
# dense layout: the grid of test_attention_fwd_bwd, then S = 64, 65, 128, 256, 384 and a B * H > 256 case at S = 72
DENSE_SHAPES = [(3, 13, 2, 32), (2, 200, 2, 64), (2, 70, 1, 16), (1, 300, 2, 128), (2, 256, 2, 64), (3, 32, 1, 64), (2, 33, 4, 32),
                (5, 53, 2, 32), (2, 129, 3, 64), (2, 512, 4, 64), (3, 257, 2, 64), (2, 300, 2, 32), (1, 481, 1, 64),
                (2, 64, 2, 64), (2, 65, 2, 32), (2, 128, 2, 64), (2, 256, 1, 32), (2, 384, 2, 64), (130, 72, 2, 64)]
PATTERNS = ['short', 'long']      # 'short': sequence 1 keeps about six live keys (the existing test's pattern); 'long': every one long


def dense_cases():
    """(dtype, B, S, H, dh, pattern); bf16 where the MFMA kernels run (dh 32 / 64), fp32 everywhere (the row kernels)"""
    out = []
    for B, S, H, dh in DENSE_SHAPES:
        for pat in PATTERNS:
            out.append((torch.float32, B, S, H, dh, pat))
            if dh in (32, 64):
                out.append((torch.bfloat16, B, S, H, dh, pat))
    return out


def dense_inputs(dtype, B, S, H, dh, pattern):
    """-> qkv [B*S, 3 H dh], pad [B, S] uint8, do [B*S, H dh]: fp32 tensors holding values of `dtype`"""
    g = torch.Generator().manual_seed(S + dh)
    d = H * dh
    qkv = (torch.randn(B * S, 3 * d, generator=g) * 0.8).to(dtype).float()
    pad = torch.zeros(B, S, dtype=torch.uint8)
    pad[0, S - 4:] = 1
    if pattern == 'short':
        if B > 1:
            pad[1, 5:S - 1] = 1
    else:
        for b in range(1, B):
            pad[b, S - (b % 3):] = 1 if b % 3 else 0
    do = torch.randn(B * S, d, generator=g).to(dtype).float()
    return qkv, pad, do


PACKED_CASES = [([200, 37, 1, 64, 129, 33, 2, 200], 2, 64), ([53, 8, 31, 32, 33], 2, 32), ([512, 40, 300, 257, 1, 256], 4, 64),
                ([224, 225, 100], 1, 64), ([1, 256, 257, 512], 2, 64)]


def packed_inputs(lens, H, dh):
    g = torch.Generator().manual_seed(sum(lens) + dh)
    d, T = H * dh, sum(lens)
    qkv = (torch.randn(T, 3 * d, generator=g) * 0.8).bfloat16().float()
    do = torch.randn(T, d, generator=g).bfloat16().float()
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    return qkv, cu, do


MQ_CASES = [(torch.float32, 2, 64, 50, 10, False), (torch.float32, 4, 32, 200, 20, True), (torch.float32, 2, 64, 300, 5, False),
            (torch.bfloat16, 2, 64, 200, 10, False), (torch.bfloat16, 4, 64, 512, 12, True), (torch.bfloat16, 2, 32, 70, 33, False),
            (torch.bfloat16, 1, 64, 3, 1, False), (torch.bfloat16, 2, 64, 33, 32, False), (torch.bfloat16, 2, 32, 64, 64, True),
            (torch.float32, 1, 32, 3, 1, False), (torch.bfloat16, 3, 64, 129, 7, False)]


def mq_inputs(dtype, H, dh, smax, mmax, pad, B=9):
    """the ragged batches of test_attn_mq_kernels_match_fp64 -> cu, moff, q, kv, do (tensors of `dtype`), key_pad or None"""
    g = torch.Generator().manual_seed(100 + smax + mmax)
    lens = torch.randint(3, smax + 1, (B,), generator=g)
    lens[0] = smax
    nq = torch.randint(0, mmax + 1, (B,), generator=g)
    nq[1 % B] = mmax
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    moff = torch.zeros(B + 1, dtype=torch.int32)
    moff[1:] = torch.cumsum(nq, 0)
    T, R, d = int(cu[-1]), int(moff[-1]), H * dh
    q = (torch.randn(R, d, generator=g) * 0.8).to(dtype)
    kv = (torch.randn(T, 2 * d, generator=g) * 0.8).to(dtype)
    go = torch.randn(R, d, generator=g).to(dtype)
    key_pad = None
    if pad:
        key_pad = (torch.rand(T, generator=torch.Generator().manual_seed(1)) < 0.15).to(torch.uint8)
        key_pad[cu[:-1].long()] = 0
    return cu, moff, q, kv, go, key_pad


# vocabulary head: (R, V, K, operand scale, ignored rows, variant, seed).  Split counts: V in {50, 129, 300, 640, 700, 1000, 1301};
# R = 5000 for tsplit > 1 in the dW sweep; the clip regime (scales 1.2 .. 2.0) with the seeds chosen so that the undecided share
# stays under 5 %
VOCAB_CASES = [
    (300, 1000, 128, 0.3, 0, 'tf', 1), (300, 1000, 128, 1.6, 5, 'tf', 1), (77, 50, 64, 0.5, 3, 'tf', 1), (130, 129, 64, 2.0, 0, 'tf', 1),
    (257, 700, 128, 1.2, 7, 'plain', 1), (1, 300, 128, 1.0, 0, 'tf', 1), (200, 640, 128, 0.8, 4, 'tf', 7), (300, 1301, 128, 0.3, 4, 'plain', 1),
    (400, 700, 64, 1.2, 7, 'tf', 1), (5000, 300, 128, 0.5, 9, 'tf', 1),
]


# edge cases (R, V, K, scale, variant, seed): V and R on, one below and one above the 128 tile edges; operand scale 0.3 (nothing
# clipped: every probability is O(1 / V), every row carries gradient), one TF case at 1.2.  Each runs in two forms (vocab_inputs(edge=...)):
# 'labels': rows 1..4 carry the labels 0, 127, 128, V - 1 and the last row V - 1; 'ignored': the same with rows 0, 127, 128, R - 1
# ignored.  The seeds were searched on the CPU for the condition of edge_report (every named edge >= 10 % of the median of its peers).
VOCAB_EDGE_CASES = [(257, 127, 128, 0.3, 'plain', 1), (129, 128, 64, 0.3, 'tf', 1), (128, 129, 128, 0.3, 'tf', 1), (127, 255, 64, 0.3, 'plain', 2),
                    (1, 257, 128, 0.3, 'tf', 1), (257, 257, 64, 0.3, 'tf', 1), (129, 129, 128, 0.3, 'plain', 1), (257, 257, 64, 1.2, 'tf', 1)]
EDGE_FORMS = ['labels', 'ignored']
EDGE_MIN = 0.1


def vocab_inputs(R, V, K, scale, n_ign, seed, edge=None):
    """bf16-representable h [R, K], W [V, K]; fp32 b [V]; labels y [R] (-1: ignored); edge: see VOCAB_EDGE_CASES.  At operand scales
    >= 1 the rows with a forced label point at it (logit about 6 above the rest: p_y about 0.5), so that the label's column carries a
    gradient of the order of grad_scale instead of a clipped nothing."""
    rng = np.random.default_rng(seed)
    h = (rng.standard_normal((R, K)) * scale).astype(np.float32)
    W = (rng.standard_normal((V, K)) * scale).astype(np.float32)
    b = (rng.standard_normal(V) * 0.5).astype(np.float32)
    y = rng.integers(0, V, size=R).astype(np.int32)
    if n_ign:
        y[rng.choice(R, n_ign, replace=False)] = -1
    if edge is not None:
        forced = {R - 1: V - 1}
        for r_, c in zip((1, 2, 3, 4), (0, 127, 128, V - 1)):
            if r_ < R - 1 and c < V:
                forced[r_] = c
        for r_, c in forced.items():
            y[r_] = c
            if scale >= 1.0:
                h[r_] = W[c] * (6.0 / float(np.dot(W[c], W[c])))
        if edge == 'ignored' and R > 1:
            for r_ in (0, 127, 128, R - 1):
                if r_ < R:
                    y[r_] = -1
    h = torch.from_numpy(h).bfloat16().float().numpy()
    W = torch.from_numpy(W).bfloat16().float().numpy()
    return h, W, b, y
