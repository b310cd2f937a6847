"""Element-wise, derived error bounds of the pre-LN backward kernels (csrc/pre_ln.hip), in the manner of tests/local_bounds.py: the
float64 reference, its absolute companion (every factor replaced by its absolute value, every subtraction by an addition) and a
count of the kernel's own rounding steps.  u = 2^-24 for the fp32 arithmetic every route does, u_out = 2^-24 / 2^-8 for the
rounding of a stored fp32 / bf16 output (local_bounds.U_F32 / U_BF16).

b4c_layernorm_bwd_add (ln_bwd_rows.h: ln_bwd_rows with ResAddEpi): the inputs are read exactly (bf16 -> fp32 is exact); per element

    xhat = (x - mean) * rstd                 2 roundings
    a    = dout * gamma                      1
    s1   = sum_j a / d,  s2 = sum_j a xhat / d      fp32 sums of d terms in some order (8 per lane, then a butterfly): at most
                                             d - 1 roundings on any path, + 1 product (+ 2 of xhat) per term, + 1 for * (1 / d)
                                             and 1 for the rounded 1 / d itself
    o    = rstd * (a - s1 - xhat * s2)       4
    dx   = round_out(res + o)                1 in fp32 (or none: a fused multiply-add), 1 to the output type

so with A = rstd (|a| + mean_j |a| + |xhat| mean_j (|a| |xhat|)) every term of o carries at most (d + 12) roundings:

    |dx - ref| <= (1 + 2^-6) ((d + 12) u A + u (|res| + A) + u_out |ref|) + 2^-109

    dgamma[j] += sum_rows dout * xhat        3 roundings per term; the sum runs over the rows in a fixed order (per thread, then LDS
    dbeta[j]  += sum_rows dout               row groups, then 1024 workgroup partials, 64 lanes and a butterfly): whatever the
                                             order, at most rows - 1 roundings on a path; + 1 for the add into the sink
    |dgamma - ref| <= (1 + 2^-6) ((rows + 3) u G + u |ref|) + 2^-109,   G = |g0| + sum_rows |dout| |xhat|,   g0 = the sink before
    |dbeta - ref|  <= (1 + 2^-6) (rows u B + u |ref|) + 2^-109,         B = |b0| + sum_rows |dout|

b4c_gemm_nt_ln_bwd_add: dout is formed in the kernel, dn = bf16(fp32 sum over K of exact bf16 products): against the float64 product

    |dn - dn_ref| <= e = u_bf16 |dn_ref| + (K + 1) u sum_k |a_k| |b_k|         (one bf16 rounding of the accumulator; the fp32 sum)

and every output is LINEAR in dout, so that error passes through the absolute companions: dx gains
rstd (|gamma| e + mean_j (|gamma| e) + |xhat| mean_j (|gamma| e |xhat|)), dgamma gains sum_rows e |xhat|, dbeta sum_rows e.  The
epilogue then runs the row kernel's arithmetic on dn (32 lanes per row whatever N is: the same count of roundings), so its terms are
added with |dn_ref| + e in the place of |dout|.  The composed pair (b4c_gemm_nt with bf16 output, then b4c_layernorm_bwd_add) rounds at
the same points and obeys the same bound.

The bounds are what this arithmetic allows, not what the kernel was seen to reach; the measured worst ratios are in the docstring
of tests/test_gpu_pre_ln_kernels.py."""
import torch

from local_bounds import SECOND_ORDER, U_BF16, U_F32, UNDERFLOW, check, worst_ratio      # noqa: F401  (re-exported)


def _finish(b):
    return b * SECOND_ORDER + UNDERFLOW


def ln_bwd_add(dout, x, mean, rstd, gamma, res, out_dtype, dgamma0=None, dbeta0=None):
    """-> {'dx': (ref, bound), 'dgamma': (ref, bound), 'dbeta': (ref, bound)} in float64.  dout, x, res [rows, d]: the values the
    kernel reads; mean, rstd [rows]: the saved fp32 stats; gamma [d]; dgamma0 / dbeta0: what the sinks held before (None: zeros)."""
    dout, x, gamma, res = [t.detach().double().cpu() for t in (dout, x, gamma, res)]
    mean, rstd = mean.detach().double().cpu()[:, None], rstd.detach().double().cpu()[:, None]
    rows, d = x.shape
    u_out = U_BF16 if out_dtype == torch.bfloat16 else U_F32
    g0 = torch.zeros(d, dtype=torch.float64) if dgamma0 is None else dgamma0.detach().double().cpu()
    b0 = torch.zeros(d, dtype=torch.float64) if dbeta0 is None else dbeta0.detach().double().cpu()
    xhat = (x - mean) * rstd
    a = dout * gamma
    o = rstd * (a - a.mean(1, keepdim=True) - xhat * (a * xhat).mean(1, keepdim=True))
    dx = res + o
    A = rstd.abs() * (a.abs() + a.abs().mean(1, keepdim=True) + xhat.abs() * (a.abs() * xhat.abs()).mean(1, keepdim=True))
    b_dx = (d + 12) * U_F32 * A + U_F32 * (res.abs() + A) + u_out * dx.abs()
    dgamma = g0 + (dout * xhat).sum(0)
    dbeta = b0 + dout.sum(0)
    G = g0.abs() + (dout.abs() * xhat.abs()).sum(0)
    B = b0.abs() + dout.abs().sum(0)
    b_dg = (rows + 3) * U_F32 * G + U_F32 * dgamma.abs()
    b_db = rows * U_F32 * B + U_F32 * dbeta.abs()
    return {'dx': (dx, _finish(b_dx)), 'dgamma': (dgamma, _finish(b_dg)), 'dbeta': (dbeta, _finish(b_db))}


def gemm_ln_bwd_add(A, Bt, x, mean, rstd, gamma, res, dgamma0=None, dbeta0=None):
    """-> {'dn': (ref, bound), 'dx': ..., 'dgamma': ..., 'dbeta': ...} of b4c_gemm_nt_ln_bwd_add (bf16).  A [M, K], Bt [N, K]: the
    values the kernel reads; the rest as ln_bwd_add."""
    A, Bt = A.detach().double().cpu(), Bt.detach().double().cpu()
    K = A.shape[1]
    dn = A @ Bt.T
    e = U_BF16 * dn.abs() + (K + 1) * U_F32 * (A.abs() @ Bt.abs().T)
    ref = ln_bwd_add(dn, x, mean, rstd, gamma, res, torch.bfloat16, dgamma0, dbeta0)
    x64, g64 = x.detach().double().cpu(), gamma.detach().double().cpu()
    m64, r64 = mean.detach().double().cpu()[:, None], rstd.detach().double().cpu()[:, None]
    xhat = ((x64 - m64) * r64).abs()
    ge = g64.abs() * e
    p_dx = r64.abs() * (ge + ge.mean(1, keepdim=True) + xhat * (ge * xhat).mean(1, keepdim=True))
    res64 = res.detach().double().cpu()
    rows, d = x64.shape
    # the row arithmetic's terms at |dn| + e (ln_bwd_add's A), the |res| and |dx| terms of the true operands
    a_abs = dn.abs() + e
    Aterm = r64.abs() * (a_abs * g64.abs() + (a_abs * g64.abs()).mean(1, keepdim=True) +
                         xhat * (a_abs * g64.abs() * xhat).mean(1, keepdim=True))
    b_dx = p_dx + (d + 12) * U_F32 * Aterm + U_F32 * (res64.abs() + Aterm) + U_BF16 * ref['dx'][0].abs()
    g0 = torch.zeros(d, dtype=torch.float64) if dgamma0 is None else dgamma0.detach().double().cpu()
    b0 = torch.zeros(d, dtype=torch.float64) if dbeta0 is None else dbeta0.detach().double().cpu()
    b_dg = (e * xhat).sum(0) + (rows + 3) * U_F32 * (g0.abs() + (a_abs * xhat).sum(0)) + U_F32 * ref['dgamma'][0].abs()
    b_db = e.sum(0) + rows * U_F32 * (b0.abs() + a_abs.sum(0)) + U_F32 * ref['dbeta'][0].abs()
    return {'dn': (dn, _finish(e)), 'dx': (ref['dx'][0], _finish(b_dx)), 'dgamma': (ref['dgamma'][0], _finish(b_dg)),
            'dbeta': (ref['dbeta'][0], _finish(b_db))}
