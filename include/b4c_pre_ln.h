/* b4c_pre_ln.h -- the backward of a pre-LN encoder half's input norm: the LayerNorm backward of the sublayer-input gradient with
 * the residual stream's gradient added as it is stored.  A PRE-LN header of include/b4c.h (which includes it; a caller includes
 * b4c.h).  Additive to ABI 12: no signature of b4c.h, of its extension header or of an add-on header changed, b4c_abi_version()
 * stays 12.  Error codes and dtype codes are b4c.h's.  (The ctypes binding reads this header beside the others:
 * bert4clickpath_amd/_lib.py, PRE_LN_HEADER_PATHS.)
 *
 * A pre-LN half is  x' = x + drop(sublayer(LN(x; gamma, beta))).  With g the gradient of x' and dn the gradient of the normalised
 * rows that the sublayer's backward leaves,  dx = g + LNbwd(dn; x, stats, gamma):  the forward needs no kernel of its own
 * (b4c_layernorm_fwd, b4c_gemm_nt_add_ln / b4c_add_dropout_layernorm_fwd with the NEXT norm's gamma / beta), this sum does. */
#ifndef B4C_PRE_LN_H
#define B4C_PRE_LN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dx[row][j] = res[row][j] + rstd * (a - mean_j(a) - xhat * mean_j(a * xhat)),  a = dout * gamma, xhat = (x - mean) * rstd from the
 * saved stats [rows][2] = {mean, rstd}: b4c_layernorm_bwd (gate == NULL) with `res` added in fp32 before the one rounding of the
 * store.  dout, x, dx: [rows][d] contiguous; res: [rows][d] with pitch ld_res elements (>= d, a multiple of 8; 16-byte aligned),
 * required.  dgamma += sum_rows dout * xhat, dbeta += sum_rows dout (fp32 [d], ADDED to) through per-workgroup sums in the
 * workspace (b4c_layernorm_bwd_add_workspace_bytes, required), added in a fixed order: no float atomics, the same bits on every
 * launch, and the bits of b4c_layernorm_bwd on the same operands.  res == 0 everywhere gives b4c_layernorm_bwd's dx bit for bit.
 * fp32 and bf16; d a multiple of 8, <= 1024; rows is a 64-bit count.  dx must not overlap an input.  Bad arguments: B4C_EINVAL,
 * nothing is launched. */
int64_t b4c_layernorm_bwd_add_workspace_bytes(int64_t rows, int d);
int b4c_layernorm_bwd_add(const void *dout, const void *x, const float *stats, const float *gamma, const void *res, int ld_res,
                          void *dx, float *dgamma, float *dbeta, int64_t rows, int d, void *workspace, int64_t workspace_bytes,
                          int dtype, void *stream);

/* The same with dout = A . Bt^T formed in the kernel (matrix cores), so that the sublayer-input gradient never reaches memory:
 *   dn = bf16(A . Bt^T)  -- the accumulator rounded to the bf16 value b4c_gemm_nt (act NONE, no bias) would have stored --
 *   dx = res + LNbwd(dn; x, stats, gamma),  dgamma += sum_rows dn * xhat,  dbeta += sum_rows dn.
 * A [M][K] (pitch lda), Bt [N][K] (pitch ldb: the dX operand of b4c_gemm_nt), x / dx [M][N] contiguous, res [M][N] with pitch
 * ld_res; bf16 only; N = d_model <= 256, N and K multiples of 8 (K covers 3 d and the padded dff); lda, ldb >= K, multiples of 8,
 * and a 128-row tile of either spans less than 2^30 bytes (b4c_gemm_nt's rule); every operand 16-byte aligned.  A workgroup
 * owns complete rows, so the two row sums of the LayerNorm backward are taken in its epilogue; taking this kernel or b4c_gemm_nt +
 * b4c_layernorm_bwd_add differs by the order of fp32 sums only.  Deterministic: per-workgroup dgamma / dbeta sums through the
 * workspace (b4c_gemm_nt_ln_bwd_add_workspace_bytes, required) in a fixed order.  Bad arguments: B4C_EINVAL, nothing is launched. */
int64_t b4c_gemm_nt_ln_bwd_add_workspace_bytes(int M, int N);
int b4c_gemm_nt_ln_bwd_add(const void *A, int lda, const void *Bt, int ldb, const void *x, const float *stats, const float *gamma,
                           const void *res, int ld_res, void *dx, float *dgamma, float *dbeta, int M, int N, int K, void *workspace,
                           int64_t workspace_bytes, int dtype, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* B4C_PRE_LN_H */
