// Forward of the feed-forward block with a GELU activation in ONE pass:
//     out = LayerNorm(x + dropout(act(x W1 + b1) W2 + b2)),  act = B4C_ACT_GELU (erf) or B4C_ACT_GELU_TANH
// The skeleton, the ring and the wait accounting are ffn_fwd.hip's (the body is one template: ffn_fwd_body.h).  A GELU block saves
// the pre-activation u beside h = act(u) -- GELU is not monotone, its backward gates with act'(u) -- so interval 1 forms
// u = bf16(acc) + b1 in fp32 (b4c_gemm_nt_act's rounding points: see ffn_fwd_body.h) and writes bf16(act(u)) into the h image and
// bf16(u) into a second [32][128] image; the u rows leave in interval 2 beside the h rows (training only: U may be NULL at
// inference); the row phase takes y with b4c_gemm_nt_add_ln's rounding points.  As two kernels (b4c_gemm_nt_act with `pre`,
// b4c_gemm_nt_add_ln) h is written and read back and x is read twice; here x is read once and h, u leave once.
// 66 KB of LDS and <= 128 registers: two workgroups per CU, as the ReLU kernel.
#include <stdlib.h>

#include "ffn_fwd_body.h"

template <int ACT> __global__ void __launch_bounds__(512, 4) ffn_act_fwd_kernel(FfnFwdActArgs a) { ffn_fwd_body<ACT>(a); }

template <int ACT> static void ffn_act_fwd_launch(const FfnFwdActArgs &a, int grid, hipStream_t st) {
    constexpr size_t lds = ffn_fwd_lds<ACT>();
    b4c_allow_lds(ffn_act_fwd_kernel<ACT>, lds);
    ffn_act_fwd_kernel<ACT><<<grid, 512, lds, st>>>(a);
}

extern "C" int b4c_ffn_act_fwd(const void *X, int ldx, const void *W1t, int ldw1, const float *b1, const void *W2t, int ldw2,
                               const float *b2, const float *gamma, const float *beta, int F, int Fp, int act, void *H, int ldh,
                               void *U, int ldu, void *Z, void *Out, float *stats, int64_t M, float eps, float dropout_rate,
                               uint64_t seed, void *stream) {
    B4C_REQUIRE(X && W1t && b1 && W2t && b2 && gamma && beta && H && Out, "ffn_act_fwd: null pointer");
    B4C_REQUIRE(act == B4C_ACT_GELU || act == B4C_ACT_GELU_TANH, "ffn_act_fwd: act %d (B4C_ACT_GELU or B4C_ACT_GELU_TANH; b4c_ffn_fwd is the ReLU kernel)", act);
    B4C_REQUIRE(U || !Z, "ffn_act_fwd: a training call (Z given) needs the pre-activation output U");
    B4C_REQUIRE(M > 0 && F > 0 && F <= Fp && Fp <= 128 && Fp % 8 == 0, "ffn_act_fwd: hidden width %d (padded %d): 1..128, padded to a multiple of 8", F, Fp);
    B4C_REQUIRE(ldx >= 128 && ldw1 >= 128 && ldw2 >= Fp && ldh >= Fp && (!U || ldu >= Fp), "ffn_act_fwd: shape");
    B4C_REQUIRE(ldx % 8 == 0 && ldw1 % 8 == 0 && ldw2 % 8 == 0 && ldh % 8 == 0 && (!U || ldu % 8 == 0) &&
                ((((uintptr_t)X | (uintptr_t)W1t | (uintptr_t)W2t | (uintptr_t)H | (uintptr_t)U | (uintptr_t)Z | (uintptr_t)Out |
                   (uintptr_t)b2 | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0) && (((uintptr_t)stats & 7) == 0) &&
                (((uintptr_t)b1 & 3) == 0),
                "ffn_act_fwd: operands must be 16-byte aligned with pitches % 8 == 0");
    B4C_REQUIRE(dropout_rate >= 0.f && dropout_rate < 1.f, "ffn_act_fwd: dropout rate");
    FfnFwdActArgs a = {};
    a.X = (const bf16_t *)X; a.W1t = (const bf16_t *)W1t; a.b1 = b1; a.W2t = (const bf16_t *)W2t; a.b2 = b2; a.gamma = gamma; a.beta = beta;
    a.H = (bf16_t *)H; a.Z = (bf16_t *)Z; a.Out = (bf16_t *)Out; a.stats = stats;
    a.ldx = ldx; a.ldw1 = ldw1; a.ldw2 = ldw2; a.ldh = ldh; a.Fp = Fp;
    a.eps = eps; a.rate = dropout_rate; a.seed = seed; a.M = M;
    a.U = (bf16_t *)U; a.ldu = ldu;
    const int64_t ntiles = (M + DD_TOK - 1) / DD_TOK;
    const int grid = (int)(ntiles < 512 ? ntiles : 512);        // two workgroups per CU
    if (act == B4C_ACT_GELU) ffn_act_fwd_launch<B4C_ACT_GELU>(a, grid, (hipStream_t)stream);
    else ffn_act_fwd_launch<B4C_ACT_GELU_TANH>(a, grid, (hipStream_t)stream);
    return b4c_check_launch("ffn_act_fwd");
}
