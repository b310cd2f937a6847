// Forward of the position-wise feed-forward block of one encoder layer in ONE pass (round 4):
//     out = LayerNorm(x + dropout(relu(x W1 + b1) W2 + b2))                                (transformer.py:154-170)
// As two kernels (b4c_gemm_nt with ReLU, b4c_gemm_nt_add_ln) the hidden activation h [T][Fp] is written and read back and x is read
// twice: 658 MB per launch at the C2 token count.  Here h leaves once (the backward pass needs it) and is consumed from LDS, x is
// read once: x in; h, z, out, stats out -- 446 MB.
//
// A persistent 512-thread workgroup walks 32-token tiles (tile i of a workgroup = global tile blockIdx.x + i gridDim.x), the skeleton
// of ffn_bwd.hip / attn_out_bwd.hip:
//   LDS-DMA     x tile [32][128] into a four-stage ring of XOR-swizzled images, three tiles ahead
//   interval 1  h = relu(x W1^T + b1) of tile t (MFMA 16x16x32: the wave's 16 hidden columns of W1 resident) -> bf16 LDS image  |
//               rows of tile t - 1: y + b2 from the staged tile, dropout, z = x + drop(y), LayerNorm with 16-lane sums
//               (add_ln_fwd's layout and order) -> z, out, stats -> global
//   interval 2  y = h W2^T of tile t (the wave's 16 output columns of W2 resident) -> fp32 staged tile  |  h rows of tile t -> global
// No register ever waits for a load in flight (every request is an LDS-DMA); the only counted wait is for tile t's x image.
// d_model = 128, dff <= 128, bf16: every other shape keeps the two kernels.
#include <stdlib.h>

#include "ffn_fwd_body.h"

// (the body, shared with the GELU kernels of ffn_act_fwd.hip: ffn_fwd_body.h)
__global__ void __launch_bounds__(512, 4) ffn_fwd_kernel(FfnFwdArgs a) { ffn_fwd_body<B4C_ACT_RELU>(a); }

extern "C" int b4c_ffn_fwd(const void *X, int ldx, const void *W1t, int ldw1, const float *b1, const void *W2t, int ldw2, const float *b2,
                           const float *gamma, const float *beta, int F, int Fp, void *H, int ldh, void *Z, void *Out, float *stats,
                           int64_t M, float eps, float dropout_rate, uint64_t seed, void *stream) {
    B4C_REQUIRE(X && W1t && b1 && W2t && b2 && gamma && beta && H && Out, "ffn_fwd: null pointer");
    B4C_REQUIRE(M > 0 && F > 0 && F <= Fp && Fp <= 128 && Fp % 8 == 0, "ffn_fwd: hidden width %d (padded %d): 1..128, padded to a multiple of 8", F, Fp);
    B4C_REQUIRE(ldx >= 128 && ldw1 >= 128 && ldw2 >= Fp && ldh >= Fp, "ffn_fwd: shape");
    B4C_REQUIRE(ldx % 8 == 0 && ldw1 % 8 == 0 && ldw2 % 8 == 0 && ldh % 8 == 0 &&
                ((((uintptr_t)X | (uintptr_t)W1t | (uintptr_t)W2t | (uintptr_t)H | (uintptr_t)Z | (uintptr_t)Out | (uintptr_t)b2 |
                   (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0) && (((uintptr_t)stats & 7) == 0) && (((uintptr_t)b1 & 3) == 0),
                "ffn_fwd: operands must be 16-byte aligned with pitches % 8 == 0");
    B4C_REQUIRE(dropout_rate >= 0.f && dropout_rate < 1.f, "ffn_fwd: dropout rate");
    FfnFwdArgs a = {};
    a.X = (const bf16_t *)X; a.W1t = (const bf16_t *)W1t; a.b1 = b1; a.W2t = (const bf16_t *)W2t; a.b2 = b2; a.gamma = gamma; a.beta = beta;
    a.H = (bf16_t *)H; a.Z = (bf16_t *)Z; a.Out = (bf16_t *)Out; a.stats = stats;
    a.ldx = ldx; a.ldw1 = ldw1; a.ldw2 = ldw2; a.ldh = ldh; a.Fp = Fp;
    a.eps = eps; a.rate = dropout_rate; a.seed = seed; a.M = M;
    const int64_t ntiles = (M + DD_TOK - 1) / DD_TOK;
    const int grid = (int)(ntiles < 512 ? ntiles : 512);        // two workgroups per CU (57 KB of LDS, <= 128 registers each)
    const size_t lds = ffn_fwd_lds<B4C_ACT_RELU>();
    b4c_allow_lds(ffn_fwd_kernel, lds);
    ffn_fwd_kernel<<<grid, 512, lds, (hipStream_t)stream>>>(a);
    return b4c_check_launch("ffn_fwd");
}
