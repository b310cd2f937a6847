// The body of the feed-forward block's single-pass forward, shared by the ReLU kernel (ffn_fwd.hip: b4c_ffn_fwd) and the GELU kernels
// (ffn_act_fwd.hip: b4c_ffn_act_fwd).  ACT is a B4C_ACT_* constant; the GELU forms differ in three places, each under `if constexpr`:
// a second [32][128] LDS image for the pre-activation u, the epilogue of interval 1 (u and act(u) instead of relu), and the u rows
// that leave beside the h rows in interval 2.  The skeleton and its wait accounting are described in ffn_fwd.hip.
#pragma once
#include "dxdw_common.h"

#define FF_OSTR 528                  // bytes per staged y row: 128 fp32 + 16

struct FfnFwdArgs {
    const bf16_t *X;      // [M][ldx]
    const bf16_t *W1t;    // [Fp][ldw1]  row = hidden column, 128 entries (the forward operand of the first Dense)
    const float *b1;      // [Fp]
    const bf16_t *W2t;    // [128][ldw2] row = output column, Fp entries
    const float *b2, *gamma, *beta;   // [128]
    bf16_t *H;            // [M][ldh]   relu(x W1 + b1), Fp columns
    bf16_t *Z;            // [M][128] or NULL (inference)
    bf16_t *Out;          // [M][128]
    float *stats;         // [M][2] or NULL
    int ldx, ldw1, ldw2, ldh, Fp;
    float eps, rate;
    uint64_t seed;
    int64_t M;
};
struct FfnFwdActArgs : FfnFwdArgs {
    bf16_t *U;            // [M][ldu]   x W1 + b1 (the pre-activation), Fp columns, or NULL (inference)
    int ldu;
};

// bytes of LDS: the x ring, the h image, the staged y, the parameters (and the u image)
template <int ACT> constexpr size_t ffn_fwd_lds() {
    return DD_RING * (size_t)DD_SUB + DD_SUB + DD_TOK * FF_OSTR + 3 * 128 * 4 + (ACT == B4C_ACT_RELU ? 0 : DD_SUB);
}

template <int ACT, class Args> __device__ __forceinline__ void ffn_fwd_body(const Args a) {
    constexpr bool GELU = ACT != B4C_ACT_RELU;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int STAGE = DD_SUB;                       // x
    char *sH = smem + DD_RING * STAGE;                  // [32][128] bf16 image of h
    char *sOut = sH + DD_SUB;                           // [32][FF_OSTR] fp32 y = h W2^T
    float *sPar = reinterpret_cast<float *>(sOut + DD_TOK * FF_OSTR);   // [3][128]: b2, gamma, beta (read per tile: registers are short at two workgroups per CU)
    char *sU = reinterpret_cast<char *>(sPar + 3 * 128);                // GELU: [32][128] bf16 image of u = x W1^T + b1
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int orow = tid >> 4, opart = tid & 15;        // row phase: token row of the tile, 8-column piece
    const int64_t ntile_all = (a.M + DD_TOK - 1) / DD_TOK;
    const int64_t t1 = (ntile_all - blockIdx.x + gridDim.x - 1) / gridDim.x;      // this workgroup's tile count (>= 1)
    const int64_t gstep = gridDim.x, gfirst = blockIdx.x;

    // resident operands: this wave's 16 output columns of each layer, B[k = 32 ks + 8 g + j][col = 16 wave + li]
    bf16x8 w1f[4], w2f[4];
    float bias1[4];
    {
        const bf16x8 zero = __builtin_bit_cast(bf16x8, (u32x4){0u, 0u, 0u, 0u});
        const int col = 16 * wave + li;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int k = ks * 32 + 8 * g;
            w1f[ks] = col < a.Fp ? *reinterpret_cast<const bf16x8 *>(a.W1t + (int64_t)col * a.ldw1 + k) : zero;
            w2f[ks] = k < a.Fp ? *reinterpret_cast<const bf16x8 *>(a.W2t + (int64_t)col * a.ldw2 + k) : zero;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int c = 16 * wave + 4 * g + j; bias1[j] = c < a.Fp ? a.b1[c] : 0.f; }
    }
    if (tid < 128) { sPar[tid] = a.b2[tid]; sPar[128 + tid] = a.gamma[tid]; sPar[256 + tid] = a.beta[tid]; }
    // the compiler's own loads are consumed HERE: its wait for them would otherwise sit at their first use inside the tile loop, where
    // it counts none of the requests below and drains them every iteration
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) { asm volatile("" : "+v"(w1f[ks])); asm volatile("" : "+v"(w2f[ks])); }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (and the parameter loads above)
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(bias1[j]));

    int xoff[2][4], poff[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int q = 0; q < 4; ++q) xoff[mi][q] = VTile<128>::chunk_off(16 * mi + li, 4 * q + g);
        // the lane's 4 consecutive columns 16 wave + 4 g .. + 3 of token 16 mi + li inside an image (8-B piece of a 16-B chunk)
        poff[mi] = VTile<128>::chunk_off(16 * mi + li, (16 * wave + 4 * g) >> 3) + ((4 * g) & 7) * 2;
    }
    const int rowoff = VTile<128>::chunk_off(orow, opart);

    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem;
    auto fetch = [&](int64_t t) {
        const int64_t tok0 = (gfirst + t * gstep) * DD_TOK;
        const int64_t M = t < t1 ? a.M : 0;             // past the last tile: zero rows (still an LDS write, still counted)
        dd_dma(a.X, a.ldx, 0, tok0, M, lds0 + (unsigned)((int)(t & 3) * STAGE), wave, lane);
    };
    fetch(0);
    fetch(1);
    fetch(2);
    const float inv_keep = a.rate > 0.f ? 1.0f / (1.0f - a.rate) : 1.0f;
    const uint32_t thr = b4c_keep_threshold(a.rate);

    // rows of tile tp: staged y, the x image of its ring stage -> z, out, stats
    auto row_phase = [&](int64_t tp) {
        const int64_t tk = (gfirst + tp * gstep) * DD_TOK + orow;
        const f32x4 lo = *reinterpret_cast<const f32x4 *>(sOut + orow * FF_OSTR + opart * 32);
        const f32x4 hi = *reinterpret_cast<const f32x4 *>(sOut + orow * FF_OSTR + opart * 32 + 16);
        const bf16x8 xv = *reinterpret_cast<const bf16x8 *>(smem + (int)(tp & 3) * STAGE + rowoff);
        const uint32_t km = a.rate > 0.f ? b4c_keep8(a.seed, (uint64_t)(tk * 128 + opart * 8), thr) : 0xFFu;
        float v[8], sum = 0.f, bias2[8];
        Vec8<float>::load(sPar + 8 * opart, bias2);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float yy = (k < 4 ? lo[k] : hi[k - 4]) + bias2[k];
            // GELU: y with the rounding points of b4c_gemm_nt_add_ln, the kernel this replaces there (the sum to bf16, + b2, to bf16
            // again: "the bf16 y that gemm_nt would have stored"), so that z, out and stats are its numbers up to the order of the
            // fp32 sum.  Measured on a 24-sequence model: with y kept in fp32 here, as the ReLU kernel keeps it, the two routes'
            // steps are 2.7 % (L2, median over the gradient tensors; ReLU: 2.9 %) apart through the bf16 steps of z alone.
            if constexpr (GELU) yy = (float)(bf16_t)((float)(bf16_t)(k < 4 ? lo[k] : hi[k - 4]) + bias2[k]);
            if (a.rate > 0.f) yy = ((km >> k) & 1u) ? yy * inv_keep : 0.f;
            v[k] = (float)xv[k] + yy;
            sum += v[k];
        }
        const float mean = group_sum<16>(sum) * (1.0f / 128.0f);
        float sq = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) { const float dlt = v[k] - mean; sq += dlt * dlt; }
        const float var = group_sum<16>(sq) * (1.0f / 128.0f);
        const float rstd = 1.0f / sqrtf(var + a.eps);
        if (tk < a.M) {
            float o[8], gm[8], bt[8];
            Vec8<float>::load(sPar + 128 + 8 * opart, gm);
            Vec8<float>::load(sPar + 256 + 8 * opart, bt);
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = (v[k] - mean) * rstd * gm[k] + bt[k];
            if (a.Z) Vec8<bf16_t>::template store_sel<B4C_NT(B4C_NT_GEMMLN_Z)>(a.Z + tk * 128 + opart * 8, v);
            Vec8<bf16_t>::template store_sel<B4C_NT(B4C_NT_GEMMLN_OUT)>(a.Out + tk * 128 + opart * 8, o);
            if (a.stats && opart == 0) { a.stats[tk * 2] = mean; a.stats[tk * 2 + 1] = rstd; }
        }
    };

    // Iteration t (0 .. t1; the last one only finishes tile t1 - 1), two barrier intervals.  Vector-memory operations per thread in
    // issue order: [z, out, stats stores of tile t - 1] | [DMA of x(t + 3)] [h store of tile t].  The only wait: x(t) landed -- its DMA
    // went out in iteration t - 3; issued since, at least: the h store of that iteration and [out store, DMA, h store] of the two
    // iterations between (inference: no z, no stats) = 7 operations, 11 when training.  `vmcnt(6)` is safe in every mode (a smaller
    // count only waits for more); the first three iterations wait for all but one.
    // GELU: [z, out, stats stores of tile t - 1] | [DMA of x(t + 3)] [h store of tile t] [u store of tile t when U is given].  The u
    // store only adds to what is issued behind x(t)'s DMA: the fewest (inference, U == NULL) are the same 7, training has 14, and
    // the same `vmcnt(6)` / `vmcnt(1)` hold (tests/test_vmcnt_ffn_act.py: m = 3, the DMAs of x(t + 2), x(t + 1), x(t)).
    for (int64_t t = 0; t <= t1; ++t) {
        const bool body = t < t1;
        const int slot = (int)(t & 3);
        // (tests/test_vmcnt_accounting.py checks both counts in the assembly: ffn_fwd.first, ffn_fwd.steady)
        if (body) { if (t < 3) asm volatile("s_waitcnt vmcnt(1) ; vmcheck ffn_fwd.first" ::: "memory"); else asm volatile("s_waitcnt vmcnt(6) ; vmcheck ffn_fwd.steady" ::: "memory"); }
        __syncthreads();                                // x(t) landed for every wave; the staged y of tile t - 1 complete, its h image read
        if (body) {
            // ---- h = act(x W1^T + b1): this wave's 16 hidden columns x 32 tokens ----
            const char *sx = smem + slot * STAGE;
            f32x4 ax[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            bf16x8 fg[2][4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) fg[mi][q] = *reinterpret_cast<const bf16x8 *>(sx + xoff[mi][q]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) ax[mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1f[q], fg[mi][q], ax[mi], 0, 0, 0);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                bf16x4 w;
                if constexpr (GELU) {
                    // u = bf16(x W1^T) + b1 in fp32 -> both images.  The sum is rounded to bf16 BEFORE the bias because b4c_gemm_nt_act's
                    // bf16 epilogue stages it so: u and h then hold the numbers of the two-kernel route (up to the order of the fp32
                    // sum), and a model computes the same step on either route.  A column past Fp has a zero W1 fragment and a zero
                    // bias: u = 0, act(0) = 0
                    bf16x4 pre;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float u = (float)(bf16_t)ax[mi][j] + bias1[j];
                        pre[j] = (bf16_t)u;
                        w[j] = (bf16_t)act_gelu(u, ACT);
                    }
                    *reinterpret_cast<bf16x4 *>(sU + poff[mi]) = pre;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) w[j] = (bf16_t)fmaxf(ax[mi][j] + bias1[j], 0.f);
                }
                *reinterpret_cast<bf16x4 *>(sH + poff[mi]) = w;
            }
        }
        if (t > 0) row_phase(t - 1);
        if (!body) break;
        __syncthreads();                                // the h image of tile t complete; the staged y and the x image of tile t - 1 read
        fetch(t + 3);                                   // into the stage that held tile t - 1
        {
            // ---- y = h W2^T: this wave's 16 output columns x 32 tokens ----
            f32x4 ax[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            bf16x8 fg[2][4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) fg[mi][q] = *reinterpret_cast<const bf16x8 *>(sH + xoff[mi][q]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) ax[mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2f[q], fg[mi][q], ax[mi], 0, 0, 0);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) *reinterpret_cast<f32x4 *>(sOut + (16 * mi + li) * FF_OSTR + (16 * wave + 4 * g) * 4) = ax[mi];
            // h rows of tile t -> global (16-B chunks of the image)
            const int64_t tk = (gfirst + t * gstep) * DD_TOK + orow;
            if (tk < a.M && opart * 8 < a.Fp) {
                const u32x4 hv = *reinterpret_cast<const u32x4 *>(sH + rowoff);
                *reinterpret_cast<u32x4 *>(a.H + tk * a.ldh + opart * 8) = hv;
                if constexpr (GELU) {
                    if (a.U) {                                  // (training: the backward pass gates with act'(u))
                        const u32x4 uv = *reinterpret_cast<const u32x4 *>(sU + rowoff);
                        *reinterpret_cast<u32x4 *>(a.U + tk * a.ldu + opart * 8) = uv;
                    }
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // requests past the last tile (zero rows) are still LDS writes: none may outlive the workgroup
}
