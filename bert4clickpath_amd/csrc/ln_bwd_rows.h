// The LayerNorm backward row body and what its deterministic launches share (rowops.hip: b4c_add_dropout_layernorm_bwd,
// b4c_layernorm_bwd, b4c_embed_ln_bwd; pre_ln.hip: b4c_layernorm_bwd_add).  A row of d elements is owned by G lanes, 8 elements per
// lane per pass (rowops.hip, "residual + dropout + LayerNorm").
#pragma once
#include "common.h"

// blocks of a grid-stride row or element kernel
static inline int grid_for(int64_t work_items, int block) {
    int64_t g = ceil_div64(work_items, block);
    const int64_t cap = 256 * 8;  // 256 CUs x 8 blocks, grid-stride the rest
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

#define LN_MAX_PASS 2  // d <= 64 lanes * 8 elems * 2 passes = 1024 (keeps the per-lane row slice in registers)

// Where the backward's rows come from: load(row, c, go, zz) = the upstream gradient and the LayerNorm input, columns c .. c+7.
template <typename T> struct RowGradSrc {
    const T *dout, *z;
    int d;
    __device__ __forceinline__ void load(int64_t row, int c, float (&go)[8], float (&zz)[8]) const {
        Vec8<T>::load(dout + row * d + c, go);
        Vec8<T>::load(z + row * d + c, zz);
    }
};
// What the plain LayerNorm backward does to 8 results before they are stored: o *= act'(gate[row][c + k]) -- ReLU = the gate's sign,
// a GELU = its derivative (NULL: none) --, then o += res[row][c + k] (NULL: none; the residual stream's gradient of a pre-LN half).
template <typename T> struct GateResEpi {
    static constexpr bool kNone = false;
    const T *gate;
    int ld, act;
    const T *res;
    int ld_res;
    __device__ __forceinline__ void apply(int64_t row, int c, float (&o)[8]) const {
        if (gate) {
            float u[8];
            Vec8<T>::load(gate + row * ld + c, u);
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = act == B4C_ACT_RELU ? (u[k] > 0.f ? o[k] : 0.f) : o[k] * act_gelu_grad(u[k], act);
        }
        if (res) {
            float r[8];
            Vec8<T>::load(res + row * ld_res + c, r);
            // a plain add, never fused into the multiply that made o: with or without res the LayerNorm term is formed in one way
            {
#pragma clang fp contract(off)
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = r[k] + o[k];
            }
        }
    }
};
// b4c_layernorm_bwd and b4c_layernorm_bwd_add are ONE kernel (pre_ln.hip: ln_bwd_kernel), launched here with the arguments already
// checked: res == NULL is the former, gate == NULL the latter, so that res == 0 gives b4c_layernorm_bwd's bits by construction
__attribute__((visibility("hidden"))) int b4c_ln_bwd_gate_res(const void *dout, const void *x, const float *stats, const float *gamma, void *dx,
                                                              float *dgamma, float *dbeta, int64_t rows, int d, const void *gate, int ld_gate,
                                                              int gate_act, const void *res, int ld_res, void *workspace, int dtype,
                                                              void *stream, const char *who);

// The backward row body: dz = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dout * gamma.
// dgamma/dbeta: per-thread partials over the block's rows -> LDS -> one atomic per column per block.
// DET (deterministic form, `partial` != NULL): the threads' partials meet in a fixed order -- through LDS [row group][2][d], summed
// group by group, the block's sums stored to partial[block][2][d]; ln_bwd_reduce_kernel then adds the blocks in block order.
// dz pitch ld_dz; `epi` is applied to dz; dy = the forward's dropout on dz, written by the forms without an epilogue only.
template <typename T, int G, int NP, bool DET, typename Src, typename Epi>
__device__ __forceinline__ void ln_bwd_rows(const Src &src, const Epi &epi, const float *__restrict__ stats,
                                            const float *__restrict__ gamma, T *__restrict__ dz, int ld_dz, T *__restrict__ dy,
                                            float *__restrict__ dgamma, float *__restrict__ dbeta, int64_t rows, int d, float rate,
                                            uint64_t seed, float *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float red[];  // [2][d]  (DET: [256 / G][2][d])
    const int lane_in_row = threadIdx.x & (G - 1);
    const int rows_per_block = 256 / G;
    const float inv_keep = rate > 0.f ? 1.0f / (1.0f - rate) : 1.0f;
    const float inv_d = 1.0f / (float)d;
    if (!DET) {
        for (int i = threadIdx.x; i < 2 * d; i += 256) red[i] = 0.f;
        __syncthreads();
    }
    // NP = passes of G * 8 columns a row needs (1 for d <= 128 at G = 16): a runtime pass count kept the second pass's
    // 64 registers allocated
    float pg[NP][8], pb[NP][8];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int k = 0; k < 8; ++k) pg[p][k] = pb[p][k] = 0.f;

    for (int64_t row = blockIdx.x * (int64_t)rows_per_block + threadIdx.x / G; row < rows;
         row += (int64_t)gridDim.x * rows_per_block) {
        const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
        float gv[NP][8], xh[NP][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            {
                const int c = (p * G + lane_in_row) * 8;
                if (c < d) {
                    float go[8], zz[8], gm[8];
                    src.load(row, c, go, zz);
                    Vec8<float>::load(gamma + c, gm);
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        xh[p][k] = (zz[k] - mean) * rstd;
                        gv[p][k] = go[k] * gm[k];
                        s1 += gv[p][k];
                        s2 += gv[p][k] * xh[p][k];
                        pg[p][k] += go[k] * xh[p][k];
                        pb[p][k] += go[k];
                    }
                }
            }
        }
        s1 = group_sum<G>(s1) * inv_d;
        s2 = group_sum<G>(s2) * inv_d;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            {
                const int c = (p * G + lane_in_row) * 8;
                if (c < d) {
                    float o[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) o[k] = rstd * (gv[p][k] - s1 - xh[p][k] * s2);
                    if (!Epi::kNone) epi.apply(row, c, o);          // (a form with an epilogue has no dy: its callers pass rate 0)
                    Vec8<T>::template store_sel<B4C_NT(B4C_NT_LNBWD_DZ)>(dz + row * ld_dz + c, o);
                    if (Epi::kNone && rate > 0.f && dy) {
                        const uint32_t km = b4c_keep8(seed, (uint64_t)(row * d + c), b4c_keep_threshold(rate));
#pragma unroll
                        for (int k = 0; k < 8; ++k) o[k] = ((km >> k) & 1u) ? o[k] * inv_keep : 0.f;
                        Vec8<T>::template store_sel<B4C_NT(B4C_NT_LNBWD_DY)>(dy + row * d + c, o);
                    }
                }
            }
        }
    }
    if (DET) {
        float *mine = red + (threadIdx.x / G) * 2 * d;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int c = (p * G + lane_in_row) * 8;
            if (c < d) {
#pragma unroll
                for (int k = 0; k < 8; ++k) { mine[c + k] = pg[p][k]; mine[d + c + k] = pb[p][k]; }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * d; i += 256) {
            float sum = 0.f;
            for (int grp = 0; grp < rows_per_block; ++grp) sum += red[grp * 2 * d + i];
            partial[(int64_t)blockIdx.x * 2 * d + i] = sum;
        }
        return;
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        {
            const int c = (p * G + lane_in_row) * 8;
            if (c < d) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    atomicAdd(&red[c + k], pg[p][k]);
                    atomicAdd(&red[d + c + k], pb[p][k]);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < d; i += 256) {
        atomicAdd(dgamma + i, red[i]);
        atomicAdd(dbeta + i, red[d + i]);
    }
}

// dgamma[i] += sum over blocks of partial[block][0][i]; dbeta likewise.  One wave per column, in a FIXED order: lane l adds the
// blocks l, l + 64, l + 128, ... one after the other, then the 64 lane sums meet in wave_sum's fixed butterfly.
static __global__ void __launch_bounds__(256) ln_bwd_reduce_kernel(const float *__restrict__ partial, int nblocks, int d, float *__restrict__ dgamma,
                                                            float *__restrict__ dbeta) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= 2 * d) return;
    float sum = 0.f;
    for (int b = lane; b < nblocks; b += 64) sum += partial[(int64_t)b * 2 * d + i];
    sum = wave_sum(sum);
    if (lane == 0) { if (i < d) dgamma[i] += sum; else dbeta[i - d] += sum; }
}

static int ln_group(int d) {
    int g = 1;
    while (g * 8 < d && g < 64) g <<= 1;
    return g;
}

// grid, LDS bytes and passes of the deterministic backward kernels (ln_bwd_kernel, embed_ln_bwd_kernel): those of add_ln_bwd_kernel<.., true>
struct LnBwdShape {
    int g, grid, npass;
    size_t shm;
};
static LnBwdShape ln_bwd_shape(int64_t rows, int d) {
    LnBwdShape s;
    s.g = ln_group(d);
    s.grid = grid_for(rows * s.g, 256);
    if (s.grid > 1024) s.grid = 1024;      // b4c_add_dropout_layernorm_bwd_workspace_bytes holds 1024 blocks' partial sums
    s.npass = (d + s.g * 8 - 1) / (s.g * 8);
    s.shm = (size_t)(256 / s.g) * 2 * (size_t)d * sizeof(float);
    return s;
}
// KERNEL<TT, G, NP><<<grid, 256, shm, st>>>(args) for the row group and pass count of `sh`
#define LN_DET_BWD_DISPATCH(KERNEL, TT, sh, ...)                                                                     \
    switch ((sh).g) {                                                                                                \
        case 1: KERNEL<TT, 1, 1><<<(sh).grid, 256, (sh).shm, st>>> __VA_ARGS__; break;                               \
        case 2: KERNEL<TT, 2, 1><<<(sh).grid, 256, (sh).shm, st>>> __VA_ARGS__; break;                               \
        case 4: KERNEL<TT, 4, 1><<<(sh).grid, 256, (sh).shm, st>>> __VA_ARGS__; break;                               \
        case 8: KERNEL<TT, 8, 1><<<(sh).grid, 256, (sh).shm, st>>> __VA_ARGS__; break;                               \
        case 16: KERNEL<TT, 16, 1><<<(sh).grid, 256, (sh).shm, st>>> __VA_ARGS__; break;                             \
        case 32: KERNEL<TT, 32, 1><<<(sh).grid, 256, (sh).shm, st>>> __VA_ARGS__; break;                             \
        default: if ((sh).npass == 1) KERNEL<TT, 64, 1><<<(sh).grid, 256, (sh).shm, st>>> __VA_ARGS__;               \
                 else KERNEL<TT, 64, 2><<<(sh).grid, 256, (sh).shm, st>>> __VA_ARGS__; break;                        \
    }
