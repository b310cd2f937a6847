// Pre-LN encoder halves (include/b4c.h): x' = x + drop(sublayer(LN(x))).  The forward runs on the post-LN launches with the
// LayerNorm parameters shifted by one place; the backward needs  dx = g + LNbwd(dn; x, stats, gamma)  -- the residual stream's
// gradient g added to the LayerNorm backward of the sublayer-input gradient dn.  The row kernel here is b4c_layernorm_bwd's (its
// row body: ln_bwd_rows.h) with that sum as its epilogue, rounded once more at the store; b4c_layernorm_bwd launches the same kernel.
#include "ln_bwd_rows.h"
#include "mfma.h"

// plain LayerNorm backward, deterministic form only: dx = epi(LNbwd(dout)) -- the activation gate in front of the norm and / or the
// residual stream's gradient behind it (GateResEpi)
template <typename T, int G, int NP>
__global__ void __launch_bounds__(256, 4) ln_bwd_kernel(const T *__restrict__ dout, const T *__restrict__ x,
                                                        const float *__restrict__ stats, const float *__restrict__ gamma,
                                                        T *__restrict__ dx, GateResEpi<T> epi, int64_t rows, int d,
                                                        float *__restrict__ partial) {
    const RowGradSrc<T> src = {dout, x, d};
    ln_bwd_rows<T, G, NP, true>(src, epi, stats, gamma, dx, d, (T *)nullptr, (float *)nullptr, (float *)nullptr, rows, d, 0.f, 0, partial);
}

int b4c_ln_bwd_gate_res(const void *dout, const void *x, const float *stats, const float *gamma, void *dx, float *dgamma, float *dbeta,
                        int64_t rows, int d, const void *gate, int ld_gate, int gate_act, const void *res, int ld_res, void *workspace,
                        int dtype, void *stream, const char *who) {
    const LnBwdShape sh = ln_bwd_shape(rows, d);
    float *partial = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == B4C_F32) {
        const GateResEpi<float> ge = {(const float *)gate, ld_gate, gate_act, (const float *)res, ld_res};
        LN_DET_BWD_DISPATCH(ln_bwd_kernel, float, sh, ((const float *)dout, (const float *)x, stats, gamma, (float *)dx, ge, rows, d, partial))
    } else {
        const GateResEpi<bf16_t> ge = {(const bf16_t *)gate, ld_gate, gate_act, (const bf16_t *)res, ld_res};
        LN_DET_BWD_DISPATCH(ln_bwd_kernel, bf16_t, sh, ((const bf16_t *)dout, (const bf16_t *)x, stats, gamma, (bf16_t *)dx, ge, rows, d, partial))
    }
    ln_bwd_reduce_kernel<<<(2 * d + 3) / 4, 256, 0, st>>>(partial, sh.grid, d, dgamma, dbeta);
    return b4c_check_launch(who);
}

extern "C" int64_t b4c_layernorm_bwd_add_workspace_bytes(int64_t rows, int d) { return b4c_layernorm_bwd_workspace_bytes(rows, d); }

extern "C" int b4c_layernorm_bwd_add(const void *dout, const void *x, const float *stats, const float *gamma, const void *res,
                                     int ld_res, void *dx, float *dgamma, float *dbeta, int64_t rows, int d, void *workspace,
                                     int64_t workspace_bytes, int dtype, void *stream) {
    B4C_REQUIRE(dout && x && stats && gamma && res && dx && dgamma && dbeta && rows > 0, "layernorm_bwd_add: null pointer / empty");
    B4C_REQUIRE(d > 0 && d % 8 == 0 && d <= 64 * 8 * LN_MAX_PASS, "layernorm_bwd_add: d=%d must be a multiple of 8, <= 1024", d);
    B4C_REQUIRE(ld_res >= d && ld_res % 8 == 0 && ((uintptr_t)res & 15) == 0, "layernorm_bwd_add: res pitch %d (>= d, a multiple of 8, 16-byte aligned rows)", ld_res);
    B4C_REQUIRE(workspace && workspace_bytes >= b4c_layernorm_bwd_add_workspace_bytes(rows, d), "layernorm_bwd_add: workspace too small");
    B4C_REQUIRE(dtype == B4C_F32 || dtype == B4C_BF16, "layernorm_bwd_add: dtype %d", dtype);
    return b4c_ln_bwd_gate_res(dout, x, stats, gamma, dx, dgamma, dbeta, rows, d, nullptr, 0, B4C_ACT_RELU, res, ld_res, workspace, dtype,
                               stream, "layernorm_bwd_add");
}

// ------------------------------------------------------------------------------------------
// The same with dout = A . Bt^T computed in the kernel (bf16, N = d_model <= 256): the last GEMM of a sublayer's backward -- dn =
// dqkv Wqkv^T or dn = dh W1^T -- and the input norm's backward in one pass, so that the sublayer-input gradient dn never goes to
// HBM (2 of the 5 [T][d] passes of b4c_gemm_nt + b4c_layernorm_bwd_add).  It mirrors b4c_gemm_nt_add_ln's wide form: a workgroup
// owns 64 whole rows x 256 columns (4 waves side by side along N, each 64 x 64 = 2 x 2 MFMA 32x32x16 tiles), operands staged
// through LDS as [rows][128 B of K] with a 16-B row pad (144-B stride: conflict-free ds_read_b128), one LDS stage with register
// prefetch of the next K tile.  MFMA roles are swapped (acc^T = Bt_tile . A_tile^T: rows = n in the registers, col = m on the
// lane), so a lane owns 4 consecutive n of one row and the accumulator leaves as 8-byte LDS writes -- rounded to bf16 there: the
// value b4c_gemm_nt would have stored.  The epilogue then gives a row to 32 consecutive lanes (8 columns each) and runs
// ln_bwd_rows' arithmetic on it.  Workgroups walk the row tiles grid-stride and keep their dgamma / dbeta sums in registers; they meet as in ln_bwd_rows' deterministic form: LDS [row group][2][N], summed group by group,
// one partial per workgroup, ln_bwd_reduce_kernel.
// ------------------------------------------------------------------------------------------
#define PL_TM 64
#define PL_TN 256
#define PL_STRIDE 144                                      // bytes per staged operand row (128 + 16 pad)
#define PL_STAGE_BYTES ((PL_TM + PL_TN) * PL_STRIDE)       // 46,080 (the registers, 234 per lane, set the occupancy: two workgroups per CU)
#define PL_OUT_STRIDE 520                                  // bytes per staged dn row: 512 + 8 (8-byte writes spread over the banks)
#define PL_MAX_GRID 1024                                   // the workspace holds 1024 workgroups' partial sums

// a raw buffer descriptor over the rows of a tile: rows outside it read as 0 (no branch in the staging loops); the byte count is
// said to be wave-uniform once, so that the descriptor stays in SGPRs
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pl_rsrc(const void *base, int64_t rows_left, int tile_rows, int64_t row_bytes) {
    const int64_t rows = rows_left < tile_rows ? (rows_left < 0 ? 0 : rows_left) : tile_rows;
    const int64_t bytes = rows * row_bytes;
    const unsigned nb = __builtin_amdgcn_readfirstlane((unsigned)(bytes > 0x3FFFFFF0ll ? 0x3FFFFFF0ll : bytes));
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, nb, 0x00020000);
}
// or-ed into a byte offset it pushes the access past every tile descriptor (a K chunk behind K reads as 0)
__device__ __forceinline__ int pl_oob(bool invalid) { return invalid ? 0x40000000 : 0; }

// 64 rows x 64 K elements of A: 512 16-B chunks, 2 per thread, 8 lanes per row
__device__ __forceinline__ void pl_load_a(const bf16_t *__restrict__ P, int ld, int64_t row0, int64_t nrows, int k0, int K, int tid, u32x4 (&reg)[2]) {
    const __amdgpu_buffer_rsrc_t rs = pl_rsrc(P + row0 * ld, nrows - row0, PL_TM, (int64_t)ld * 2);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + i * 256;
        const int row = c >> 3, gk = k0 + (c & 7) * 8;
        reg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, ((row * ld + gk) * 2) | pl_oob(gk >= K), 0, 0);
    }
}
// 256 rows x 64 K elements of Bt as two 128-row tiles (a tile's descriptor spans less than 2^30 bytes: b4c_gemm_nt's pitch rule)
__device__ __forceinline__ void pl_load_b(const bf16_t *__restrict__ P, int ld, int nrows, int k0, int K, int tid, u32x4 (&reg)[8]) {
    const __amdgpu_buffer_rsrc_t rs0 = pl_rsrc(P, (int64_t)nrows, 128, (int64_t)ld * 2);
    const __amdgpu_buffer_rsrc_t rs1 = pl_rsrc(P + (int64_t)128 * ld, (int64_t)nrows - 128, 128, (int64_t)ld * 2);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = tid + (i & 3) * 256;
        const int row = c >> 3, gk = k0 + (c & 7) * 8;
        reg[i] = __builtin_amdgcn_raw_buffer_load_b128(i < 4 ? rs0 : rs1, ((row * ld + gk) * 2) | pl_oob(gk >= K), 0, 0);
    }
}
template <int NR> __device__ __forceinline__ void pl_store(char *s, int tid, const u32x4 (&reg)[NR]) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int c = tid + i * 256;
        *reinterpret_cast<u32x4 *>(s + (c >> 3) * PL_STRIDE + (c & 7) * 16) = reg[i];
    }
}
// one stage of MFMAs: acc[j][i] += Bt_tile(rows wave*64 + j*32 ..) . A_tile(rows i*32 ..)^T over 64 K elements
__device__ __forceinline__ void pl_mma_stage(const char *sB, const char *sA, int wave, int r, int h, f32x16 (&acc)[2][2]) {
    const char *b0 = sB + (wave * 64 + r) * PL_STRIDE;
    const char *a0 = sA + r * PL_STRIDE;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const bf16x8 fb0 = *reinterpret_cast<const bf16x8 *>(b0 + kk * 32 + h * 16);
        const bf16x8 fb1 = *reinterpret_cast<const bf16x8 *>(b0 + 32 * PL_STRIDE + kk * 32 + h * 16);
        const bf16x8 fa0 = *reinterpret_cast<const bf16x8 *>(a0 + kk * 32 + h * 16);
        const bf16x8 fa1 = *reinterpret_cast<const bf16x8 *>(a0 + 32 * PL_STRIDE + kk * 32 + h * 16);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb0, fa0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb0, fa1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb1, fa0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb1, fa1, acc[1][1], 0, 0, 0);
    }
}

__global__ void __launch_bounds__(256, 2) gemm_nt_ln_bwd_add_kernel(const bf16_t *__restrict__ A, int lda, const bf16_t *__restrict__ Bt, int ldb,
                                                                    const bf16_t *__restrict__ x, const float *__restrict__ stats,
                                                                    const float *__restrict__ gamma, const bf16_t *__restrict__ res, int ld_res,
                                                                    bf16_t *__restrict__ dx, int M, int N, int K, float *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *sA = smem, *sB = smem + PL_TM * PL_STRIDE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const bool mma_on = wave * 64 < N;           // (wave-uniform) a wave whose 64 columns lie behind N has nothing to multiply
    // epilogue chunk q of this thread: row (tid >> 5) + 8 q of the tile, columns 8 (tid & 31) ...
    const int part = tid & 31, col = part * 8;
    float gm[8], pg[8], pb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) gm[k] = pg[k] = pb[k] = 0.f;
    if (col < N) Vec8<float>::load(gamma + col, gm);
    const float inv_d = 1.0f / (float)N;
    const int nk = (K + 63) / 64;
    for (int64_t m0 = (int64_t)blockIdx.x * PL_TM; m0 < M; m0 += (int64_t)gridDim.x * PL_TM) {
        f32x16 acc[2][2];     // acc[j][i]: rows = n (tile j of the wave's 64 columns), col = m (tile i of the 64 rows)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int t = 0; t < 16; ++t) acc[i][j][t] = 0.f;
        u32x4 xa[2], xb[8];
        pl_load_a(A, lda, m0, M, 0, K, tid, xa);
        pl_load_b(Bt, ldb, N, 0, K, tid, xb);
        pl_store<2>(sA, tid, xa);
        pl_store<8>(sB, tid, xb);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const bool more = kt + 1 < nk;
            if (more) {
                pl_load_a(A, lda, m0, M, (kt + 1) * 64, K, tid, xa);
                pl_load_b(Bt, ldb, N, (kt + 1) * 64, K, tid, xb);
            }
            if (mma_on) pl_mma_stage(sB, sA, wave, r, h, acc);
            __syncthreads();
            if (more) {
                pl_store<2>(sA, tid, xa);
                pl_store<8>(sB, tid, xb);
                __syncthreads();
            }
        }
        // acc[j][i] register t: n = wave*64 + j*32 + (t&3) + 8*(t>>2) + 4*h, m = i*32 + r  ->  LDS [m][n] bf16
        if (mma_on) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int tq = 0; tq < 4; ++tq) {
                        typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
                        bf16x4_t w;
#pragma unroll
                        for (int k = 0; k < 4; ++k) w[k] = (bf16_t)acc[j][i][4 * tq + k];
                        *reinterpret_cast<bf16x4_t *>(smem + (i * 32 + r) * PL_OUT_STRIDE + (wave * 64 + j * 32 + 8 * tq + 4 * h) * 2) = w;
                    }
        }
        __syncthreads();
#pragma unroll 2
        for (int q = 0; q < 8; ++q) {
            const int row = (tid >> 5) + 8 * q;
            const int64_t grow = m0 + row;
            const bool on = grow < M && col < N;     // rows are uniform over their 32 lanes
            float gv[8], xh[8];
            float s1 = 0.f, s2 = 0.f, rstd = 0.f;
            if (on) {
                const u32x2 lo = *reinterpret_cast<const u32x2 *>(smem + row * PL_OUT_STRIDE + part * 16);
                const u32x2 hi = *reinterpret_cast<const u32x2 *>(smem + row * PL_OUT_STRIDE + part * 16 + 8);
                const u32x4 w4 = {lo[0], lo[1], hi[0], hi[1]};
                const bf16x8 cv = __builtin_bit_cast(bf16x8, w4);      // the bf16 dn that b4c_gemm_nt would have stored
                float zz[8];
                Vec8<bf16_t>::load(x + grow * N + col, zz);
                const float mean = stats[grow * 2];
                rstd = stats[grow * 2 + 1];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float go = (float)cv[k];
                    xh[k] = (zz[k] - mean) * rstd;
                    gv[k] = go * gm[k];
                    s1 += gv[k];
                    s2 += gv[k] * xh[k];
                    pg[k] += go * xh[k];
                    pb[k] += go;
                }
            }
            s1 = group_sum<32>(s1) * inv_d;
            s2 = group_sum<32>(s2) * inv_d;
            if (on) {
                float o[8], rr[8];
                Vec8<bf16_t>::load(res + grow * ld_res + col, rr);
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = rstd * (gv[k] - s1 - xh[k] * s2);
                {
#pragma clang fp contract(off)
#pragma unroll
                    for (int k = 0; k < 8; ++k) o[k] = rr[k] + o[k];
                }
                Vec8<bf16_t>::store(dx + grow * N + col, o);
            }
        }
        __syncthreads();          // the staged rows are read: the next tile's operands may overwrite them
    }
    // the threads' dgamma / dbeta sums meet in a fixed order: LDS [row group][2][N], summed group by group -> partial[block][2][N]
    float *red = reinterpret_cast<float *>(smem);
    float *mine = red + (tid >> 5) * 2 * N;
    if (col < N) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { mine[col + k] = pg[k]; mine[N + col + k] = pb[k]; }
    }
    __syncthreads();
    for (int i = tid; i < 2 * N; i += 256) {
        float sum = 0.f;
        for (int grp = 0; grp < 8; ++grp) sum += red[grp * 2 * N + i];
        partial[(int64_t)blockIdx.x * 2 * N + i] = sum;
    }
}

extern "C" int64_t b4c_gemm_nt_ln_bwd_add_workspace_bytes(int M, int N) {
    if (M <= 0 || N <= 0) return 0;
    return (int64_t)PL_MAX_GRID * 2 * N * 4;
}

extern "C" int b4c_gemm_nt_ln_bwd_add(const void *A, int lda, const void *Bt, int ldb, const void *x, const float *stats,
                                      const float *gamma, const void *res, int ld_res, void *dx, float *dgamma, float *dbeta, int M,
                                      int N, int K, void *workspace, int64_t workspace_bytes, int dtype, void *stream) {
    B4C_REQUIRE(A && Bt && x && stats && gamma && res && dx && dgamma && dbeta, "gemm_nt_ln_bwd_add: null pointer");
    B4C_REQUIRE(dtype == B4C_BF16, "gemm_nt_ln_bwd_add: bf16 only (dtype %d)", dtype);
    B4C_REQUIRE(M > 0 && N > 0 && N <= PL_TN && N % 8 == 0 && K > 0 && K % 8 == 0,
                "gemm_nt_ln_bwd_add: M=%d N=%d K=%d (N <= 256, N, K %% 8 == 0)", M, N, K);
    B4C_REQUIRE(lda >= K && ldb >= K && lda % 8 == 0 && ldb % 8 == 0 && ld_res >= N && ld_res % 8 == 0,
                "gemm_nt_ln_bwd_add: pitches lda=%d ldb=%d ld_res=%d (multiples of 8, lda, ldb >= K, ld_res >= N)", lda, ldb, ld_res);
    B4C_REQUIRE((int64_t)(lda > ldb ? lda : ldb) * 128 * 2 < (1ll << 30),
                "gemm_nt_ln_bwd_add: lda=%d / ldb=%d: a 128-row tile of an operand must span less than 2^30 bytes", lda, ldb);
    B4C_REQUIRE(((((uintptr_t)A | (uintptr_t)Bt | (uintptr_t)x | (uintptr_t)res | (uintptr_t)dx | (uintptr_t)gamma) & 15) == 0),
                "gemm_nt_ln_bwd_add: operands must be 16-byte aligned");
    B4C_REQUIRE(workspace && workspace_bytes >= b4c_gemm_nt_ln_bwd_add_workspace_bytes(M, N), "gemm_nt_ln_bwd_add: workspace too small");
    int64_t tiles = ((int64_t)M + PL_TM - 1) / PL_TM;
    const int grid = (int)(tiles < PL_MAX_GRID ? tiles : PL_MAX_GRID);
    hipStream_t st = (hipStream_t)stream;
    gemm_nt_ln_bwd_add_kernel<<<grid, 256, PL_STAGE_BYTES, st>>>((const bf16_t *)A, lda, (const bf16_t *)Bt, ldb, (const bf16_t *)x, stats,
                                                                 gamma, (const bf16_t *)res, ld_res, (bf16_t *)dx, M, N, K,
                                                                 (float *)workspace);
    ln_bwd_reduce_kernel<<<(2 * N + 3) / 4, 256, 0, st>>>((const float *)workspace, grid, N, dgamma, dbeta);
    return b4c_check_launch("gemm_nt_ln_bwd_add");
}
