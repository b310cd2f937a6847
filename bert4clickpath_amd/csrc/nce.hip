// In-batch contrastive loss (NT-Xent / InfoNCE over the rows of a batch): b4c_nce_fwd / b4c_nce_bwd of include/b4c.h, whose
// comment is the definition.  The [N, N] scores never reach memory.
//
// bf16: one matrix-core kernel per direction (nce_mfma_kernel).  A workgroup of 4 waves owns 32 query rows (query i = the lane's
// column r, both halves hf); the operand fragments of z_i stay in registers for the whole sweep.  The 128-row column tiles of z
// come in by LDS-DMA (VTile::dma), double-buffered: s_waitcnt vmcnt(0) + a barrier before a tile is read, nothing hand-counted.
// Wave w takes the 32-key block w of every tile (N / 32 workgroups of 4 waves: one wave per SIMD of the whole device at N = 8192;
// with a wave per query block and all keys, a 128-row tile kept three quarters of the device idle).  The block's scores S^T[j][i]
// sit in one accumulator (keys j on the registers, rowmap); the forward keeps a max-shifted (m, l) per lane, the backward turns
// the block into the coefficients (G_ij + G_ji) rnorm_j, repacks them as the B operand (pack8) and multiplies by z_j^T read
// transposed from the same LDS image (frag_tr2): dz^T[d][i] accumulates over the wave's blocks in ascending order.  At the end the
// four waves' partial results meet in LDS and wave 0 adds them in wave order: no atomics, an order that depends on N alone.
// Per-column scalars {pos, group, rnorm, lse} travel beside the tile as one 16-byte entry per key.
// fp32: a plain wave-per-row kernel (nce_row_kernel), the parity path.
#include <float.h>
#include <math.h>

#include "mfma.h"

#define NCE_DMA_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define NCE_NEG (-3.0e38f)          // "no key yet": finite, so that exp(m - m') never sees inf - inf

struct NceArgs {
    const void *z;
    const int32_t *pos, *group;
    const float *rnorm, *lse, *gscale;
    float *lse_out, *item_loss;
    void *dz;
    float inv_temp;
    int ld_z, ld_dz, N, K, cosine;
};

// pos[i] when row i is live, else -1
__device__ __forceinline__ int nce_live_pos(const int32_t *__restrict__ pos, int i, int N) {
    const int p = pos[i];
    return (p >= 0 && p < N && p != i) ? p : -1;
}
// key(i, j) and key(j, i) of the definition from the two rows' scalars (pi, pj: nce_live_pos; gi, gj: group or -1);
// ne: i != j, j_is_pi: j == pi, i_is_pj: i == pj
__device__ __forceinline__ void nce_keys(bool ne, bool j_is_pi, bool i_is_pj, int pi, int pj, int gi, int gj, bool &kij, bool &kji) {
    const bool gok = gi < 0 || gj < 0 || gi != gj;
    kij = ne && pi >= 0 && (j_is_pi || (pj >= 0 && gok));
    kji = ne && pj >= 0 && (i_is_pj || (pi >= 0 && gok));
}

// rnorm[i] = 1 / max(||z_i||, 1e-12): one wave per row
template <typename T>
__global__ void __launch_bounds__(64) nce_rnorm_kernel(const T *__restrict__ z, int ld_z, int K, float *__restrict__ rnorm) {
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    float ss = 0.f;
    if (lane * 8 < K) {
        float v[8];
        Vec8<T>::load(z + i * ld_z + lane * 8, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) ss += v[k] * v[k];
    }
    ss = wave_sum(ss);
    if (lane == 0) rnorm[i] = 1.f / fmaxf(sqrtf(ss), 1e-12f);
}

// ---- bf16: the matrix-core sweep ------------------------------------------------------------------------------------------
template <int KD, bool BWD>
__global__ void __launch_bounds__(256, 2) nce_mfma_kernel(NceArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NKS = KD / 16, NDT = KD / 32, STR = VTile<KD>::STR, TILE_B = VTile<KD>::BYTES;
    u32x4 *sMeta = reinterpret_cast<u32x4 *>(smem + 2 * TILE_B);      // [2][128] {pos (live) or -1, group or -1, rnorm, lse}
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hf = lane >> 5, li = lane & 15, g = lane >> 4;
    const bf16_t *__restrict__ z = reinterpret_cast<const bf16_t *>(a.z);
    const int N = a.N, K = a.K;
    const int nct = (N + 127) >> 7;
    const int i = blockIdx.x * 32 + r;                       // the lane's query row (the same 32 rows in all four waves)

    bf16x8 zi[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        u32x4 q = {0u, 0u, 0u, 0u};
        if (i < N && ks * 16 + hf * 8 < K) q = *reinterpret_cast<const u32x4 *>(z + (int64_t)i * a.ld_z + ks * 16 + hf * 8);
        zi[ks] = __builtin_bit_cast(bf16x8, q);
    }
    int pos_i = -1, g_i = -1;
    float rn_i = 1.f, lse_i = 0.f;
    if (i < N) {
        pos_i = nce_live_pos(a.pos, i, N);
        if (a.group) g_i = a.group[i];
        if (a.cosine) rn_i = a.rnorm[i];
        if (BWD) lse_i = a.lse[i];
    }
    int foff[NKS], toff[NDT][2];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) foff[ks] = VTile<KD>::frag_off(r, ks, hf);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
        toff[dt][0] = VTile<KD>::tr_off(hf, li, g, dt, 0);
        toff[dt][1] = VTile<KD>::tr_off(hf, li, g, dt, 1);
    }

    u32x4 mreg = {0u, 0u, 0u, 0u};
    auto fetch = [&](int ct, int buf) {
        VTile<KD>::template dma<256>(z, a.ld_z, (int64_t)ct * 128, ct < nct ? N : 0, smem + buf * TILE_B, tid);
        if (tid < 128) {
            const int j = ct * 128 + tid;
            int pj = -1, gj = -1;
            float rnj = 0.f, lsej = 0.f;
            if (ct < nct && j < N) {
                pj = nce_live_pos(a.pos, j, N);
                if (a.group) gj = a.group[j];
                rnj = a.cosine ? a.rnorm[j] : 1.f;
                if (BWD) lsej = a.lse[j];
            }
            mreg = (u32x4){(unsigned)pj, (unsigned)gj, __float_as_uint(rnj), __float_as_uint(lsej)};
        }
    };
    fetch(0, 0);
    if (tid < 128) sMeta[tid] = mreg;
    NCE_DMA_WAIT();
    __syncthreads();

    float m_run = NCE_NEG, l_run = 0.f, s_pos = 0.f;      // forward: the lane's share of row i (its half of the keys)
    constexpr int NDZ = BWD ? NDT : 1;
    f32x16 dZ[NDZ];                                       // backward: dz^T[d = 32 dt + rowmap(t, hf)][i]
#pragma unroll
    for (int dt = 0; dt < NDZ; ++dt)
#pragma unroll
        for (int t = 0; t < 16; ++t) dZ[dt][t] = 0.f;

    auto tile = [&](auto BUF, int ct) {
        constexpr int buf = decltype(BUF)::value;
        const char *hh = smem + buf * TILE_B;
        const char *ml = reinterpret_cast<const char *>(sMeta + buf * 128) + 4 * hf * 16;
        fetch(ct + 1, buf ^ 1);        // the other buffer was last read one tile ago (behind the previous barrier)
        {
            const int jb = wave;       // the wave's 32-key block of the tile
            f32x16 acc;
#pragma unroll
            for (int t = 0; t < 16; ++t) acc[t] = 0.f;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                // every k-step of the template's width runs; a 16-byte chunk behind K (whatever the pitch holds there) is zeroed
                // in both operands, zi above and the key's here
                u32x4 q = *reinterpret_cast<const u32x4 *>(hh + jb * 32 * STR + foff[ks]);
                if (ks * 16 + hf * 8 >= K) q = (u32x4){0u, 0u, 0u, 0u};
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, q), zi[ks], acc, 0, 0, 0);
            }
            // the lane's row and its positive relative to this block's first key of the lane's half: compared with the
            // register's constant offset below (compared as i == j, the 64 differences are loop invariants the compiler keeps live)
            const int jbase = ct * 128 + jb * 32 + 4 * hf;
            int di = i - jbase, dp = pos_i >= 0 ? pos_i - jbase : -1;
            asm volatile("" : "+v"(di), "+v"(dp));
            float w[16];
            float bm = NCE_NEG;
            bool onehot = false;      // backward: this block holds the lane's positive, or a row whose positive the lane is
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int jo = (t & 3) + 8 * (t >> 2);
                const u32x4 mj = *reinterpret_cast<const u32x4 *>(ml + (jb * 32 + jo) * 16);      // broadcast
                const int pj = (int)mj[0], gj = (int)mj[1];
                const float s = acc[t] * (rn_i * __uint_as_float(mj[2])) * a.inv_temp;
                const bool j_is_pi = dp == jo, i_is_pj = pj == i;      // (pj = -1 when j is not live: never i)
                bool kij, kji;
                nce_keys(di != jo, j_is_pi, i_is_pj, pos_i, pj, g_i, gj, kij, kji);
                if (!BWD) {
                    if (j_is_pi) s_pos += s;
                    acc[t] = kij ? s : -INFINITY;      // (exp(-inf - mn) = 0: mn is finite, NCE_NEG at the least)
                    bm = fmaxf(bm, acc[t]);
                } else {
                    const float gij = (kij ? __expf(s - lse_i) : 0.f) - (j_is_pi ? 1.f : 0.f);
                    const float gji = (kji ? __expf(s - __uint_as_float(mj[3])) : 0.f) - (i_is_pj ? 1.f : 0.f);
                    w[t] = (gij + gji) * __uint_as_float(mj[2]);
                    onehot = onehot || j_is_pi || i_is_pj;
                }
            }
            if (!BWD) {
                const float mn = fmaxf(m_run, bm);
                float add = 0.f;
#pragma unroll
                for (int t = 0; t < 16; ++t) add += __expf(acc[t] - mn);
                l_run = l_run * __expf(m_run - mn) + add;
                m_run = mn;
            } else {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const bf16x8 pf = pack8(w + 8 * s2);
                    const char *hb = hh + (jb * 32 + 16 * s2) * STR;
#pragma unroll
                    for (int dt = 0; dt < NDT; ++dt) {
                        // z^T[d = 32 dt + r][keys 16 s2 + 4 hf + {0..3, 8..11} of this 32-key block]; a row d >= K holds whatever
                        // the pitch does and reaches only row d of dZ, which is never stored
                        const bf16x8 ztf = frag_tr2(hb + toff[dt][0], hb + toff[dt][1]);
                        dZ[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ztf, pf, dZ[dt], 0, 0, 0);
                    }
                }
                // The -[j == pos[i]] terms make a coefficient of size 1 .. 2 out of probabilities of size 1 / N, and its bf16
                // rounding (2^-9 of 2) would be the largest error of the row's gradient.  The few blocks that hold such a term
                // (wave-uniform test) add the product with the rounding residual: there the coefficient carries 16 bits.
                if (__any(onehot)) {
#pragma unroll
                    for (int t = 0; t < 16; ++t) w[t] -= (float)(bf16_t)w[t];
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        const bf16x8 pf = pack8(w + 8 * s2);
                        const char *hb = hh + (jb * 32 + 16 * s2) * STR;
#pragma unroll
                        for (int dt = 0; dt < NDT; ++dt) {
                            const bf16x8 ztf = frag_tr2(hb + toff[dt][0], hb + toff[dt][1]);
                            dZ[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ztf, pf, dZ[dt], 0, 0, 0);
                        }
                    }
                }
            }
        }
        if (tid < 128) sMeta[(buf ^ 1) * 128 + tid] = mreg;
        NCE_DMA_WAIT();
        B4C_LDS_BARRIER();
    };
    for (int ct = 0; ct < nct; ct += 2) {
        tile(std::integral_constant<int, 0>{}, ct);
        if (ct + 1 < nct) tile(std::integral_constant<int, 1>{}, ct + 1);
    }

    // ---- the four waves' partial results -> LDS (the tile buffers: every DMA has landed behind the last barrier) -> wave 0 ----
    float *sRed = reinterpret_cast<float *>(smem);
    if (!BWD) {
        sRed[(wave * 3 + 0) * 64 + lane] = m_run;
        sRed[(wave * 3 + 1) * 64 + lane] = l_run;
        sRed[(wave * 3 + 2) * 64 + lane] = s_pos;
        __syncthreads();
        if (wave == 0 && hf == 0 && i < N) {
            // row i's keys are split over 4 waves x 2 halves: the 8 shares in a fixed order
            float M = NCE_NEG;
#pragma unroll
            for (int e = 0; e < 8; ++e) M = fmaxf(M, sRed[((e >> 1) * 3 + 0) * 64 + 32 * (e & 1) + r]);
            float Lsum = 0.f, sp = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int o = 32 * (e & 1) + r;
                Lsum += sRed[((e >> 1) * 3 + 1) * 64 + o] * __expf(sRed[((e >> 1) * 3 + 0) * 64 + o] - M);
                sp += sRed[((e >> 1) * 3 + 2) * 64 + o];
            }
            const bool live = pos_i >= 0;
            const float lse = live ? M + __logf(Lsum) : 0.f;
            a.lse_out[i] = lse;
            a.item_loss[i] = live ? lse - sp : 0.f;
        }
    } else {
        if (wave > 0) {
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int t = 0; t < 16; ++t) sRed[((wave - 1) * NDT * 16 + dt * 16 + t) * 64 + lane] = dZ[dt][t];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 0; w < 3; ++w)
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int t = 0; t < 16; ++t) dZ[dt][t] += sRed[(w * NDT * 16 + dt * 16 + t) * 64 + lane];
        const float gs = a.gscale[0] * a.inv_temp;
        bf16_t *__restrict__ dz = reinterpret_cast<bf16_t *>(a.dz);
        float zh[NDT][16];
        float dot = 0.f;
        if (a.cosine) {
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int tq = 0; tq < 4; ++tq) {
                    const int d0 = dt * 32 + 8 * tq + 4 * hf;
                    bf16x4 q = {(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
                    if (i < N && d0 < K) q = *reinterpret_cast<const bf16x4 *>(z + (int64_t)i * a.ld_z + d0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        zh[dt][4 * tq + e] = (float)q[e] * rn_i;
                        if (d0 < K) dot += zh[dt][4 * tq + e] * (dZ[dt][4 * tq + e] * gs);
                    }
                }
            dot += __shfl_xor(dot, 32);
        }
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int tq = 0; tq < 4; ++tq) {
                const int d0 = dt * 32 + 8 * tq + 4 * hf;
                if (i < N && d0 < K) {
                    bf16x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v = dZ[dt][4 * tq + e] * gs;
                        if (a.cosine) v = rn_i * (v - zh[dt][4 * tq + e] * dot);
                        o[e] = (bf16_t)v;
                    }
                    *reinterpret_cast<bf16x4 *>(dz + (int64_t)i * a.ld_dz + d0) = o;
                }
            }
    }
}

// ---- fp32: one wave per row -----------------------------------------------------------------------------------------------
// Forward: lane = key j (64 at a time), the dot product against z_i in LDS.  Backward: the 64 coefficients of a key block go
// through LDS, then lane = column d (d, d + 64) adds w_j z_j[d] for the block's keys in ascending order (coalesced rows).
template <bool BWD>
__global__ void __launch_bounds__(64) nce_row_kernel(NceArgs a) {
    __shared__ __attribute__((aligned(16))) float zi[128];
    __shared__ float wj[64];
    const int i = blockIdx.x, lane = threadIdx.x, N = a.N, K = a.K;
    const float *__restrict__ z = reinterpret_cast<const float *>(a.z);
    const int pos_i = nce_live_pos(a.pos, i, N);
    const int g_i = a.group ? a.group[i] : -1;
    const float rn_i = a.cosine ? a.rnorm[i] : 1.f;
    if (!BWD && pos_i < 0) {      // block-uniform
        if (lane == 0) { a.lse_out[i] = 0.f; a.item_loss[i] = 0.f; }
        return;
    }
    for (int k = lane; k < K; k += 64) zi[k] = z[(int64_t)i * a.ld_z + k];
    __syncthreads();
    const float lse_i = BWD ? a.lse[i] : 0.f;
    float m_run = NCE_NEG, l_run = 0.f, s_pos = 0.f, acc0 = 0.f, acc1 = 0.f;
    for (int j0 = 0; j0 < N; j0 += 64) {
        const int j = j0 + lane;
        float w = 0.f;
        if (j < N) {
            const float *zj = z + (int64_t)j * a.ld_z;
            float dotv = 0.f;
            for (int k = 0; k < K; k += 4) {
                const f32x4 q = *reinterpret_cast<const f32x4 *>(zj + k);
                const f32x4 p = *reinterpret_cast<const f32x4 *>(zi + k);
                dotv += p[0] * q[0];
                dotv += p[1] * q[1];
                dotv += p[2] * q[2];
                dotv += p[3] * q[3];
            }
            const int pj = nce_live_pos(a.pos, j, N), gj = a.group ? a.group[j] : -1;
            const float rnj = a.cosine ? a.rnorm[j] : 1.f;
            const float s = dotv * (rn_i * rnj) * a.inv_temp;
            bool kij, kji;
            nce_keys(i != j, j == pos_i, i == pj, pos_i, pj, g_i, gj, kij, kji);
            if (!BWD) {
                if (kij) {
                    const float mn = fmaxf(m_run, s);
                    l_run = l_run * __expf(m_run - mn) + __expf(s - mn);
                    m_run = mn;
                }
                if (j == pos_i) s_pos = s;
            } else {
                const float gij = (kij ? __expf(s - lse_i) : 0.f) - (j == pos_i ? 1.f : 0.f);
                const float gji = (kji ? __expf(s - a.lse[j]) : 0.f) - ((pj >= 0 && i == pj) ? 1.f : 0.f);
                w = (gij + gji) * rnj;
            }
        }
        if (BWD) {
            wj[lane] = w;
            __syncthreads();
            const int jn = N - j0 < 64 ? N - j0 : 64;
            for (int jj = 0; jj < jn; ++jj) {
                const float wv = wj[jj];
                const float *zj = z + (int64_t)(j0 + jj) * a.ld_z;
                if (lane < K) acc0 += wv * zj[lane];
                if (lane + 64 < K) acc1 += wv * zj[lane + 64];
            }
            __syncthreads();
        }
    }
    if (!BWD) {
        const float M = wave_max(m_run);
        const float L = wave_sum(l_run * __expf(m_run - M));
        const float sp = wave_sum(s_pos);
        if (lane == 0) {
            const float lse = M + __logf(L);
            a.lse_out[i] = lse;
            a.item_loss[i] = lse - sp;
        }
    } else {
        const float gs = a.gscale[0] * a.inv_temp;
        float v0 = acc0 * gs, v1 = acc1 * gs;
        if (a.cosine) {
            const float h0 = lane < K ? zi[lane] * rn_i : 0.f, h1 = lane + 64 < K ? zi[lane + 64] * rn_i : 0.f;
            const float dot = wave_sum(h0 * v0 + h1 * v1);
            v0 = rn_i * (v0 - h0 * dot);
            v1 = rn_i * (v1 - h1 * dot);
        }
        float *__restrict__ dz = reinterpret_cast<float *>(a.dz) + (int64_t)i * a.ld_dz;
        if (lane < K) dz[lane] = v0;
        if (lane + 64 < K) dz[lane + 64] = v1;
    }
}

// ---- entry points ---------------------------------------------------------------------------------------------------------
// the checks of the header comment that need no pointer
static int nce_check_scalars(const char *who, int64_t N, int K, int dtype, float inv_temp, uint32_t flags) {
    B4C_REQUIRE(K >= 8 && K <= 128 && K % 8 == 0, "%s: K = %d (a multiple of 8, 8 .. 128)", who, K);
    B4C_REQUIRE(dtype == B4C_F32 || dtype == B4C_BF16, "%s: dtype %d (B4C_F32 or B4C_BF16)", who, dtype);
    B4C_REQUIRE(inv_temp > 0.f && inv_temp <= FLT_MAX, "%s: inv_temp = %g (finite, > 0)", who, (double)inv_temp);
    B4C_REQUIRE((flags & ~B4C_NCE_COSINE) == 0, "%s: flags 0x%x (B4C_NCE_COSINE is the one bit)", who, flags);
    B4C_REQUIRE(N >= 0 && N < B4C_NCE_MAX_N, "%s: N = %lld (0 .. 2^24 - 1)", who, (long long)N);
    return B4C_OK;
}
// a [N][ld] operand of dtype: pitch, 16-byte alignment, the tile loader's 32-bit offsets
static int nce_check_rows(const char *who, const char *name, const void *p, int ld, int K, int dtype) {
    B4C_REQUIRE(ld >= K && ld <= (1 << 21), "%s: ld_%s = %d (K = %d .. 2^21)", who, name, ld, K);
    B4C_REQUIRE(((uintptr_t)p & 15) == 0 && ld % (dtype == B4C_F32 ? 4 : 8) == 0, "%s: %s must be 16-byte aligned, rows included (ld_%s = %d)",
                who, name, name, ld);
    return B4C_OK;
}

template <bool BWD> static void nce_launch(const NceArgs &a, int dtype, hipStream_t st) {
    if (dtype == B4C_F32) {
        nce_row_kernel<BWD><<<(unsigned)a.N, 64, 0, st>>>(a);
        return;
    }
    const unsigned grid = (unsigned)((a.N + 31) / 32);
    if (a.K <= 64) {
        const size_t lds = 2 * VTile<64>::BYTES + 2 * 128 * 16;
        b4c_allow_lds(nce_mfma_kernel<64, BWD>, lds);
        nce_mfma_kernel<64, BWD><<<grid, 256, lds, st>>>(a);
    } else {
        const size_t lds = 2 * VTile<128>::BYTES + 2 * 128 * 16;
        b4c_allow_lds(nce_mfma_kernel<128, BWD>, lds);
        nce_mfma_kernel<128, BWD><<<grid, 256, lds, st>>>(a);
    }
}

extern "C" int b4c_nce_fwd(const void *z, int ld_z, int64_t N, int K, int dtype, const int32_t *pos, const int32_t *group, float inv_temp,
                           uint32_t flags, float *rnorm, float *lse, float *item_loss, void *stream) {
    int rc = nce_check_scalars("nce_fwd", N, K, dtype, inv_temp, flags);
    if (rc != B4C_OK) return rc;
    if (N == 0) return B4C_OK;
    B4C_REQUIRE(rnorm || !(flags & B4C_NCE_COSINE), "nce_fwd: B4C_NCE_COSINE without rnorm");
    B4C_REQUIRE(z && pos && lse && item_loss, "nce_fwd: null pointer (z, pos, lse or item_loss)");
    rc = nce_check_rows("nce_fwd", "z", z, ld_z, K, dtype);
    if (rc != B4C_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int cosine = (flags & B4C_NCE_COSINE) ? 1 : 0;
    if (cosine) {
        if (dtype == B4C_F32) nce_rnorm_kernel<float><<<(unsigned)N, 64, 0, st>>>((const float *)z, ld_z, K, rnorm);
        else nce_rnorm_kernel<bf16_t><<<(unsigned)N, 64, 0, st>>>((const bf16_t *)z, ld_z, K, rnorm);
        rc = b4c_check_launch("nce_fwd (rnorm)");
        if (rc != B4C_OK) return rc;
    }
    NceArgs a = {};
    a.z = z; a.pos = pos; a.group = group; a.rnorm = rnorm; a.lse_out = lse; a.item_loss = item_loss;
    a.inv_temp = inv_temp; a.ld_z = ld_z; a.N = (int)N; a.K = K; a.cosine = cosine;
    nce_launch<false>(a, dtype, st);
    return b4c_check_launch("nce_fwd");
}

extern "C" int b4c_nce_bwd(const void *z, int ld_z, int64_t N, int K, int dtype, const int32_t *pos, const int32_t *group, float inv_temp,
                           uint32_t flags, const float *rnorm, const float *lse, const float *gscale, void *dz, int ld_dz, void *stream) {
    int rc = nce_check_scalars("nce_bwd", N, K, dtype, inv_temp, flags);
    if (rc != B4C_OK) return rc;
    if (N == 0) return B4C_OK;
    B4C_REQUIRE(rnorm || !(flags & B4C_NCE_COSINE), "nce_bwd: B4C_NCE_COSINE without rnorm");
    B4C_REQUIRE(z && pos && lse && gscale && dz, "nce_bwd: null pointer (z, pos, lse, gscale or dz)");
    rc = nce_check_rows("nce_bwd", "z", z, ld_z, K, dtype);
    if (rc != B4C_OK) return rc;
    rc = nce_check_rows("nce_bwd", "dz", dz, ld_dz, K, dtype);
    if (rc != B4C_OK) return rc;
    NceArgs a = {};
    a.z = z; a.pos = pos; a.group = group; a.rnorm = rnorm; a.lse = lse; a.gscale = gscale; a.dz = dz;
    a.inv_temp = inv_temp; a.ld_z = ld_z; a.ld_dz = ld_dz; a.N = (int)N; a.K = K; a.cosine = (flags & B4C_NCE_COSINE) ? 1 : 0;
    nce_launch<true>(a, dtype, (hipStream_t)stream);
    return b4c_check_launch("nce_bwd");
}
