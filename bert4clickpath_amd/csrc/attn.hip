// Multi-head self-attention with a key-side padding mask (reference: transformer.py:64-97,
// 130-156).  qkv rows are [q | k | v] blocks of d_model columns; head h owns columns
// [h*dh, (h+1)*dh) of each block, so no split_heads / merge transposes ever touch HBM.
//
// "row" kernels (this file, both dtypes, fp32 math): one thread owns one query (forward, dQ)
// or one key (dK/dV); the other side streams through LDS in 64-row tiles and is read with
// wave-uniform (broadcast) ds_read_b128.  Scores never leave registers; softmax is online in
// forward and recomputed from the saved log-sum-exp in backward.  These are the exact fp32
// parity kernels; the bf16 MFMA kernels (attn_mfma.hip) replace them on the throughput path.
#include <math.h>

#include "common.h"

#define ATT_TILE 64

// stage rows [r0, r0+64) x DH columns starting at column col0 of a [B*S][ld] matrix into fp32 LDS
template <typename T, int DH>
__device__ __forceinline__ void stage_tile(const T *__restrict__ base, int ld, int64_t tok0, int r0, int S, int col0,
                                           float (*s)[DH], int tid) {
    constexpr int CPR = DH / 8;
    for (int c = tid; c < ATT_TILE * CPR; c += 256) {
        const int row = c / CPR, part = c % CPR;
        float t[8];
        if (r0 + row < S) Vec8<T>::load(base + (tok0 + r0 + row) * ld + col0 + part * 8, t);
        else {
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) s[row][part * 8 + k] = t[k];
    }
}

// DROP (all three kernels): attention-probability dropout by the keep rule of common.h (b4c_attn_keep); q and k are the positions,
// the pitch is S.  The DROP = false instantiations are the kernels without it.
// CAUSAL (all three kernels; the CAUSAL = false instantiations are the kernels without it): key k is visible to query q iff k <= q.
// The key loop (forward, dQ) or the query loop (dK / dV) is clamped at the diagonal: per workgroup for the staging (every thread
// takes part in it), per thread for the arithmetic.  The dropout keep rule is untouched.
template <typename T, int DH, bool DROP, bool CAUSAL>
__global__ void __launch_bounds__(256) attn_fwd_row_kernel(const T *__restrict__ qkv, int ld, const uint8_t *__restrict__ key_pad,
                                                           T *__restrict__ o, int ld_o, float *__restrict__ lse, int S, int H,
                                                           float sqrt_dk, float rate, uint64_t seed) {
    __shared__ __attribute__((aligned(16))) float sK[ATT_TILE][DH];
    __shared__ __attribute__((aligned(16))) float sV[ATT_TILE][DH];
    __shared__ uint8_t sPad[ATT_TILE];
    const int tid = threadIdx.x;
    const int b = blockIdx.y / H, h = blockIdx.y % H, dm = H * DH;
    const int64_t tok0 = (int64_t)b * S;
    const int qi = blockIdx.x * 256 + tid;
    const bool active = qi < S;
    float q[DH], acc[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) { q[d] = 0.f; acc[d] = 0.f; }
    if (active) load_row<T, DH>(qkv + (tok0 + qi) * ld + h * DH, q);
    float m = -INFINITY, l = 0.f;
    const uint32_t thr = DROP ? b4c_keep_threshold(rate) : 0u;
    const uint64_t drow = (uint64_t)blockIdx.y * S + (uint32_t)qi;
    uint32_t kb = 0;
    const int k_end = CAUSAL ? min(S, (int)blockIdx.x * 256 + 256) : S;      // past the workgroup's last query nothing is visible
    for (int k0 = 0; k0 < k_end; k0 += ATT_TILE) {
        __syncthreads();
        stage_tile<T, DH>(qkv, ld, tok0, k0, S, dm + h * DH, sK, tid);
        stage_tile<T, DH>(qkv, ld, tok0, k0, S, 2 * dm + h * DH, sV, tid);
        if (tid < ATT_TILE) sPad[tid] = (k0 + tid < S) ? key_pad[tok0 + k0 + tid] : 1;
        __syncthreads();
        if (!active) continue;
        const int nk = CAUSAL ? min(ATT_TILE, qi + 1 - k0) : min(ATT_TILE, S - k0);
        for (int j = 0; j < nk; ++j) {
            float s = dot_lds<DH>(q, &sK[j][0]) / sqrt_dk;
            if (sPad[j]) s += -1e9f;
            if (s > m) {
                const float corr = expf(m - s);
                l *= corr;
#pragma unroll
                for (int d = 0; d < DH; ++d) acc[d] *= corr;
                m = s;
            }
            const float p = expf(s - m);
            l += p;
            if (DROP) {      // l keeps the undropped sum; 1 / (1 - rate) joins the final 1 / l.  One hash per four keys.
                if ((j & 3) == 0) kb = b4c_attn_keep4(seed, b4c_attn_ctr(drow, k0 + j, S), thr);
                if (!((kb >> (j & 3)) & 1u)) continue;
            }
#pragma unroll
            for (int d = 0; d < DH; d += 4) {
                const f32x4 vv = *reinterpret_cast<const f32x4 *>(&sV[j][d]);
                acc[d] += p * vv[0];
                acc[d + 1] += p * vv[1];
                acc[d + 2] += p * vv[2];
                acc[d + 3] += p * vv[3];
            }
        }
    }
    if (active) {
        const float inv = DROP ? (1.0f / (1.0f - rate)) / l : 1.0f / l;
#pragma unroll
        for (int d = 0; d < DH; ++d) acc[d] *= inv;
        store_row<T, DH>(o + (tok0 + qi) * ld_o + h * DH, acc);
        if (lse) lse[((int64_t)b * H + h) * S + qi] = m + logf(l);
    }
}

// dQ: thread per query; also writes delta[q] = sum_d dO[q][d] * O[q][d]
template <typename T, int DH, bool DROP, bool CAUSAL>
__global__ void __launch_bounds__(256) attn_bwd_dq_kernel(const T *__restrict__ qkv, int ld, const uint8_t *__restrict__ key_pad,
                                                          const T *__restrict__ o, int ld_o, const T *__restrict__ d_o, int ld_do,
                                                          const float *__restrict__ lse, float *__restrict__ delta,
                                                          T *__restrict__ dqkv, int ld_dq, int S, int H, float sqrt_dk, float rate,
                                                          uint64_t seed) {
    __shared__ __attribute__((aligned(16))) float sK[ATT_TILE][DH];
    __shared__ __attribute__((aligned(16))) float sV[ATT_TILE][DH];
    __shared__ uint8_t sPad[ATT_TILE];
    const int tid = threadIdx.x;
    const int b = blockIdx.y / H, h = blockIdx.y % H, dm = H * DH;
    const int64_t tok0 = (int64_t)b * S;
    const int qi = blockIdx.x * 256 + tid;
    const bool active = qi < S;
    float q[DH], g[DH], dq[DH];
    float dlt = 0.f, L = 0.f;
#pragma unroll
    for (int d = 0; d < DH; ++d) { q[d] = 0.f; g[d] = 0.f; dq[d] = 0.f; }
    if (active) {
        load_row<T, DH>(qkv + (tok0 + qi) * ld + h * DH, q);
        load_row<T, DH>(d_o + (tok0 + qi) * ld_do + h * DH, g);
        float ov[DH];
        load_row<T, DH>(o + (tok0 + qi) * ld_o + h * DH, ov);
#pragma unroll
        for (int d = 0; d < DH; ++d) dlt += g[d] * ov[d];
        L = lse[((int64_t)b * H + h) * S + qi];
        delta[((int64_t)b * H + h) * S + qi] = dlt;
    }
    const uint32_t thr = DROP ? b4c_keep_threshold(rate) : 0u;
    const float inv_keep = DROP ? 1.0f / (1.0f - rate) : 1.0f;
    const uint64_t drow = (uint64_t)blockIdx.y * S + (uint32_t)qi;
    uint32_t kb = 0;
    const int k_end = CAUSAL ? min(S, (int)blockIdx.x * 256 + 256) : S;
    for (int k0 = 0; k0 < k_end; k0 += ATT_TILE) {
        __syncthreads();
        stage_tile<T, DH>(qkv, ld, tok0, k0, S, dm + h * DH, sK, tid);
        stage_tile<T, DH>(qkv, ld, tok0, k0, S, 2 * dm + h * DH, sV, tid);
        if (tid < ATT_TILE) sPad[tid] = (k0 + tid < S) ? key_pad[tok0 + k0 + tid] : 1;
        __syncthreads();
        if (!active) continue;
        const int nk = CAUSAL ? min(ATT_TILE, qi + 1 - k0) : min(ATT_TILE, S - k0);
        for (int j = 0; j < nk; ++j) {
            if (DROP && (j & 3) == 0) kb = b4c_attn_keep4(seed, b4c_attn_ctr(drow, k0 + j, S), thr);
            if (sPad[j]) continue;  // p == 0 exactly (exp(-1e9 - lse))
            const float s = dot_lds<DH>(q, &sK[j][0]) / sqrt_dk;
            const float p = expf(s - L);
            float dp = dot_lds<DH>(g, &sV[j][0]);
            if (DROP) dp = ((kb >> (j & 3)) & 1u) ? dp * inv_keep : 0.f;     // dP = keep / (1 - rate) * dP~
            const float ds = p * (dp - dlt);
#pragma unroll
            for (int d = 0; d < DH; d += 4) {
                const f32x4 kv = *reinterpret_cast<const f32x4 *>(&sK[j][d]);
                dq[d] += ds * kv[0];
                dq[d + 1] += ds * kv[1];
                dq[d + 2] += ds * kv[2];
                dq[d + 3] += ds * kv[3];
            }
        }
    }
    if (active) {
#pragma unroll
        for (int d = 0; d < DH; ++d) dq[d] /= sqrt_dk;
        store_row<T, DH>(dqkv + (tok0 + qi) * ld_dq + h * DH, dq);
    }
}

// dK, dV: thread per key; queries (q, dO, lse, delta) stream through LDS
template <typename T, int DH, bool DROP, bool CAUSAL>
__global__ void __launch_bounds__(256) attn_bwd_dkv_kernel(const T *__restrict__ qkv, int ld, const uint8_t *__restrict__ key_pad,
                                                           const T *__restrict__ d_o, int ld_do, const float *__restrict__ lse,
                                                           const float *__restrict__ delta, T *__restrict__ dqkv, int ld_dq, int S,
                                                           int H, float sqrt_dk, float rate, uint64_t seed) {
    __shared__ __attribute__((aligned(16))) float sQ[ATT_TILE][DH];
    __shared__ __attribute__((aligned(16))) float sG[ATT_TILE][DH];
    __shared__ float sL[ATT_TILE], sD[ATT_TILE];
    const int tid = threadIdx.x;
    const int b = blockIdx.y / H, h = blockIdx.y % H, dm = H * DH;
    const int64_t tok0 = (int64_t)b * S;
    const int kj = blockIdx.x * 256 + tid;
    const bool inrange = kj < S;
    const bool active = inrange && !key_pad[tok0 + kj];
    float k[DH], v[DH], dk[DH], dv[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) { k[d] = 0.f; v[d] = 0.f; dk[d] = 0.f; dv[d] = 0.f; }
    if (active) {
        load_row<T, DH>(qkv + (tok0 + kj) * ld + dm + h * DH, k);
        load_row<T, DH>(qkv + (tok0 + kj) * ld + 2 * dm + h * DH, v);
    }
    for (int q0 = CAUSAL ? (int)blockIdx.x * 256 : 0; q0 < S; q0 += ATT_TILE) {      // CAUSAL: no query before the workgroup's first key sees it
        __syncthreads();
        stage_tile<T, DH>(qkv, ld, tok0, q0, S, h * DH, sQ, tid);
        stage_tile<T, DH>(d_o, ld_do, tok0, q0, S, h * DH, sG, tid);
        if (tid < ATT_TILE) {
            const bool ok = q0 + tid < S;
            sL[tid] = ok ? lse[((int64_t)b * H + h) * S + q0 + tid] : 0.f;
            sD[tid] = ok ? delta[((int64_t)b * H + h) * S + q0 + tid] : 0.f;
        }
        __syncthreads();
        if (!active) continue;
        const int nq = min(ATT_TILE, S - q0);
        for (int i = CAUSAL ? max(0, kj - q0) : 0; i < nq; ++i) {
            const float s = dot_lds<DH>(k, &sQ[i][0]) / sqrt_dk;
            const float p = expf(s - sL[i]);
            float dp = dot_lds<DH>(v, &sG[i][0]);
            float pd = p;           // what dV sums: the dropped, rescaled P~
            if (DROP) {
                // one hash per (query, key): the thread owns ONE key of the four a hash covers (the exact-parity path, not the
                // throughput path)
                const float kf = b4c_keep_elem(seed, ((uint64_t)blockIdx.y * S + (uint32_t)(q0 + i)) * b4c_attn_s4(S) + (uint32_t)kj, rate)
                                     ? 1.0f / (1.0f - rate) : 0.f;
                pd = p * kf;
                dp *= kf;
            }
            const float ds = p * (dp - sD[i]);
#pragma unroll
            for (int d = 0; d < DH; d += 4) {
                const f32x4 gv = *reinterpret_cast<const f32x4 *>(&sG[i][d]);
                const f32x4 qv = *reinterpret_cast<const f32x4 *>(&sQ[i][d]);
                dv[d] += pd * gv[0];
                dv[d + 1] += pd * gv[1];
                dv[d + 2] += pd * gv[2];
                dv[d + 3] += pd * gv[3];
                dk[d] += ds * qv[0];
                dk[d + 1] += ds * qv[1];
                dk[d + 2] += ds * qv[2];
                dk[d + 3] += ds * qv[3];
            }
        }
    }
    if (inrange) {
#pragma unroll
        for (int d = 0; d < DH; ++d) dk[d] /= sqrt_dk;
        store_row<T, DH>(dqkv + (tok0 + kj) * ld_dq + dm + h * DH, dk);
        store_row<T, DH>(dqkv + (tok0 + kj) * ld_dq + 2 * dm + h * DH, dv);
    }
}

// bf16 MFMA forward/backward (attn_mfma.hip); return B4C_EUNSUPPORTED when the shape is not covered.
int b4c_attn_fwd_mfma(const void *qkv, int ld_qkv, const uint8_t *key_pad, void *o, int ld_o, float *lse, int B, int S,
                      int H, int dh, const int32_t *cu, float rate, uint64_t seed, bool causal, hipStream_t st);
int b4c_attn_bwd_mfma(const void *qkv, int ld_qkv, const uint8_t *key_pad, const void *o, int ld_o, const void *d_o,
                      int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv, int B, int S, int H, int dh,
                      void *workspace, int64_t workspace_bytes, const int32_t *cu, float rate, uint64_t seed, bool causal,
                      hipStream_t st);
int64_t b4c_attn_bwd_mfma_workspace_bytes(int B, int S, int H, int dh);

// bf16 shapes the MFMA kernels do not cover (S > 512 or head depth 16 / 128) run on the fp32-math row kernels, which are
// several times slower: say so once per process instead of degrading silently.
static void note_row_fallback(const char *who, int S, int dh) {
    static bool said = false;
    if (said) return;
    said = true;
    fprintf(stderr, "[b4c] %s: bf16 attention with S=%d, head depth %d is outside the MFMA kernels (S <= 512, depth 32 / 64); "
                    "using the fp32-math row kernels (exact, several times slower).  This notice is printed once.\n", who, S, dh);
}

static int check_attn(const char *who, int ld_qkv, int ld_o, int B, int S, int H, int dh) {
    B4C_REQUIRE(B > 0 && S > 0 && H > 0 && dh > 0, "%s: bad shape", who);
    B4C_REQUIRE(dh == 16 || dh == 32 || dh == 64 || dh == 128, "%s: head depth %d not in {16,32,64,128}", who, dh);
    B4C_REQUIRE(ld_qkv >= 3 * H * dh && ld_qkv % 8 == 0 && ld_o >= H * dh && ld_o % 8 == 0, "%s: bad pitch", who);
    B4C_REQUIRE((int64_t)B * H <= 65535, "%s: B*H = %lld exceeds the grid.y limit 65535", who, (long long)B * H);
    return B4C_OK;
}
// the attention-probability dropout rate of the *_drop entry points: [0, 1) (a NaN fails the comparison too)
static int check_attn_rate(const char *who, float rate) {
    B4C_REQUIRE(rate >= 0.f && rate < 1.f, "%s: dropout rate %g outside [0, 1)", who, (double)rate);
    return B4C_OK;
}
static int check_attn_flags(const char *who, uint32_t flags) {
    B4C_REQUIRE((flags & ~B4C_ATTN_CAUSAL) == 0, "%s: unknown flag bits 0x%x", who, flags & ~B4C_ATTN_CAUSAL);
    return B4C_OK;
}

// One host path per direction, behind every entry point below.  cu_seqlens: NULL is the dense layout, S rows per sequence.
// Otherwise the packed (padding-free) layout: sequence b owns rows cu_seqlens[b] .. cu_seqlens[b+1] of qkv / o / d_o / dqkv and S
// is max_len, the longest sequence (LDS sizing, lse / delta pitch: [B][H][max_len]); key_pad [total tokens] is all zeros unless the
// caller keeps masked keys inside the packed rows.  The packed layout exists for the throughput path -- bf16, head depth 32 / 64,
// max_len <= 512, an error outside it --, the fp32 parity path stays dense, and dense bf16 outside the MFMA kernels falls back to
// the row kernels.  rate == 0 selects the DROP = false instantiations, the kernels of the entry points without dropout, and
// !causal the CAUSAL = false ones.
static int attn_fwd_launch(const char *who, const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, void *o,
                           int ld_o, float *lse, int B, int S, int H, int dh, float rate, uint64_t seed, bool causal, int dtype,
                           void *stream) {
    B4C_REQUIRE(qkv && key_pad && o, "%s: null pointer", who);
    int rc = check_attn(who, ld_qkv, ld_o, B, S, H, dh);
    if (rc) return rc;
    B4C_REQUIRE(!cu_seqlens || dtype == B4C_BF16, "%s: bf16 only", who);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == B4C_BF16) {
        rc = b4c_attn_fwd_mfma(qkv, ld_qkv, key_pad, o, ld_o, lse, B, S, H, dh, cu_seqlens, rate, seed, causal, st);
        B4C_REQUIRE(!cu_seqlens || rc != B4C_EUNSUPPORTED, "%s: max_len %d / head depth %d outside the MFMA kernels (<= 512, 32 or 64)", who, S, dh);
        if (rc != B4C_EUNSUPPORTED) return rc;
        note_row_fallback(who, S, dh);
    }
    const float sq = sqrtf((float)dh);
    dim3 grid((S + 255) / 256, B * H);
    auto rows = [&](auto *t) {
        using T = std::remove_pointer_t<decltype(t)>;
        b4c_by_int<16, 32, 64, 128>(dh, [&](auto DH) { b4c_by_bool(rate != 0.f, [&](auto DR) { b4c_by_bool(causal, [&](auto CA) {
            attn_fwd_row_kernel<T, DH(), DR(), CA()><<<grid, 256, 0, st>>>((const T *)qkv, ld_qkv, key_pad, (T *)o, ld_o, lse, S, H, sq, rate, seed);
        }); }); });
    };
    if (dtype == B4C_F32) rows((float *)nullptr);
    else if (dtype == B4C_BF16) rows((bf16_t *)nullptr);
    else B4C_REQUIRE(false, "%s: dtype %d", who, dtype);
    return b4c_check_launch(who);
}

static int attn_bwd_launch(const char *who, const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens,
                           const void *o, int ld_o, const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv,
                           int ld_dqkv, int B, int S, int H, int dh, void *workspace, int64_t workspace_bytes, float rate,
                           uint64_t seed, bool causal, int dtype, void *stream) {
    B4C_REQUIRE(qkv && key_pad && o && d_o && lse && delta && dqkv, "%s: null pointer", who);
    int rc = check_attn(who, ld_qkv, ld_o, B, S, H, dh);
    if (rc) return rc;
    B4C_REQUIRE(!cu_seqlens || dtype == B4C_BF16, "%s: bf16 only", who);
    B4C_REQUIRE(ld_do >= H * dh && ld_do % 8 == 0 && ld_dqkv >= 3 * H * dh && ld_dqkv % 8 == 0, "%s: bad pitch", who);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == B4C_BF16) {
        rc = b4c_attn_bwd_mfma(qkv, ld_qkv, key_pad, o, ld_o, d_o, ld_do, lse, delta, dqkv, ld_dqkv, B, S, H, dh, workspace,
                               workspace_bytes, cu_seqlens, rate, seed, causal, st);
        B4C_REQUIRE(!cu_seqlens || rc != B4C_EUNSUPPORTED, "%s: shape outside the MFMA kernels, or workspace missing for max_len > 256", who);
        if (rc != B4C_EUNSUPPORTED) return rc;
        note_row_fallback(who, S, dh);
    }
    const float sq = sqrtf((float)dh);
    dim3 grid((S + 255) / 256, B * H);
    auto rows = [&](auto *t) {
        using T = std::remove_pointer_t<decltype(t)>;
        b4c_by_int<16, 32, 64, 128>(dh, [&](auto DH) { b4c_by_bool(rate != 0.f, [&](auto DR) { b4c_by_bool(causal, [&](auto CA) {
            attn_bwd_dq_kernel<T, DH(), DR(), CA()><<<grid, 256, 0, st>>>((const T *)qkv, ld_qkv, key_pad, (const T *)o, ld_o, (const T *)d_o, ld_do, lse, delta, (T *)dqkv, ld_dqkv, S, H, sq, rate, seed);
            attn_bwd_dkv_kernel<T, DH(), DR(), CA()><<<grid, 256, 0, st>>>((const T *)qkv, ld_qkv, key_pad, (const T *)d_o, ld_do, lse, delta, (T *)dqkv, ld_dqkv, S, H, sq, rate, seed);
        }); }); });
    };
    if (dtype == B4C_F32) rows((float *)nullptr);
    else if (dtype == B4C_BF16) rows((bf16_t *)nullptr);
    else B4C_REQUIRE(false, "%s: dtype %d", who, dtype);
    return b4c_check_launch(who);
}

extern "C" int64_t b4c_attn_bwd_workspace_bytes(int B, int S, int H, int dh, int dtype) {
    return dtype == B4C_BF16 ? b4c_attn_bwd_mfma_workspace_bytes(B, S, H, dh) : 0;
}

// ---- the entry points of include/b4c.h: each fixes what its name leaves out (dense: no cu_seqlens; no _drop: rate 0; never causal)
// and is otherwise the call above.  A _varlen entry point without cu_seqlens is a null pointer, not a dense launch.
extern "C" int b4c_attn_fwd(const void *qkv, int ld_qkv, const uint8_t *key_pad, void *o, int ld_o, float *lse, int B,
                            int S, int H, int dh, int dtype, void *stream) {
    return attn_fwd_launch("attn_fwd", qkv, ld_qkv, key_pad, nullptr, o, ld_o, lse, B, S, H, dh, 0.f, 0, false, dtype, stream);
}

extern "C" int b4c_attn_fwd_drop(const void *qkv, int ld_qkv, const uint8_t *key_pad, void *o, int ld_o, float *lse, int B,
                                 int S, int H, int dh, int dtype, void *stream, float dropout_rate, uint64_t seed) {
    if (int rc = check_attn_rate("attn_fwd_drop", dropout_rate)) return rc;
    return attn_fwd_launch("attn_fwd_drop", qkv, ld_qkv, key_pad, nullptr, o, ld_o, lse, B, S, H, dh, dropout_rate, seed, false, dtype, stream);
}

extern "C" int b4c_attn_fwd_varlen(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, void *o, int ld_o,
                                   float *lse, int B, int max_len, int H, int dh, int dtype, void *stream) {
    B4C_REQUIRE(cu_seqlens, "attn_fwd_varlen: null pointer");
    return attn_fwd_launch("attn_fwd_varlen", qkv, ld_qkv, key_pad, cu_seqlens, o, ld_o, lse, B, max_len, H, dh, 0.f, 0, false, dtype, stream);
}

extern "C" int b4c_attn_fwd_varlen_drop(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, void *o,
                                        int ld_o, float *lse, int B, int max_len, int H, int dh, int dtype, void *stream,
                                        float dropout_rate, uint64_t seed) {
    if (int rc = check_attn_rate("attn_fwd_varlen_drop", dropout_rate)) return rc;
    B4C_REQUIRE(cu_seqlens, "attn_fwd_varlen_drop: null pointer");
    return attn_fwd_launch("attn_fwd_varlen_drop", qkv, ld_qkv, key_pad, cu_seqlens, o, ld_o, lse, B, max_len, H, dh, dropout_rate, seed,
                           false, dtype, stream);
}

extern "C" int b4c_attn_bwd(const void *qkv, int ld_qkv, const uint8_t *key_pad, const void *o, int ld_o,
                            const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv, int B,
                            int S, int H, int dh, int dtype, void *stream) {
    return b4c_attn_bwd_ws(qkv, ld_qkv, key_pad, o, ld_o, d_o, ld_do, lse, delta, dqkv, ld_dqkv, B, S, H, dh, nullptr, 0, dtype, stream);
}

extern "C" int b4c_attn_bwd_ws(const void *qkv, int ld_qkv, const uint8_t *key_pad, const void *o, int ld_o,
                               const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv, int B,
                               int S, int H, int dh, void *workspace, int64_t workspace_bytes, int dtype, void *stream) {
    return attn_bwd_launch("attn_bwd", qkv, ld_qkv, key_pad, nullptr, o, ld_o, d_o, ld_do, lse, delta, dqkv, ld_dqkv, B, S, H, dh, workspace,
                           workspace_bytes, 0.f, 0, false, dtype, stream);
}

extern "C" int b4c_attn_bwd_drop_ws(const void *qkv, int ld_qkv, const uint8_t *key_pad, const void *o, int ld_o,
                                    const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv, int B,
                                    int S, int H, int dh, void *workspace, int64_t workspace_bytes, int dtype, void *stream,
                                    float dropout_rate, uint64_t seed) {
    if (int rc = check_attn_rate("attn_bwd_drop", dropout_rate)) return rc;
    return attn_bwd_launch("attn_bwd_drop", qkv, ld_qkv, key_pad, nullptr, o, ld_o, d_o, ld_do, lse, delta, dqkv, ld_dqkv, B, S, H, dh,
                           workspace, workspace_bytes, dropout_rate, seed, false, dtype, stream);
}

extern "C" int b4c_attn_bwd_varlen(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, const void *o,
                                   int ld_o, const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv,
                                   int B, int max_len, int H, int dh, void *workspace, int64_t workspace_bytes, int dtype,
                                   void *stream) {
    B4C_REQUIRE(cu_seqlens, "attn_bwd_varlen: null pointer");
    return attn_bwd_launch("attn_bwd_varlen", qkv, ld_qkv, key_pad, cu_seqlens, o, ld_o, d_o, ld_do, lse, delta, dqkv, ld_dqkv, B, max_len,
                           H, dh, workspace, workspace_bytes, 0.f, 0, false, dtype, stream);
}

extern "C" int b4c_attn_bwd_varlen_drop(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, const void *o,
                                        int ld_o, const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv,
                                        int ld_dqkv, int B, int max_len, int H, int dh, void *workspace, int64_t workspace_bytes,
                                        int dtype, void *stream, float dropout_rate, uint64_t seed) {
    if (int rc = check_attn_rate("attn_bwd_varlen_drop", dropout_rate)) return rc;
    B4C_REQUIRE(cu_seqlens, "attn_bwd_varlen_drop: null pointer");
    return attn_bwd_launch("attn_bwd_varlen_drop", qkv, ld_qkv, key_pad, cu_seqlens, o, ld_o, d_o, ld_do, lse, delta, dqkv, ld_dqkv, B,
                           max_len, H, dh, workspace, workspace_bytes, dropout_rate, seed, false, dtype, stream);
}

// ---- one entry point per direction that takes everything (include/b4c.h): layout by cu_seqlens (NULL: dense), dropout by the
// rate, causal masking by flags.  flags == 0 reaches exactly the launches of the entry points above.
extern "C" int b4c_attn_fwd_ex(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, void *o, int ld_o,
                               float *lse, int B, int S, int H, int dh, int dtype, void *stream, float dropout_rate, uint64_t seed,
                               uint32_t flags) {
    if (int rc = check_attn_flags("attn_fwd_ex", flags)) return rc;
    if (int rc = check_attn_rate("attn_fwd_ex", dropout_rate)) return rc;
    return attn_fwd_launch("attn_fwd_ex", qkv, ld_qkv, key_pad, cu_seqlens, o, ld_o, lse, B, S, H, dh, dropout_rate, seed,
                           (flags & B4C_ATTN_CAUSAL) != 0, dtype, stream);
}

extern "C" int b4c_attn_bwd_ex(const void *qkv, int ld_qkv, const uint8_t *key_pad, const int32_t *cu_seqlens, const void *o,
                               int ld_o, const void *d_o, int ld_do, const float *lse, float *delta, void *dqkv, int ld_dqkv,
                               int B, int S, int H, int dh, void *workspace, int64_t workspace_bytes, int dtype, void *stream,
                               float dropout_rate, uint64_t seed, uint32_t flags) {
    if (int rc = check_attn_flags("attn_bwd_ex", flags)) return rc;
    if (int rc = check_attn_rate("attn_bwd_ex", dropout_rate)) return rc;
    return attn_bwd_launch("attn_bwd_ex", qkv, ld_qkv, key_pad, cu_seqlens, o, ld_o, d_o, ld_do, lse, delta, dqkv, ld_dqkv, B, S, H, dh,
                           workspace, workspace_bytes, dropout_rate, seed, (flags & B4C_ATTN_CAUSAL) != 0, dtype, stream);
}

// the keep rule of the *_drop entry points on the host (common.h: b4c_attn_keep_elem)
extern "C" int b4c_attn_keep(uint64_t seed, int b, int h, int q, int k, int H, int S_arg, float rate) {
    return b4c_attn_keep_elem(seed, b, h, q, k, H, S_arg, rate) ? 1 : 0;
}
