// Sampled-negative training (include/b4c.h): the loss of each row over its own candidate
// list -- target in column 0; SASRec's binary cross-entropy (its target term weighted by beta: gBCE), the list-wise softmax or BPR,
// over scores that a per-item correction (logQ) may shift -- and its backward into dh and the row-sparse fp32 gradient sinks.
//
// One wave per row as its own 64-thread workgroup, as in candidates.hip: rows share nothing.  Both kernels read the fp32 MASTER
// table at the listed rows (for bf16 h each element is rounded to bf16 first: the value the packed copy would hold), so nothing
// is repacked and the row-lazy optimizer only has to bring the listed rows up to date.  The forward is a gather (C rows of K
// floats per row of h) with FP32 FMAs on the VALU; the backward gathers the same rows once more for dh and adds C rows of K
// floats into the table's gradient with float atomics: its floor is the chip-wide atomic rate.
#include "common.h"
#include <cfloat>

template <typename T> __device__ __forceinline__ float cl_operand(float w) { return w; }
template <> __device__ __forceinline__ float cl_operand<bf16_t>(float w) { return (float)(bf16_t)w; }

// A table row of K floats is nch = K / 8 chunks of 8 (two 16-byte loads).  G lanes (a power of two >= nch, at most 64) share one
// list position, each with NC chunks (NC = 2 only for K > 512), so one wave-instruction gathers from 64 / G rows; U such groups
// of positions are loaded before any is used.  (The lane layout of cand_score_kernel.)
template <typename T, int G, int NC>
__device__ __forceinline__ void cl_load_row(const float *__restrict__ table, int ld_t, int64_t row_off, int id, int sub, int nch,
                                            float (&w)[NC][8]) {
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const int ch = sub + q * G;
        if (id >= 0 && ch < nch) {
            Vec8<float>::load(table + (row_off + id) * (int64_t)ld_t + ch * 8, w[q]);
#pragma unroll
            for (int e = 0; e < 8; ++e) w[q][e] = cl_operand<T>(w[q][e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) w[q][e] = 0.f;
        }
    }
}

template <typename T, int G, int NC, int U>
__global__ void __launch_bounds__(64) cand_loss_fwd_kernel(const T *__restrict__ h, int ld_h, const float *__restrict__ table, int ld_t,
                                                           int64_t row_off, const float *__restrict__ bias,
                                                           const int32_t *__restrict__ cand, int ld_c, int C, int V, int K, int kind,
                                                           float beta, const float *__restrict__ corr, int flags,
                                                           float *__restrict__ item_loss, float *__restrict__ g, int ld_g,
                                                           float *__restrict__ scores, int ld_s) {
    extern __shared__ int cl_lds[];
    float *sv = reinterpret_cast<float *>(cl_lds);      // [C] corrected scores z of the list (z = s without corr)
    int *si = cl_lds + C;                               // [C] ids, -1 where absent
    constexpr int PER = 64 / G;
    const int lane = threadIdx.x, sub = lane % G, slot = lane / G;
    const int64_t row = blockIdx.x;
    const int nch = K >> 3;
    const int32_t *cr = cand + row * (int64_t)ld_c;
    float *gr = g + row * (int64_t)ld_g;
    float *sr = scores ? scores + row * (int64_t)ld_s : nullptr;
    const int y = cr[0];
    if (y < 0 || y >= V) {                              // ignored row: nothing is read, nothing is owed
        for (int p = lane; p < C; p += 64) {
            gr[p] = 0.f;
            if (sr) sr[p] = __builtin_nanf("");
        }
        if (lane == 0) item_loss[row] = 0.f;
        return;
    }
    const T *hr = h + row * (int64_t)ld_h;
    float hv[NC][8];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const int ch = sub + q * G;
        if (ch < nch) Vec8<T>::load(hr + ch * 8, hv[q]);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) hv[q][e] = 0.f;
        }
    }
    for (int p0 = 0; p0 < C; p0 += PER * U) {
        int id[U];
        float w[U][NC][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + u * PER + slot;
            const int c = p < C ? cr[p] : -1;
            id[u] = (c >= 0 && c < V) ? c : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cl_load_row<T, G, NC>(table, ld_t, row_off, id[u], sub, nch, w[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float acc = 0.f;
#pragma unroll
            for (int q = 0; q < NC; ++q)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc = fmaf(hv[q][e], w[u][q][e], acc);
            acc = group_sum<G>(acc);
            const int p = p0 + u * PER + slot;
            if (sub == 0 && p < C) {
                const float s = id[u] >= 0 ? acc + bias[id[u]] : __builtin_nanf("");
                sv[p] = s;
                si[p] = id[u];
                if (sr) sr[p] = s;
            }
        }
    }
    __syncthreads();
    if (corr) {
        // z = s - corr[id]: one fp32 subtraction on the stored score, after the gather (inside it, next to the bias load, the
        // K = 128 bf16 form needs 66 VGPRs and drops to 7 waves / SIMD; here every form keeps the registers it had -- DESIGN.md)
        const int first = (flags & B4C_CANDX_CORR_TARGET) ? 0 : 1;
        for (int p = lane; p < C; p += 64)
            if (p >= first && si[p] >= 0) sv[p] -= corr[si[p]];
        __syncthreads();
    }
    float loss;
    if (kind == B4C_CANDX_BCE) {
        // the target's term is beta * softplus(-z_0) with coefficient -(beta * sigma(-z_0)): one form, x = -z at the target.
        // (beta == 1: the products are exact, the bits of b4c_candidate_loss_fwd)
        float l = 0.f;
        for (int p = lane; p < C; p += 64) {
            float gc = 0.f;
            if (si[p] >= 0) {
                const float x = p == 0 ? -sv[p] : sv[p];
                const float e = expf(-fabsf(x));
                const float t = fmaxf(x, 0.f) + log1pf(e);
                const float sig = (x >= 0.f ? 1.f : e) / (1.f + e);
                l += p == 0 ? beta * t : t;
                gc = p == 0 ? -(beta * sig) : sig;
            }
            gr[p] = gc;
        }
        loss = wave_sum(l);
    } else if (kind == B4C_CANDX_BPR) {
        // every present negative against the target: softplus(z_c - z_0); the target's coefficient is minus the sum of the others'
        const float z0 = sv[0];
        float l = 0.f, gsum = 0.f;
        for (int p = lane; p < C; p += 64) {
            if (p == 0) continue;
            float gc = 0.f;
            if (si[p] >= 0) {
                const float x = sv[p] - z0;
                const float e = expf(-fabsf(x));
                l += fmaxf(x, 0.f) + log1pf(e);
                gc = (x >= 0.f ? 1.f : e) / (1.f + e);
                gsum += gc;
            }
            gr[p] = gc;
        }
        loss = wave_sum(l);
        gsum = wave_sum(gsum);
        if (lane == 0) gr[0] = 0.f - gsum;                  // no present negative: 0 - 0, and the loss is the empty sum
    } else {
        float m = -__builtin_inff();
        for (int p = lane; p < C; p += 64)
            if (si[p] >= 0) m = fmaxf(m, sv[p]);
        m = wave_max(m);
        float sum = 0.f;
        for (int p = lane; p < C; p += 64)
            if (si[p] >= 0) sum += expf(sv[p] - m);
        sum = wave_sum(sum);
        loss = (m - sv[0]) + logf(sum);                  // C == 1: m = s_0 and sum = 1, so 0 + 0
        for (int p = lane; p < C; p += 64) gr[p] = si[p] >= 0 ? expf(sv[p] - m) / sum - (p == 0 ? 1.f : 0.f) : 0.f;
    }
    if (lane == 0) item_loss[row] = loss;
}

template <typename T, int G, int NC, int U>
__global__ void __launch_bounds__(64) cand_loss_bwd_kernel(const T *__restrict__ h, int ld_h, const float *__restrict__ table, int ld_t,
                                                           int64_t row_off, const int32_t *__restrict__ cand, int ld_c,
                                                           const float *__restrict__ g, int ld_g, const float *__restrict__ gscale,
                                                           int C, int V, int K, T *__restrict__ dh, int ld_dh,
                                                           float *__restrict__ dtable, int ld_dt, float *__restrict__ dbias) {
    extern __shared__ int cl_lds[];
    float *sg = reinterpret_cast<float *>(cl_lds);      // [C] gs * g
    int *si = cl_lds + C;                               // [C] ids, -1 where the entry adds nothing (absent, or gs * g == 0)
    float *sh = reinterpret_cast<float *>(cl_lds + 2 * C);   // [K] the h row in fp32
    constexpr int PER = 64 / G;
    const int lane = threadIdx.x, sub = lane % G, slot = lane / G;
    const int64_t row = blockIdx.x;
    const int nch = K >> 3;
    const int32_t *cr = cand + row * (int64_t)ld_c;
    T *dr = dh + row * (int64_t)ld_dh;
    const int y = cr[0];
    if (y < 0 || y >= V) {                              // ignored row: dh = 0, no add anywhere
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int ch = lane; ch < nch; ch += 64) Vec8<T>::store(dr + ch * 8, z);
        return;
    }
    const float gs = gscale[0];
    const float *gr = g + row * (int64_t)ld_g;
    for (int p = lane; p < C; p += 64) {                // (dbias: R C floats in all, 1 / K of the table's adds)
        const int c = cr[p];
        const float gc = (c >= 0 && c < V) ? gs * gr[p] : 0.f;
        sg[p] = gc;
        si[p] = gc != 0.f ? c : -1;
        if (gc != 0.f) atomicAdd(dbias + c, gc);
    }
    const T *hr = h + row * (int64_t)ld_h;
    for (int ch = lane; ch < nch; ch += 64) {
        float v[8];
        Vec8<T>::load(hr + ch * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) sh[ch * 8 + e] = v[e];
    }
    __syncthreads();
    // dh: the forward's gather; every lane sums its chunks over the positions of its slot, then the slots are summed
    float acc[NC][8];
#pragma unroll
    for (int q = 0; q < NC; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[q][e] = 0.f;
    for (int p0 = 0; p0 < C; p0 += PER * U) {
        int id[U];
        float gc[U];
        float w[U][NC][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + u * PER + slot;
            id[u] = p < C ? si[p] : -1;
            gc[u] = id[u] >= 0 ? sg[p] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cl_load_row<T, G, NC>(table, ld_t, row_off, id[u], sub, nch, w[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < NC; ++q)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[q][e] = fmaf(gc[u], w[u][q][e], acc[q][e]);
    }
#pragma unroll
    for (int o = G; o < 64; o <<= 1)
#pragma unroll
        for (int q = 0; q < NC; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[q][e] += __shfl_xor(acc[q][e], o);
    if (slot == 0) {
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const int ch = sub + q * G;
            if (ch < nch) Vec8<T>::store(dr + ch * 8, acc[q]);
        }
    }
    // dtable: lane = column, so every atomic wave-instruction is up to 256 contiguous bytes of ONE table row
    for (int p = 0; p < C; ++p) {
        const int id = si[p];
        if (id < 0) continue;
        const float gc = sg[p];
        float *drow = dtable + (row_off + id) * (int64_t)ld_dt;
        for (int k = lane; k < K; k += 64) atomicAdd(drow + k, gc * sh[k]);
    }
}

// ---- entry points ---------------------------------------------------------------------------------------------------------
// f(G, NC) for the lane layout of a row of nch chunks
template <typename F> static void cl_by_chunks(int nch, F &&f) {
    using one = std::integral_constant<int, 1>;
    if (nch <= 1) f(one{}, one{});
    else if (nch <= 2) f(std::integral_constant<int, 2>{}, one{});
    else if (nch <= 4) f(std::integral_constant<int, 4>{}, one{});
    else if (nch <= 8) f(std::integral_constant<int, 8>{}, one{});
    else if (nch <= 16) f(std::integral_constant<int, 16>{}, one{});
    else if (nch <= 32) f(std::integral_constant<int, 32>{}, one{});
    else if (nch <= 64) f(std::integral_constant<int, 64>{}, one{});
    else f(std::integral_constant<int, 64>{}, std::integral_constant<int, 2>{});
}
template <int G> constexpr int cl_unroll() { return G >= 16 ? 4 : (G >= 4 ? 2 : 1); }

// the checks the two entry points share: shapes, the table, the list, h and its alignment
static int cl_check(const char *who, const void *h, int ld_h, const float *table, int ld_t, int64_t rows, int64_t row_off,
                    const int32_t *cand, int ld_c, int64_t R, int C, int V, int K, int dtype) {
    B4C_REQUIRE(R >= 0 && R <= 0x7fffffff && V > 0 && C >= 1 && C <= B4C_MAX_CAND, "%s: R = %lld, V = %d, C = %d (1 .. %d)", who,
                (long long)R, V, C, B4C_MAX_CAND);
    B4C_REQUIRE(K >= 8 && K <= 1024 && K % 8 == 0, "%s: K = %d (a multiple of 8, 8 .. 1024)", who, K);
    B4C_REQUIRE(dtype == B4C_F32 || dtype == B4C_BF16, "%s: dtype %d", who, dtype);
    B4C_REQUIRE(h && table && cand, "%s: null pointer (h, table or cand)", who);
    B4C_REQUIRE(ld_h >= K && ld_c >= C && ld_t >= K, "%s: a pitch below its width (ld_h = %d, ld_t = %d for K = %d; ld_c = %d for C = %d)",
                who, ld_h, ld_t, K, ld_c, C);
    B4C_REQUIRE(row_off >= 0 && row_off + V <= rows, "%s: rows %lld .. %lld of a table of %lld rows", who, (long long)row_off,
                (long long)(row_off + V), (long long)rows);
    const int he = dtype == B4C_F32 ? 4 : 8;      // elements of h per 16 bytes
    B4C_REQUIRE(((uintptr_t)h & 15) == 0 && ld_h % he == 0 && ((uintptr_t)table & 15) == 0 && ld_t % 4 == 0,
                "%s: h and table must be 16-byte aligned, rows included (ld_h = %d, ld_t = %d)", who, ld_h, ld_t);
    return B4C_OK;
}

// the one forward launch of both entry points; lds = 8 C bytes
static_assert(B4C_CAND_BCE == B4C_CANDX_BCE && B4C_CAND_SOFTMAX == B4C_CANDX_SOFTMAX, "the extended kinds continue the first two");
static void cl_launch_fwd(const void *h, int ld_h, const float *table, int ld_t, int64_t row_off, const float *bias, const int32_t *cand,
                          int ld_c, int64_t R, int C, int V, int K, int dtype, int kind, float beta, const float *corr, int flags,
                          float *item_loss, float *g, int ld_g, float *scores, int ld_s, hipStream_t st) {
    const size_t lds = (size_t)C * 8;
    cl_by_chunks(K / 8, [&](auto G, auto NC) {
        constexpr int U = cl_unroll<G()>();
        if (dtype == B4C_F32)
            cand_loss_fwd_kernel<float, G(), NC(), U><<<(unsigned)R, 64, lds, st>>>((const float *)h, ld_h, table, ld_t, row_off, bias, cand,
                                                                                  ld_c, C, V, K, kind, beta, corr, flags, item_loss, g,
                                                                                  ld_g, scores, ld_s);
        else
            cand_loss_fwd_kernel<bf16_t, G(), NC(), U><<<(unsigned)R, 64, lds, st>>>((const bf16_t *)h, ld_h, table, ld_t, row_off, bias, cand,
                                                                                   ld_c, C, V, K, kind, beta, corr, flags, item_loss, g,
                                                                                   ld_g, scores, ld_s);
    });
}

extern "C" int b4c_candidate_loss_fwd(const void *h, int ld_h, const float *table, int ld_t, int64_t rows, int64_t row_off,
                                      const float *bias, const int32_t *cand, int ld_c, int64_t R, int C, int V, int K, int dtype,
                                      int kind, float *item_loss, float *g, int ld_g, float *scores, int ld_s, void *stream) {
    const int rc = cl_check("candidate_loss_fwd", h, ld_h, table, ld_t, rows, row_off, cand, ld_c, R, C, V, K, dtype);
    if (rc != B4C_OK) return rc;
    B4C_REQUIRE(kind >= 0 && kind < B4C_CAND_KINDS, "candidate_loss_fwd: kind %d (B4C_CAND_BCE, B4C_CAND_SOFTMAX)", kind);
    B4C_REQUIRE(bias && item_loss && g, "candidate_loss_fwd: null pointer (bias, item_loss or g)");
    B4C_REQUIRE(ld_g >= C && (!scores || ld_s >= C), "candidate_loss_fwd: ld_g = %d or ld_s = %d below C = %d", ld_g, ld_s, C);
    if (R == 0) return B4C_OK;
    // (B4C_CAND_BCE / _SOFTMAX are B4C_CANDX_BCE / _SOFTMAX; beta = 1, no correction: the kernel's products by beta are exact)
    cl_launch_fwd(h, ld_h, table, ld_t, row_off, bias, cand, ld_c, R, C, V, K, dtype, kind, 1.f, nullptr, 0, item_loss, g, ld_g, scores,
                  ld_s, (hipStream_t)stream);
    return b4c_check_launch("candidate_loss_fwd");
}

extern "C" int b4c_candidate_loss_fwd_ex(const void *h, int ld_h, const float *table, int ld_t, int64_t rows, int64_t row_off,
                                         const float *bias, const int32_t *cand, int ld_c, int64_t R, int C, int V, int K, int dtype,
                                         int kind, float beta, const float *corr, int flags, float *item_loss, float *g, int ld_g,
                                         float *scores, int ld_s, void *stream) {
    const int rc = cl_check("candidate_loss_fwd_ex", h, ld_h, table, ld_t, rows, row_off, cand, ld_c, R, C, V, K, dtype);
    if (rc != B4C_OK) return rc;
    B4C_REQUIRE(kind >= 0 && kind < B4C_CANDX_KINDS, "candidate_loss_fwd_ex: kind %d (B4C_CANDX_BCE, B4C_CANDX_SOFTMAX, B4C_CANDX_BPR)",
                kind);
    B4C_REQUIRE((flags & ~B4C_CANDX_CORR_TARGET) == 0, "candidate_loss_fwd_ex: flags 0x%x (B4C_CANDX_CORR_TARGET is the one bit)", flags);
    B4C_REQUIRE(corr || !(flags & B4C_CANDX_CORR_TARGET), "candidate_loss_fwd_ex: B4C_CANDX_CORR_TARGET without corr");
    B4C_REQUIRE(beta >= 0.f && beta <= FLT_MAX, "candidate_loss_fwd_ex: beta = %g (finite, >= 0)", (double)beta);
    B4C_REQUIRE(bias && item_loss && g, "candidate_loss_fwd_ex: null pointer (bias, item_loss or g)");
    B4C_REQUIRE(ld_g >= C && (!scores || ld_s >= C), "candidate_loss_fwd_ex: ld_g = %d or ld_s = %d below C = %d", ld_g, ld_s, C);
    if (R == 0) return B4C_OK;
    cl_launch_fwd(h, ld_h, table, ld_t, row_off, bias, cand, ld_c, R, C, V, K, dtype, kind, beta, corr, flags, item_loss, g, ld_g, scores,
                  ld_s, (hipStream_t)stream);
    return b4c_check_launch("candidate_loss_fwd_ex");
}

extern "C" int b4c_candidate_loss_bwd(const void *h, int ld_h, const float *table, int ld_t, int64_t rows, int64_t row_off,
                                      const int32_t *cand, int ld_c, const float *g, int ld_g, const float *gscale, int64_t R, int C,
                                      int V, int K, int dtype, void *dh, int ld_dh, float *dtable, int ld_dt, float *dbias,
                                      void *stream) {
    const int rc = cl_check("candidate_loss_bwd", h, ld_h, table, ld_t, rows, row_off, cand, ld_c, R, C, V, K, dtype);
    if (rc != B4C_OK) return rc;
    B4C_REQUIRE(g && gscale && dh && dtable && dbias, "candidate_loss_bwd: null pointer (g, gscale, dh, dtable or dbias)");
    B4C_REQUIRE(ld_g >= C && ld_dh >= K && ld_dt >= K, "candidate_loss_bwd: a pitch below its width (ld_g = %d for C = %d; ld_dh = %d, "
                "ld_dt = %d for K = %d)", ld_g, C, ld_dh, ld_dt, K);
    B4C_REQUIRE(((uintptr_t)dh & 15) == 0 && ld_dh % (dtype == B4C_F32 ? 4 : 8) == 0,
                "candidate_loss_bwd: dh must be 16-byte aligned, rows included (ld_dh = %d)", ld_dh);
    if (R == 0) return B4C_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)C * 8 + (size_t)K * 4;
    cl_by_chunks(K / 8, [&](auto G, auto NC) {
        constexpr int U = cl_unroll<G()>();
        if (dtype == B4C_F32)
            cand_loss_bwd_kernel<float, G(), NC(), U><<<(unsigned)R, 64, lds, st>>>((const float *)h, ld_h, table, ld_t, row_off, cand, ld_c, g,
                                                                                  ld_g, gscale, C, V, K, (float *)dh, ld_dh, dtable, ld_dt,
                                                                                  dbias);
        else
            cand_loss_bwd_kernel<bf16_t, G(), NC(), U><<<(unsigned)R, 64, lds, st>>>((const bf16_t *)h, ld_h, table, ld_t, row_off, cand, ld_c,
                                                                                   g, ld_g, gscale, C, V, K, (bf16_t *)dh, ld_dh, dtable,
                                                                                   ld_dt, dbias);
    });
    return b4c_check_launch("candidate_loss_bwd");
}
