// Candidate lists (include/b4c.h, "candidate lists"): the sampler of per-row negatives, and the rank / top-k of a per-row list
// of items, scored here (b4c_candidate_score) or gathered from materialised scores (b4c_candidate_rank_rows).
//
// Every kernel runs one wave per row as its own 64-thread workgroup: rows share no columns, so there is nothing to share
// between waves, and a one-wave barrier costs nothing.  Scoring is batched GEMV work (a row's own h against its own C rows of
// wt): FP32 FMAs on the VALU, bound by the gather of the wt rows (from L2 / the Infinity Cache for a table of a few MB).
#include "common.h"
#include "sampler.h"

__device__ __forceinline__ bool cand_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// ---- scoring --------------------------------------------------------------------------------------------------------------
// A wt row of K elements is nch = K / 8 chunks of 8 (16 B bf16, 32 B fp32).  G lanes (a power of two >= nch, at most 64) share
// one list position, each holding NC chunks of the h row in registers (NC = 2 only for K > 512), so one wave-instruction
// gathers 64 / G rows; U such groups of positions are loaded before any is reduced.  Position C is the label: it goes through
// the same lanes and the same reduction as any listed item, so a listed copy of the label gets the identical score.
template <typename T, int G, int NC, int U>
__global__ void __launch_bounds__(64) cand_score_kernel(const T *__restrict__ h, int ld_h, const T *__restrict__ wt, int ld_w,
                                                        const float *__restrict__ bias, const int32_t *__restrict__ cand, int ld_c,
                                                        int C, int V, int K, const int32_t *__restrict__ labels,
                                                        float *__restrict__ scores, int ld_s, int32_t *__restrict__ rank, int k,
                                                        int32_t *__restrict__ idx, int hb) {
    extern __shared__ int cand_lds[];
    float *sv = reinterpret_cast<float *>(cand_lds);
    int *si = cand_lds + (C + 1);
    int *hk = cand_lds + 2 * (C + 1), *hp = hk + (1 << hb);
    constexpr int PER = 64 / G;
    const int lane = threadIdx.x, sub = lane % G, slot = lane / G;
    const int64_t row = blockIdx.x;
    const int nch = K >> 3;
    const T *hr = h + row * (int64_t)ld_h;
    float hv[NC][8];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const int ch = sub + q * G;
#pragma unroll
        for (int e = 0; e < 8; ++e) hv[q][e] = ch < nch ? (float)hr[ch * 8 + e] : 0.f;
    }
    int y = labels ? labels[row] : -1;
    if (y >= V) y = -1;
    if (y < 0) y = -1;
    const int32_t *cr = cand + row * (int64_t)ld_c;
    const int npos = (y >= 0) ? C + 1 : C;
    for (int p0 = 0; p0 < npos; p0 += PER * U) {
        int id[U];
        float w[U][NC][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + u * PER + slot;
            int c = p < C ? cr[p] : (p == C ? y : -1);
            id[u] = (c >= 0 && c < V) ? c : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const int ch = sub + q * G;
                if (id[u] >= 0 && ch < nch) Vec8<T>::load(wt + (int64_t)id[u] * ld_w + ch * 8, w[u][q]);
                else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) w[u][q][e] = 0.f;
                }
            }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float acc = 0.f;
#pragma unroll
            for (int q = 0; q < NC; ++q)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc = fmaf(hv[q][e], w[u][q][e], acc);
            acc = group_sum<G>(acc);
            const int p = p0 + u * PER + slot;
            if (sub == 0 && p < npos) {
                const float s = id[u] >= 0 ? acc + bias[id[u]] : __builtin_nanf("");
                sv[p] = s;
                si[p] = id[u];
                if (scores && p < C) scores[row * (int64_t)ld_s + p] = s;
            }
        }
    }
    __syncthreads();
    const float sy = y >= 0 ? sv[C] : 0.f;
#include "cand_rank_body.inc"
}

// ---- ranking materialised scores ------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(64) cand_rank_rows_kernel(const T *__restrict__ x, int ld, const int32_t *__restrict__ cand,
                                                            int ld_c, int C, int V, const int32_t *__restrict__ labels,
                                                            int32_t *__restrict__ rank, int k, int32_t *__restrict__ idx,
                                                            int hb) {
    extern __shared__ int cand_lds[];
    float *sv = reinterpret_cast<float *>(cand_lds);
    int *si = cand_lds + C;
    int *hk = cand_lds + 2 * C, *hp = hk + (1 << hb);
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    const T *xr = x + row * (int64_t)ld;
    const int32_t *cr = cand + row * (int64_t)ld_c;
    for (int p = lane; p < C; p += 64) {
        const int c = cr[p];
        const bool ok = c >= 0 && c < V;
        sv[p] = ok ? (float)xr[c] : __builtin_nanf("");
        si[p] = ok ? c : -1;
    }
    int y = labels ? labels[row] : -1;
    if (y >= V) y = -1;
    if (y < 0) y = -1;
    const float sy = y >= 0 ? (float)xr[y] : 0.f;
    __syncthreads();
#include "cand_rank_body.inc"
}

// ---- sampler --------------------------------------------------------------------------------------------------------------
// The row's list is one wave's work (sampler.h); its exclusion list is copied to LDS for the binary search.
__global__ void __launch_bounds__(64) cand_sample_kernel(const int32_t *__restrict__ labels, int V, int N, uint64_t seed,
                                                         int64_t row_base, const int32_t *__restrict__ excl, int ld_e, int E,
                                                         const int64_t *__restrict__ cdf, int32_t *__restrict__ cand, int ld_c,
                                                         int32_t *__restrict__ short_count, int hb) {
    extern __shared__ int cand_lds[];
    int *tab = cand_lds, *sx = cand_lds + (1 << hb);
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    int nx = 0;                                  // canonical list: ascending ids, then -1
    for (int i = lane; i < E; i += 64) {
        const int v = excl[row * (int64_t)ld_e + i];
        sx[i] = v;
        nx += v >= 0 ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nx += __shfl_xor(nx, o);
    const uint64_t total = cdf ? (uint64_t)cdf[V - 1] : 0;
    sampler_wave(sx, nx, tab, hb, labels[row], V, N, seed, (uint64_t)(row_base + row), cdf, total, cand + row * (int64_t)ld_c, short_count,
                 lane);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------
extern "C" int b4c_sample_candidates(const int32_t *labels, int64_t R, int V, int N, uint64_t seed, int64_t row_base,
                                     const int32_t *excl, int ld_e, int E, const int64_t *cdf, int32_t *cand, int ld_c,
                                     int32_t *short_count, void *stream) {
    B4C_REQUIRE(R >= 0 && V > 0 && N >= 0 && N < B4C_MAX_CAND, "sample_candidates: R = %lld, V = %d, N = %d (0 .. %d)",
                (long long)R, V, N, B4C_MAX_CAND - 1);
    B4C_REQUIRE(row_base >= 0 && row_base + R <= ((int64_t)1 << 44), "sample_candidates: row_base %lld", (long long)row_base);
    B4C_REQUIRE(E >= 0 && E <= B4C_MAX_EXCL && (E == 0 || (excl && ld_e >= E)), "sample_candidates: exclusion list (ld_e = %d, E = %d)",
                ld_e, E);
    B4C_REQUIRE(labels && cand && short_count && ld_c >= N + 1, "sample_candidates: null pointer or ld_c < N + 1");
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(short_count, 0, 4, st);
    if (R == 0) return B4C_OK;
    const int hb = sampler_hash_bits(N);
    const size_t lds = (size_t)((1 << hb) + E) * 4;
    cand_sample_kernel<<<(unsigned)R, 64, lds, st>>>(labels, V, N, seed, row_base, excl, ld_e, E, cdf, cand, ld_c, short_count, hb);
    return b4c_check_launch("sample_candidates");
}

template <typename T, int G, int NC>
static void cand_score_launch(const void *h, int ld_h, const void *wt, int ld_w, const float *bias, const int32_t *cand, int ld_c,
                              int64_t R, int C, int V, int K, const int32_t *labels, float *scores, int ld_s, int32_t *rank, int k,
                              int32_t *idx, hipStream_t st) {
    constexpr int U = G >= 16 ? 4 : (G >= 4 ? 2 : 1);
    const int hb = sampler_hash_bits(C);
    const size_t lds = (size_t)(C + 1) * 8 + (rank ? (size_t)8 << hb : 0);
    cand_score_kernel<T, G, NC, U><<<(unsigned)R, 64, lds, st>>>((const T *)h, ld_h, (const T *)wt, ld_w, bias, cand, ld_c, C, V, K,
                                                                 labels, scores, ld_s, rank, k, idx, hb);
}

template <typename T>
static void cand_score_dispatch(const void *h, int ld_h, const void *wt, int ld_w, const float *bias, const int32_t *cand, int ld_c,
                                int64_t R, int C, int V, int K, const int32_t *labels, float *scores, int ld_s, int32_t *rank,
                                int k, int32_t *idx, hipStream_t st) {
    const int nch = K / 8;
#define CAND_L(G, NC) cand_score_launch<T, G, NC>(h, ld_h, wt, ld_w, bias, cand, ld_c, R, C, V, K, labels, scores, ld_s, rank, k, idx, st)
    if (nch <= 1) CAND_L(1, 1);
    else if (nch <= 2) CAND_L(2, 1);
    else if (nch <= 4) CAND_L(4, 1);
    else if (nch <= 8) CAND_L(8, 1);
    else if (nch <= 16) CAND_L(16, 1);
    else if (nch <= 32) CAND_L(32, 1);
    else if (nch <= 64) CAND_L(64, 1);
    else CAND_L(64, 2);
#undef CAND_L
}

extern "C" int b4c_candidate_score(const void *h, int ld_h, const void *wt, int ld_w, const float *bias, const int32_t *cand, int ld_c,
                                   int64_t R, int C, int V, int K, int dtype, const int32_t *labels, float *scores, int ld_s,
                                   int32_t *rank, int k, int32_t *idx, void *stream) {
    B4C_REQUIRE(R >= 0 && V > 0 && C >= 1 && C <= B4C_MAX_CAND, "candidate_score: R = %lld, V = %d, C = %d (1 .. %d)", (long long)R,
                V, C, B4C_MAX_CAND);
    B4C_REQUIRE(K >= 8 && K <= 1024 && K % 8 == 0, "candidate_score: K = %d (a multiple of 8, at most 1024)", K);
    B4C_REQUIRE(dtype == B4C_F32 || dtype == B4C_BF16, "candidate_score: dtype %d", dtype);
    B4C_REQUIRE(h && wt && bias && cand && ld_h >= K && ld_c >= C, "candidate_score: null pointer, ld_h < K or ld_c < C");
    B4C_REQUIRE(ld_w >= K && ld_w % 8 == 0 && ((uintptr_t)wt & 15) == 0, "candidate_score: wt pitch %d (>= K, a multiple of 8) and "
                "16-B alignment", ld_w);
    B4C_REQUIRE(!scores || ld_s >= C, "candidate_score: ld_s < C");
    B4C_REQUIRE(!rank || labels, "candidate_score: rank needs labels");
    B4C_REQUIRE(k >= 0 && k <= B4C_MAX_TOPK && (k == 0) == (idx == nullptr), "candidate_score: k = %d (0 .. %d; idx iff k > 0)", k,
                B4C_MAX_TOPK);
    if (R == 0) return B4C_OK;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == B4C_F32) cand_score_dispatch<float>(h, ld_h, wt, ld_w, bias, cand, ld_c, R, C, V, K, labels, scores, ld_s, rank, k, idx, st);
    else cand_score_dispatch<bf16_t>(h, ld_h, wt, ld_w, bias, cand, ld_c, R, C, V, K, labels, scores, ld_s, rank, k, idx, st);
    return b4c_check_launch("candidate_score");
}

extern "C" int b4c_candidate_rank_rows(const void *scores, int ld, int dtype, const int32_t *cand, int ld_c, int64_t R, int C, int V,
                                       const int32_t *labels, int32_t *rank, int k, int32_t *idx, void *stream) {
    B4C_REQUIRE(R >= 0 && V > 0 && C >= 1 && C <= B4C_MAX_CAND, "candidate_rank_rows: R = %lld, V = %d, C = %d (1 .. %d)",
                (long long)R, V, C, B4C_MAX_CAND);
    B4C_REQUIRE(dtype == B4C_F32 || dtype == B4C_BF16, "candidate_rank_rows: dtype %d", dtype);
    B4C_REQUIRE(scores && cand && ld >= V && ld_c >= C, "candidate_rank_rows: null pointer, ld < V or ld_c < C");
    B4C_REQUIRE(!rank || labels, "candidate_rank_rows: rank needs labels");
    B4C_REQUIRE(k >= 0 && k <= B4C_MAX_TOPK && (k == 0) == (idx == nullptr), "candidate_rank_rows: k = %d (0 .. %d; idx iff k > 0)", k,
                B4C_MAX_TOPK);
    if (R == 0) return B4C_OK;
    hipStream_t st = (hipStream_t)stream;
    const int hb = sampler_hash_bits(C);
    const size_t lds = (size_t)C * 8 + (rank ? (size_t)8 << hb : 0);
    if (dtype == B4C_F32)
        cand_rank_rows_kernel<float><<<(unsigned)R, 64, lds, st>>>((const float *)scores, ld, cand, ld_c, C, V, labels, rank, k, idx, hb);
    else
        cand_rank_rows_kernel<bf16_t><<<(unsigned)R, 64, lds, st>>>((const bf16_t *)scores, ld, cand, ld_c, C, V, labels, rank, k, idx, hb);
    return b4c_check_launch("candidate_rank_rows");
}
