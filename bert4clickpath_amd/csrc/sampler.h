// The negative sampler of candidates.hip (b4c_sample_candidates) and of next_item_batch.hip, which promises each of its lists to be
// what b4c_sample_candidates draws for that one target (include/b4c.h): one wave per list, both call sampler_wave.
#pragma once
#include "common.h"

// ---- the draws: shared with the host entry b4c_next_item_row ------------------------------------------------------------------
// attempt j of the list with the counter i (b4c_sample_candidates: row_base + row; next-item: the target token's CSR index)
__host__ __device__ __forceinline__ uint64_t sampler_draw(uint64_t seed, uint64_t i, uint32_t j) { return b4c_rand64(seed, (i << 20) | j); }
__host__ __device__ __forceinline__ uint64_t sampler_mulhi64(uint64_t x, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(x, v);
#else
    return (uint64_t)(((unsigned __int128)x * v) >> 64);
#endif
}
// the drawn item: uniform mulhi64(x, V), or min{i : cdf[i] > mulhi64(x, total)}; -1 when the cdf has no mass
__host__ __device__ __forceinline__ int sampler_item_of(uint64_t x, int V, const int64_t *cdf, uint64_t total) {
    if (!cdf) return (int)sampler_mulhi64(x, (uint64_t)V);
    if ((int64_t)total <= 0) return -1;
    const uint64_t u = sampler_mulhi64(x, total);
    int lo = 0, hi = V - 1;                                    // cdf[V - 1] = total > u
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint64_t)cdf[mid] > u) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// ---- LDS sets ------------------------------------------------------------------------------------------------------------------
// hash tables of item ids (linear probing, 2^hb slots, -1: free): the sampler's accepted set and the rank's first-occurrence table
__device__ __forceinline__ int sampler_hash_slot(int item, int hb) { return (int)(((uint32_t)item * 2654435761u) >> (32 - hb)); }
static inline int sampler_hash_bits(int n) {                   // hb of a table for n ids: at least 64 slots, at most half full
    int hb = 6;
    while ((1 << hb) < 2 * n) ++hb;
    return hb;
}
__device__ __forceinline__ bool sampler_hash_has(const int *tab, int hb, int item) {
    for (int s = sampler_hash_slot(item, hb);; s = (s + 1) & ((1 << hb) - 1)) {
        const int v = tab[s];
        if (v == item) return true;
        if (v < 0) return false;
    }
}
__device__ __forceinline__ void sampler_hash_put(int *tab, int hb, int item) {
    for (int s = sampler_hash_slot(item, hb);; s = (s + 1) & ((1 << hb) - 1))
        if (atomicCAS(&tab[s], -1, item) == -1) return;
}
// sx[0 .. n): ascending ids, duplicates allowed (a lower-bound search)
__device__ __forceinline__ bool sampler_sorted_has(const int *sx, int n, int item) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sx[mid] < item) lo = mid + 1; else hi = mid;
    }
    return lo < n && sx[lo] == item;
}
// one wave's LDS writes are visible to its own later reads: order them for the compiler, the hardware keeps a wave's LDS in order
__device__ __forceinline__ void sampler_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- one list by one wave: out[0] = y, then N negatives, -1 where the 64 N attempts did not yield them (counted in short_count) -----
// Step t: lane l makes attempt j = 64 t + l.  An item is refused when it is y, in the exclusion set sx[0 .. nx) (written by this wave
// or in front of a workgroup barrier) or in the accepted set tab (2^hb slots of this wave's own); an earlier lane of the step with the
// same item wins (its attempt comes first), and the accepted lanes append in lane order through a ballot prefix count.
__device__ __forceinline__ void sampler_wave(const int *sx, int nx, int *tab, int hb, int y, int V, int N, uint64_t seed, uint64_t i,
                                             const int64_t *__restrict__ cdf, uint64_t total, int32_t *__restrict__ out,
                                             int32_t *__restrict__ short_count, int lane) {
    if (y < 0 || y >= V) {
        for (int p = lane; p <= N; p += 64) out[p] = -1;
        return;
    }
    for (int s = lane; s < (1 << hb); s += 64) tab[s] = -1;
    sampler_wave_sync();
    int count = 0;
    for (int t = 0; t < N && count < N; ++t) {
        const int item = sampler_item_of(sampler_draw(seed, i, (uint32_t)(t * 64 + lane)), V, cdf, total);
        bool ok = item >= 0 && item != y && !sampler_sorted_has(sx, nx, item) && !sampler_hash_has(tab, hb, item);
        const int mine = ok ? item : -1;
#pragma unroll 8
        for (int l = 0; l < 63; ++l) {
            const int v = __builtin_amdgcn_readlane(mine, l);
            if (l < lane && v == item) ok = false;
        }
        const uint64_t m = __ballot(ok);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (ok && count + pre < N) {
            out[1 + count + pre] = item;
            sampler_hash_put(tab, hb, item);
        }
        count += __popcll(m);
        sampler_wave_sync();
    }
    if (count > N) count = N;
    for (int p = 1 + count + lane; p <= N; p += 64) out[p] = -1;
    if (lane == 0) {
        out[0] = y;
        if (count < N) atomicAdd(short_count, 1);
    }
}
