// Shared device/host helpers for libb4c_hip.so (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/b4c.h"

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

#define B4C_WAVE 64

// Workgroup barrier that orders LDS only.  __syncthreads() also makes every wave wait for ALL of its
// outstanding global loads and stores (s_waitcnt vmcnt(0)): inside a loop that stores results or keeps a
// prefetch in flight, that drains the memory pipeline once per iteration.  Use this where only LDS data is
// exchanged between the waves.
#define B4C_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

void b4c_set_error(const char *fmt, ...);
int b4c_check_launch(const char *what);

#define B4C_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            b4c_set_error(__VA_ARGS__);   \
            return B4C_EINVAL;            \
        }                                 \
    } while (0)

static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Opt `kernel` in to `bytes` of dynamic LDS (more than the 64 KiB a launch may ask for unasked).  Per host thread the runtime is
// called when the kernel is new or asks for more than it was last given.  One table per kernel signature and file; the most that
// share one are vocab_ce.hip's 12 token sweeps over VceArgs.  A kernel that finds the table full is not remembered: it asks every time.
template <typename K> static void b4c_allow_lds(K kernel, size_t bytes) {
    constexpr int CAP = 32;
    static thread_local const void *done[CAP];
    static thread_local size_t done_bytes[CAP];
    static thread_local int ndone = 0;
    int i = 0;
    while (i < ndone && done[i] != (const void *)kernel) ++i;
    if (i < ndone && done_bytes[i] >= bytes) return;
    (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (i < CAP) { done[i] = (const void *)kernel; done_bytes[i] = bytes; if (i == ndone) ++ndone; }
}

// A run-time value as a template argument: f is called with std::true_type / std::false_type, or with the
// std::integral_constant<int, V> of the listed V that v equals (returns false, f not called, when v is none of them).  Nested, they
// take the place of one macro ladder per launcher; the launch statement is written once, inside the innermost lambda:
//   b4c_by_int<32, 64>(dh, [&](auto DH) { b4c_by_bool(causal, [&](auto CA) { kernel<DH(), CA()><<<grid, block, 0, st>>>(...); }); });
template <typename F> static inline void b4c_by_bool(bool v, F &&f) {
    if (v) f(std::true_type{}); else f(std::false_type{});
}
template <int... Vs, typename F> static inline bool b4c_by_int(int v, F &&f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// ---- element IO: 8 consecutive elements <-> 8 floats (16 B for bf16, 32 B for fp32) ----
// Which streaming outputs use nontemporal stores (bit per site): measured per site on the C2 step.
#ifndef B4C_NT_MASK
#define B4C_NT_MASK 255
#endif
#define B4C_NT(site) (((B4C_NT_MASK) >> (site)) & 1)
#define B4C_NT_EMBED 0
#define B4C_NT_GEMM 1
#define B4C_NT_GEMMLN_Z 2
#define B4C_NT_GEMMLN_OUT 3
#define B4C_NT_LNBWD_DZ 4
#define B4C_NT_LNBWD_DY 5
#define B4C_NT_ATTN_O 6
#define B4C_NT_ATTN_DQKV 7
template <typename T> struct Vec8;
template <> struct Vec8<float> {
    static __device__ __forceinline__ void load(const float *p, float (&v)[8]) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p);
        const f32x4 b = *reinterpret_cast<const f32x4 *>(p + 4);
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
        v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    }
    static __device__ __forceinline__ void store(float *p, const float (&v)[8]) {
        f32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
        *reinterpret_cast<f32x4 *>(p) = a;
        *reinterpret_cast<f32x4 *>(p + 4) = b;
    }
    // streaming store (nt bit): for outputs that are far larger than L2 and are next read by another kernel
    static __device__ __forceinline__ void store_nt(float *p, const float (&v)[8]) {
        f32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
        __builtin_nontemporal_store(a, reinterpret_cast<f32x4 *>(p));
        __builtin_nontemporal_store(b, reinterpret_cast<f32x4 *>(p + 4));
    }
    template <bool NT> static __device__ __forceinline__ void store_sel(float *p, const float (&v)[8]) {
        if (NT) store_nt(p, v); else store(p, v);
    }
};
template <> struct Vec8<bf16_t> {
    static __device__ __forceinline__ void load(const bf16_t *p, float (&v)[8]) {
        const bf16x8 a = *reinterpret_cast<const bf16x8 *>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)a[i];
    }
    static __device__ __forceinline__ void store(bf16_t *p, const float (&v)[8]) {
        bf16x8 a;
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = (bf16_t)v[i];
        *reinterpret_cast<bf16x8 *>(p) = a;
    }
    static __device__ __forceinline__ void store_nt(bf16_t *p, const float (&v)[8]) {
        bf16x8 a;
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = (bf16_t)v[i];
        __builtin_nontemporal_store(a, reinterpret_cast<bf16x8 *>(p));
    }
    template <bool NT> static __device__ __forceinline__ void store_sel(bf16_t *p, const float (&v)[8]) {
        if (NT) store_nt(p, v); else store(p, v);
    }
};

// one row (or part of one) of N elements <-> N floats, and its dot product with an fp32 row in LDS (the lanes that share `row`
// read one address: broadcast)
template <typename T, int N>
__device__ __forceinline__ void load_row(const T *__restrict__ p, float (&v)[N]) {
#pragma unroll
    for (int c = 0; c < N; c += 8) {
        float t[8];
        Vec8<T>::load(p + c, t);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[c + k] = t[k];
    }
}
template <typename T, int N>
__device__ __forceinline__ void store_row(T *__restrict__ p, const float (&v)[N]) {
#pragma unroll
    for (int c = 0; c < N; c += 8) {
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = v[c + k];
        Vec8<T>::store(p + c, t);
    }
}
template <int N> __device__ __forceinline__ float dot_lds(const float (&a)[N], const float *__restrict__ row) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < N; d += 4) {
        const f32x4 kv = *reinterpret_cast<const f32x4 *>(row + d);
        s += a[d] * kv[0];
        s += a[d + 1] * kv[1];
        s += a[d + 2] * kv[2];
        s += a[d + 3] * kv[3];
    }
    return s;
}

// ---- counter-based dropout mask ----
// Threefry-2x32 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), 12 rounds,
// key = seed, counter = e >> 2: 64 random bits = four 16-bit uniforms, one per element.  Adds, rotates and xors
// only: 32-bit integer multiplies run at quarter rate on CDNA, and the 64-bit-multiply mixer used first made the
// mask the most expensive part of every dropout site (0.9 ms of the 19.2 ms C2 step).
__host__ __device__ __forceinline__ uint32_t b4c_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__host__ __device__ __forceinline__ uint64_t b4c_rand64(uint64_t seed, uint64_t ctr) {
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), k2 = 0x1BD11BDAu ^ k0 ^ k1;
    uint32_t x0 = (uint32_t)ctr + k0, x1 = (uint32_t)(ctr >> 32) + k1;
#define B4C_TF_ROUND(R) x0 += x1; x1 = b4c_rotl32(x1, R); x1 ^= x0;
    B4C_TF_ROUND(13) B4C_TF_ROUND(15) B4C_TF_ROUND(26) B4C_TF_ROUND(6)
    x0 += k1; x1 += k2 + 1u;
    B4C_TF_ROUND(17) B4C_TF_ROUND(29) B4C_TF_ROUND(16) B4C_TF_ROUND(24)
    x0 += k2; x1 += k0 + 2u;
    B4C_TF_ROUND(13) B4C_TF_ROUND(15) B4C_TF_ROUND(26) B4C_TF_ROUND(6)
    x0 += k0; x1 += k1 + 3u;
#undef B4C_TF_ROUND
    return (uint64_t)x0 | ((uint64_t)x1 << 32);
}
// element e is kept iff its 16-bit uniform >= ceil(rate * 65536)
__host__ __device__ __forceinline__ uint32_t b4c_keep_threshold(float rate) {
    const float t = rate * 65536.0f;
    uint32_t thr = (uint32_t)t;
    if ((float)thr < t) ++thr;
    return thr;
}
__host__ __device__ __forceinline__ bool b4c_keep_elem(uint64_t seed, uint64_t e, float rate) {
    const uint64_t h = b4c_rand64(seed, e >> 2);
    return (uint32_t)((h >> (16 * (e & 3))) & 0xFFFFu) >= b4c_keep_threshold(rate);
}
// keep bits of the 8 consecutive elements e0 .. e0+7 (e0 % 4 == 0): bit k = element e0 + k.  Two hashes.
__host__ __device__ __forceinline__ uint32_t b4c_keep8(uint64_t seed, uint64_t e0, uint32_t thr) {
    const uint64_t h0 = b4c_rand64(seed, e0 >> 2), h1 = b4c_rand64(seed, (e0 >> 2) + 1);
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        m |= (((uint32_t)(h0 >> (16 * k)) & 0xFFFFu) >= thr ? 1u : 0u) << k;
        m |= (((uint32_t)(h1 >> (16 * k)) & 0xFFFFu) >= thr ? 1u : 0u) << (4 + k);
    }
    return m;
}

// ---- attention-probability dropout: the one keep rule (include/b4c.h, b4c_attn_keep) ----
// The probability of (sequence b, head h, query q, key k) is element e = ((b*H + h) * S_arg + q) * S4 + k of the keep-mask
// stream, S4 = S_arg rounded up to a multiple of 4; q, k = row indices inside the sequence, S_arg = the pitch of the launch (S, or
// the packed layout's max_len).  S4 % 4 == 0: the four keys k0 .. k0+3 (k0 % 4 == 0) of one query share ONE hash, whose
// counter is b4c_attn_ctr(row, k0), row = (b*H + h) * S_arg + q.
__host__ __device__ __forceinline__ uint32_t b4c_attn_s4(int S_arg) { return ((uint32_t)S_arg + 3u) & ~3u; }
__host__ __device__ __forceinline__ uint64_t b4c_attn_ctr(uint64_t row, int k0, int S_arg) {
    return row * (b4c_attn_s4(S_arg) >> 2) + (uint32_t)(k0 >> 2);
}
__host__ __device__ __forceinline__ bool b4c_attn_keep_elem(uint64_t seed, int b, int h, int q, int k, int H, int S_arg, float rate) {
    const uint64_t row = ((uint64_t)b * H + h) * S_arg + q;
    return b4c_keep_elem(seed, row * b4c_attn_s4(S_arg) + (uint32_t)k, rate);
}
// keep bits of the keys k0 .. k0+3 of one query (bit j = key k0 + j), ctr = b4c_attn_ctr(row, k0, S_arg).  One hash.
__host__ __device__ __forceinline__ uint32_t b4c_attn_keep4(uint64_t seed, uint64_t ctr, uint32_t thr) {
    const uint64_t h = b4c_rand64(seed, ctr);
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) m |= (((uint32_t)(h >> (16 * j)) & 0xFFFFu) >= thr ? 1u : 0u) << j;
    return m;
}
// (device) the workgroup-uniform part of b4c_attn_ctr for item bh = b*H + h, and the value of lane C of every quad (DPP quad
// broadcast; EXEC must be full): what the matrix-core attention kernels build their keep bits from
__device__ __forceinline__ uint64_t attn_ctr_base(int bh, int S_arg) { return (uint64_t)bh * S_arg * (b4c_attn_s4(S_arg) >> 2); }
template <int C> __device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, C * 0x55, 0xf, 0xf, true);
}

// ---- activations ----
// GELU (B4C_ACT_GELU: x Phi(x) with erf; B4C_ACT_GELU_TANH: the tanh form) and its derivative, in fp32.  The derivative is
// applied to the SAVED pre-activation u (the `pre` output of b4c_gemm_nt_act): GELU is not monotone, so unlike ReLU its
// backward cannot be read off the activation.
__device__ __forceinline__ float act_gelu(float x, int act) {
    if (act == B4C_ACT_GELU) return 0.5f * x * (1.f + erff(x * 0.70710678118654752f));
    const float t = tanhf(0.79788456080286536f * (x + 0.044715f * x * x * x));
    return 0.5f * x * (1.f + t);
}
__device__ __forceinline__ float act_gelu_grad(float u, int act) {
    if (act == B4C_ACT_GELU)      // Phi(u) + u phi(u)
        return 0.5f * (1.f + erff(u * 0.70710678118654752f)) + u * 0.39894228040143268f * __expf(-0.5f * u * u);
    u = fminf(fmaxf(u, -10.f), 10.f);      // tanh is +-1 in fp32 well before |u| = 10: the step's limit, and u * u stays finite
    const float u2 = u * u;
    const float t = tanhf(0.79788456080286536f * (u + 0.044715f * u * u2));
    return 0.5f * (1.f + t) + 0.5f * u * (1.f - t * t) * 0.79788456080286536f * (1.f + 3.f * 0.044715f * u2);
}

// ---- wave / block reductions ----
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// reduce over groups of G consecutive lanes (G power of two <= 64)
template <int G> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
