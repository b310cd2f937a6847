// Global L2 norm of the fp32 gradient arena and the clip coefficient of Adam(global_clipnorm=...), on the device.
//
// POSITION-DEFINED REDUCTION.  The value depends on the gradient's contents only, never on who computed it, over which
// range, or in what order:
//   * the arena is cut into chunks of B4C_GRAD_CHUNK (1024) consecutive elements, counted from the arena's first element
//     (a chunk is a property of the arena offset, not of any parameter: it may hold the tail of one parameter and the head
//     of the next);
//   * partial[c] is the float64 sum of the squares of the WHOLE chunk c (clipped to the arena's end), in one fixed order:
//     lane l of a wave adds elements 4 (l + 64 j) + k for j = 0..3, k = 0..3 in that order, then a 6-level xor butterfly
//     over the lanes.  fp32 x fp32 is exact in float64 and cannot overflow or underflow there, so gradients of 1e-20 and of
//     1e15 (what the optimizer tests feed) are summed as they are;
//   * whoever writes partial[c] -- the dense pass over a range that touches the chunk, or the row pass for a row that
//     overlaps it -- reads the whole chunk and stores the same bits.  Recomputing is idempotent: duplicates and neighbours
//     store the same value, so the row form needs no sort, no claim array and no atomic.  A row-lazy optimizer zero-fills
//     its partials first, so a chunk nobody names contributes an exact 0.0 (its gradient IS all zeros: optim.LazyRows),
//     and the dense optimizer's pass over such a chunk stores the same 0.0;
//   * total = a tree over partial[0 .. n_chunks) whose shape depends on n_chunks only, in two levels (groups of
//     B4C_GRAD_GROUP = 4096 partials, one workgroup each; then one workgroup over the group sums), so no single workgroup
//     reads megabytes (config 5: 500k partials).
// Hence the row-lazy optimizer and the dense one, and every replica of a data-parallel run, get the same bits.
//
//   norm = (float)(sqrt(total) |grad_mul|)                                  (for logging)
//   coef = norm64 > clip ? (float)(clip / norm64) : 1.0f;   NaN when the norm is not finite (tf.clip_by_global_norm does the
//          same: the failure shows, it does not hide)
// coef is EXACTLY 1.0f when nothing is clipped, where TensorFlow computes clip * min(1 / norm, 1 / clip) (at most one
// rounding away): it buys "a clip that never bites changes no bit".  Parity is unpinned here: the reference never clips.
// The two scalars are written by one lane with ordinary vector stores; nothing here synchronises with the host.
#include "common.h"

#define GN_CHUNK B4C_GRAD_CHUNK
#define GN_GROUP B4C_GRAD_GROUP

__device__ __forceinline__ double gn_wave_sum(double acc) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);      // a + b == b + a bit for bit: every lane ends equal
    return acc;
}

// float64 sum of the squares of chunk c of g[0, n): the whole wave, the same value in every lane
__device__ __forceinline__ double gn_chunk_sumsq(const float *__restrict__ g, int64_t n, int64_t c, int lane) {
    const int64_t base = c * GN_CHUNK;
    double acc = 0.0;
    if (base + GN_CHUNK <= n) {
        f32x4 x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = *reinterpret_cast<const f32x4 *>(g + base + (lane + 64 * j) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) { const double d = (double)x[j][k]; acc += d * d; }
    } else {                                              // the arena's last chunk: elements past the end count as 0 (adds +0.0)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t e = base + (lane + 64 * j) * 4 + k;
                const double d = e < n ? (double)g[e] : 0.0;
                acc += d * d;
            }
    }
    return gn_wave_sum(acc);
}

// dense form: one wave per chunk, grid-stride over the chunks [c_lo, c_hi)
__global__ void __launch_bounds__(256) grad_sumsq_kernel(const float *__restrict__ g, int64_t n, int64_t c_lo, int64_t c_hi,
                                                         double *__restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t c = c_lo + blockIdx.x * 4ll + wave; c < c_hi; c += (int64_t)gridDim.x * 4) {
        const double s = gn_chunk_sumsq(g, n, c, lane);
        if (lane == 0) partial[c] = s;
    }
}

// row form: one wave per entry of ids (repeats allowed, clamped as adam_rows_kernel clamps them) recomputes every chunk the
// row [table_lo + r width, + width) overlaps
__global__ void __launch_bounds__(256) grad_sumsq_rows_kernel(const float *__restrict__ g, int64_t n, int64_t table_lo, int64_t rows,
                                                              int width, const int64_t *__restrict__ ids, int64_t n_ids,
                                                              double *__restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t i = blockIdx.x * 4ll + wave;
    if (i >= n_ids) return;
    int64_t r = ids[i];
    r = r < 0 ? 0 : (r >= rows ? rows - 1 : r);
    const int64_t first = table_lo + r * (int64_t)width;
    const int64_t c1 = (first + width - 1) / GN_CHUNK;
    for (int64_t c = first / GN_CHUNK; c <= c1; ++c) {
        const double s = gn_chunk_sumsq(g, n, c, lane);
        if (lane == 0) partial[c] = s;
    }
}

// 256 threads: thread t adds src[t], src[t + 256], ... (count entries) in that order; then butterfly per wave and
// ((w0 + w1) + w2) + w3.  Valid in thread 0.
__device__ __forceinline__ double gn_block_sum(const double *__restrict__ src, int64_t count, double *lds) {
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += 256) acc += src[i];
    acc = gn_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__global__ void __launch_bounds__(256) grad_group_sums_kernel(const double *__restrict__ partial, int64_t n_chunks,
                                                              double *__restrict__ group_sums) {
    __shared__ double lds[4];
    const int64_t lo = blockIdx.x * (int64_t)GN_GROUP;
    const int64_t count = n_chunks - lo < GN_GROUP ? n_chunks - lo : GN_GROUP;
    const double s = gn_block_sum(partial + lo, count, lds);
    if (threadIdx.x == 0) group_sums[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) grad_clip_coef_kernel(const double *__restrict__ group_sums, int64_t n_groups, float clip,
                                                             float grad_mul, double *__restrict__ total, float *__restrict__ norm_coef) {
    __shared__ double lds[4];
    const double s = gn_block_sum(group_sums, n_groups, lds);
    if (threadIdx.x == 0) {
        const double norm64 = sqrt(s) * fabs((double)grad_mul);
        float coef = 1.0f;
        if (!(norm64 < __builtin_inf())) coef = __builtin_nanf("");             // Inf or NaN in the gradient
        else if (norm64 > (double)clip) coef = (float)((double)clip / norm64);
        if (total) *total = s;
        norm_coef[0] = (float)norm64;
        norm_coef[1] = coef;
    }
}

static inline int64_t gn_chunks(int64_t n) { return (n + GN_CHUNK - 1) / GN_CHUNK; }

extern "C" int b4c_grad_sumsq(const float *g, int64_t n, int64_t lo, int64_t hi, double *partial, void *stream) {
    B4C_REQUIRE(g && partial && n > 0, "grad_sumsq: null pointer / empty arena");
    B4C_REQUIRE(((uintptr_t)g & 15) == 0 && ((uintptr_t)partial & 7) == 0, "grad_sumsq: the arena must be 16-byte aligned, the partials 8-byte");
    B4C_REQUIRE(lo >= 0 && lo <= hi && hi <= n, "grad_sumsq: range [%lld, %lld) outside the arena of %lld elements", (long long)lo,
                (long long)hi, (long long)n);
    if (lo == hi) return B4C_OK;
    const int64_t c_lo = lo / GN_CHUNK, c_hi = gn_chunks(hi);
    int64_t blocks = (c_hi - c_lo + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    grad_sumsq_kernel<<<(int)blocks, 256, 0, (hipStream_t)stream>>>(g, n, c_lo, c_hi, partial);
    return b4c_check_launch("grad_sumsq");
}

extern "C" int b4c_grad_sumsq_rows(const float *g, int64_t n, int64_t table_lo, int64_t rows, int width, const int64_t *ids,
                                   int64_t n_ids, double *partial, void *stream) {
    B4C_REQUIRE(g && partial && ids && n > 0, "grad_sumsq_rows: null pointer / empty arena");
    B4C_REQUIRE(((uintptr_t)g & 15) == 0 && ((uintptr_t)partial & 7) == 0 && ((uintptr_t)ids & 7) == 0,
                "grad_sumsq_rows: the arena must be 16-byte aligned, the partials and the ids 8-byte");
    B4C_REQUIRE(rows > 0 && width > 0 && table_lo >= 0 && table_lo <= n && rows <= (n - table_lo) / width,
                "grad_sumsq_rows: table [%lld + %lld x %d) outside the arena of %lld elements", (long long)table_lo, (long long)rows,
                width, (long long)n);
    if (n_ids <= 0) return B4C_OK;
    const int64_t blocks = (n_ids + 3) / 4;
    B4C_REQUIRE(blocks < (1ll << 31), "grad_sumsq_rows: %lld ids in one call", (long long)n_ids);
    grad_sumsq_rows_kernel<<<(int)blocks, 256, 0, (hipStream_t)stream>>>(g, n, table_lo, rows, width, ids, n_ids, partial);
    return b4c_check_launch("grad_sumsq_rows");
}

extern "C" int b4c_grad_clip_coef(const double *partial, int64_t n_chunks, double *group_sums, int64_t n_groups, float clip,
                                  float grad_mul, double *total, float *norm_coef, void *stream) {
    B4C_REQUIRE(partial && group_sums && norm_coef && n_chunks > 0, "grad_clip_coef: null pointer / no chunks");
    B4C_REQUIRE((((uintptr_t)partial | (uintptr_t)group_sums | (uintptr_t)total) & 7) == 0 && ((uintptr_t)norm_coef & 3) == 0,
                "grad_clip_coef: misaligned pointer");
    B4C_REQUIRE(n_groups == (n_chunks + GN_GROUP - 1) / GN_GROUP && n_groups < (1ll << 31),
                "grad_clip_coef: %lld chunks need %lld group sums, not %lld", (long long)n_chunks,
                (long long)((n_chunks + GN_GROUP - 1) / GN_GROUP), (long long)n_groups);
    B4C_REQUIRE(clip > 0.f, "grad_clip_coef: clip %g must be positive", (double)clip);
    grad_group_sums_kernel<<<(int)n_groups, 256, 0, (hipStream_t)stream>>>(partial, n_chunks, group_sums);
    int rc = b4c_check_launch("grad_clip_coef (group sums)");
    if (rc) return rc;
    grad_clip_coef_kernel<<<1, 256, 0, (hipStream_t)stream>>>(group_sums, n_groups, clip, grad_mul, total, norm_coef);
    return b4c_check_launch("grad_clip_coef");
}
