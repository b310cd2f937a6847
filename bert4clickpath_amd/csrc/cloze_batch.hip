// Cloze batches built on the device (include/b4c.h, "Cloze batches"): one row of model input ids and padded labels per named
// sequence of a CSR data set, masked by a rule that is a pure function of (seed, sequence index, sequence, mode).
//
// One 256-thread workgroup per row, three phases with a barrier between them: the L <= 1021 keys go to LDS (8 KB), every
// thread ranks its own positions by counting the smaller (key, position) pairs over LDS, then writes its columns -- a masked
// position's label slot is the number of masked positions before it.  O(L^2) compares per row (40 k at L = 200): integer work
// beside a training step of milliseconds; nothing here is tuned further.
#include "common.h"

#define CLOZE_MAX_W 1021     // p < 1024 in the counter, S = W + 3 <= 1024
#define CLOZE_MAX_M 64
#define CLOZE_THREADS 256
#define CLOZE_RESERVED 10    // NUM_RESERVED_TOKENS: input id = item index + 10
#define CLOZE_MASK_ID 1
#define CLOZE_INPUT_PAD 0
#define CLOZE_LABEL_PAD (-1.0f)

// ---- the rule: shared by the kernel and the host entry ---------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t cloze_key(uint64_t seed, uint64_t g, int p) {
    return b4c_rand64(seed, (g << 10) | (uint64_t)(uint32_t)p);
}
// (ka, a) < (kb, b), lexicographic: ties of the key go to the lower position, so the order is total
__host__ __device__ __forceinline__ bool cloze_before(uint64_t ka, int a, uint64_t kb, int b) { return ka < kb || (ka == kb && a < b); }
// position p is masked iff fewer than n positions come before it
__host__ __device__ __forceinline__ bool cloze_chosen(const uint64_t *keys, int L, int p, int n) {
    const uint64_t kp = keys[p];
    int c = 0;
    for (int q = 0; q < L; ++q) c += cloze_before(keys[q], q, kp, p) ? 1 : 0;
    return c < n;
}
// float32 product, then truncation: input_pipeline.n_masked
__host__ __device__ __forceinline__ int cloze_n_masked(int L, float masked_percentage, int max_masked) {
    int n = (int)((float)L * masked_percentage);
    n = n < 0 ? 0 : n;
    return n > max_masked ? max_masked : n;                    // <= L: masked_percentage <= 1 (checked by the entry point)
}

// ---- kernel ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CLOZE_THREADS) cloze_batch_kernel(const int32_t *__restrict__ items, const int64_t *__restrict__ offsets,
                                                                    const int32_t *__restrict__ seq_idx, int W, int mode,
                                                                    float masked_percentage, int max_masked, uint64_t seed,
                                                                    int64_t *__restrict__ items_out, int ld_items,
                                                                    float *__restrict__ labels_out, int ld_lab, int M,
                                                                    int32_t *__restrict__ n_masked_out) {
    __shared__ uint64_t keys[1024];
    __shared__ uint8_t chosen[1024];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t g = seq_idx[b];
    int64_t o0 = 0, len = 0;
    if (g >= 0) {
        o0 = offsets[g];
        len = offsets[g + 1] - o0;
    }
    if (mode == 0) len -= 1;                                   // TRAIN: the last item is held out
    const int L = len < 0 ? 0 : (len > W ? W : (int)len);      // longer than W: the caller's error; nothing leaves the row
    const int n = mode == 0 ? cloze_n_masked(L, masked_percentage, max_masked) : (L > 0 ? 1 : 0);
    if (mode == 0) {
        for (int p = tid; p < L; p += CLOZE_THREADS) keys[p] = cloze_key(seed, (uint64_t)g, p);
        __syncthreads();
        for (int p = tid; p < L; p += CLOZE_THREADS) chosen[p] = cloze_chosen(keys, L, p, n) ? 1 : 0;
    } else {
        for (int p = tid; p < L; p += CLOZE_THREADS) chosen[p] = p == L - 1 ? 1 : 0;
    }
    __syncthreads();
    int64_t *row = items_out + b * (int64_t)ld_items;
    float *lab = labels_out + b * (int64_t)ld_lab;
    for (int p = tid; p < W; p += CLOZE_THREADS) {
        int64_t id = CLOZE_INPUT_PAD;
        if (p < L) {
            const int item = items[o0 + p];
            if (chosen[p]) {
                int slot = 0;
                for (int q = 0; q < p; ++q) slot += chosen[q];
                if (slot < M) lab[slot] = (float)item;
                id = CLOZE_MASK_ID;
            } else {
                id = (int64_t)item + CLOZE_RESERVED;
            }
        }
        row[p] = id;
    }
    for (int s = n + tid; s < M; s += CLOZE_THREADS) lab[s] = CLOZE_LABEL_PAD;
    if (n_masked_out && tid == 0) n_masked_out[b] = n;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------
extern "C" int b4c_cloze_batch(const int32_t *items, const int64_t *offsets, const int32_t *seq_idx, int B, int W, int mode,
                               float masked_percentage, int max_masked, uint64_t seed, int64_t *items_out, int ld_items,
                               float *labels_out, int ld_lab, int M, int32_t *n_masked_out, void *stream) {
    B4C_REQUIRE(B >= 0 && W >= 1 && W <= CLOZE_MAX_W, "cloze_batch: B = %d, W = %d (1 .. %d)", B, W, CLOZE_MAX_W);
    B4C_REQUIRE(mode == 0 || mode == 1, "cloze_batch: mode %d (0 = TRAIN, 1 = EVAL)", mode);
    B4C_REQUIRE(M >= mode && M <= CLOZE_MAX_M, "cloze_batch: M = %d (%d .. %d)", M, mode, CLOZE_MAX_M);       // EVAL masks one position
    B4C_REQUIRE(mode == 1 || (max_masked >= 0 && max_masked <= M), "cloze_batch: max_masked = %d (0 .. M = %d)", max_masked, M);
    B4C_REQUIRE(mode == 1 || (masked_percentage >= 0.f && masked_percentage <= 1.f), "cloze_batch: masked_percentage %g outside [0, 1]",
                (double)masked_percentage);
    B4C_REQUIRE(ld_items >= W && ld_lab >= M, "cloze_batch: ld_items = %d < W = %d or ld_lab = %d < M = %d", ld_items, W, ld_lab, M);
    if (B == 0) return B4C_OK;
    B4C_REQUIRE(items && offsets && seq_idx && items_out && (labels_out || M == 0), "cloze_batch: null pointer");
    cloze_batch_kernel<<<(unsigned)B, CLOZE_THREADS, 0, (hipStream_t)stream>>>(items, offsets, seq_idx, W, mode, masked_percentage,
                                                                              max_masked, seed, items_out, ld_items, labels_out,
                                                                              ld_lab, M, n_masked_out);
    return b4c_check_launch("cloze_batch");
}

// the TRAIN rule on the host: the n positions of [0, L) that the kernel masks for sequence g, ascending
extern "C" int b4c_cloze_choose(uint64_t seed, int64_t g, int L, int n, int32_t *pos) {
    B4C_REQUIRE(L >= 0 && L <= CLOZE_MAX_W && n >= 0 && n <= L, "cloze_choose: L = %d (0 .. %d), n = %d (0 .. L)", L, CLOZE_MAX_W, n);
    B4C_REQUIRE(g >= 0 && g < ((int64_t)1 << 54), "cloze_choose: g = %lld (0 .. 2^54)", (long long)g);
    B4C_REQUIRE(pos || n == 0, "cloze_choose: null pointer");
    uint64_t keys[1024];
    for (int p = 0; p < L; ++p) keys[p] = cloze_key(seed, (uint64_t)g, p);
    int k = 0;
    for (int p = 0; p < L && k < n; ++p)
        if (cloze_chosen(keys, L, p, n)) pos[k++] = p;
    return B4C_OK;
}
