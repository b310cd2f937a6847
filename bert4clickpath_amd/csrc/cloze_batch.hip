// Cloze batches built on the device (include/b4c.h, "Cloze batches"): one row of model input ids and padded labels per named
// sequence of a CSR data set, masked by a rule that is a pure function of (seed, sequence index, sequence, mode).
//
// One 256-thread workgroup per row, three phases with a barrier between them: the L <= 1021 keys go to LDS (8 KB), every
// thread ranks its own positions by counting the smaller (key, position) pairs over LDS, then writes its columns -- a masked
// position's label slot is the number of masked positions before it.  O(L^2) compares per row (40 k at L = 200): integer work
// beside a training step of milliseconds; nothing here is tuned further.
// The windowed entry ("Cloze batches over windows") fetches (g, a, L) from a device table (batch_rows.h: row_window and the Cloze
// layout of batch_row_rule) and decides the last-only rows in front of the same three phases; b4c_cloze_history is a plain gather
// of the items in front of a sequence's target.
#include "batch_rows.h"

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

// window seed and the last-only draw of the windowed rule (include/b4c.h, "Cloze batches over windows")
__host__ __device__ __forceinline__ uint64_t cloze_window_seed(uint64_t seed, uint64_t a) {
    return a == 0 ? seed : b4c_rand64(seed ^ 0x9E3779B97F4A7C15ull, a);
}
__host__ __device__ __forceinline__ bool cloze_last_only(uint64_t seed_a, uint64_t g, int L, uint32_t last_thr) {
    return L > 0 && (uint32_t)(b4c_rand64(seed_a ^ 0xD1B54A32D192ED03ull, g) >> 40) < last_thr;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
// The three phases of one row over src[0 .. L): draw = the n smallest (key, position) pairs of (key_seed, g) are masked,
// otherwise position L - 1 is (n = 1; n = 0 for L = 0).
__device__ __forceinline__ void cloze_row(const int32_t *__restrict__ src, uint64_t key_seed, uint64_t g, int L, int n, bool draw, int W,
                                          int64_t *__restrict__ row, float *__restrict__ lab, int M) {
    __shared__ uint64_t keys[1024];
    __shared__ uint8_t chosen[1024];
    const int tid = threadIdx.x;
    if (draw) {
        for (int p = tid; p < L; p += ROW_THREADS) keys[p] = cloze_key(key_seed, g, p);
        __syncthreads();
        for (int p = tid; p < L; p += ROW_THREADS) chosen[p] = cloze_chosen(keys, L, p, n) ? 1 : 0;
    } else {
        for (int p = tid; p < L; p += ROW_THREADS) chosen[p] = p == L - 1 ? 1 : 0;
    }
    __syncthreads();
    for (int p = tid; p < W; p += ROW_THREADS) {
        int64_t id = ROW_INPUT_PAD;
        if (p < L) {
            const int item = src[p];
            if (chosen[p]) {
                int slot = 0;
                for (int q = 0; q < p; ++q) slot += chosen[q];
                if (slot < M) lab[slot] = (float)item;
                id = ROW_MASK_ID;
            } else {
                id = (int64_t)item + ROW_RESERVED;
            }
        }
        row[p] = id;
    }
    for (int s = n + tid; s < M; s += ROW_THREADS) lab[s] = CLOZE_LABEL_PAD;
}

__global__ void __launch_bounds__(ROW_THREADS) cloze_batch_kernel(const int32_t *__restrict__ items, const int64_t *__restrict__ offsets,
                                                                    const int32_t *__restrict__ seq_idx, int W, int mode,
                                                                    float masked_percentage, int max_masked, uint64_t seed,
                                                                    int64_t *__restrict__ items_out, int ld_items,
                                                                    float *__restrict__ labels_out, int ld_lab, int M,
                                                                    int32_t *__restrict__ n_masked_out) {
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
    cloze_row(items + o0, seed, (uint64_t)g, L, n, mode == 0, W, items_out + b * (int64_t)ld_items, labels_out + b * (int64_t)ld_lab, M);
    if (n_masked_out && threadIdx.x == 0) n_masked_out[b] = n;
}

// one row per window (g, a, L): the window fetch and the last-only draw in front of the same three phases
__global__ void __launch_bounds__(ROW_THREADS) cloze_window_kernel(const int32_t *__restrict__ items, const int64_t *__restrict__ offsets,
                                                                     const int32_t *__restrict__ win_seq, const int32_t *__restrict__ win_start,
                                                                     const int32_t *__restrict__ win_len, const int32_t *__restrict__ row_win,
                                                                     int W, int mode, float masked_percentage, int max_masked, uint64_t seed,
                                                                     uint32_t last_thr, int64_t *__restrict__ items_out, int ld_items,
                                                                     float *__restrict__ labels_out, int ld_lab, int M,
                                                                     int32_t *__restrict__ n_masked_out) {
    const int64_t b = blockIdx.x;
    const RowWindow win = row_window(row_win, win_seq, win_start, win_len, offsets, b, true);
    const BatchRow r = batch_row_rule(B4C_FEAT_CLOZE, win.a, win.len, win.n_g, 0, 0, W);
    const int L = r.n;
    const uint64_t g = (uint64_t)win.g;
    bool draw = false;
    uint64_t seed_a = seed;
    int n = L > 0 ? 1 : 0;                                     // EVAL and last-only rows: position L - 1
    if (mode == 0) {
        seed_a = cloze_window_seed(seed, (uint64_t)win.a);
        draw = !cloze_last_only(seed_a, g, L, last_thr);
        if (draw) n = cloze_n_masked(L, masked_percentage, max_masked);
    }
    cloze_row(items + win.o0 + r.first, seed_a, g, L, n, draw, W, items_out + b * (int64_t)ld_items, labels_out + b * (int64_t)ld_lab, M);
    if (n_masked_out && threadIdx.x == 0) n_masked_out[b] = n;
}

// out[b][e] = the e-th of the most recent E items in front of sequence seq_idx[b]'s target, -1 past them: a gather
__global__ void __launch_bounds__(ROW_THREADS) cloze_history_kernel(const int32_t *__restrict__ items, const int64_t *__restrict__ offsets,
                                                                      const int32_t *__restrict__ seq_idx, int drop, int E,
                                                                      int32_t *__restrict__ out, int ld) {
    const int64_t b = blockIdx.x;
    const int64_t g = seq_idx[b];
    int64_t o0 = 0, H = 0;
    if (g >= 0) {
        o0 = offsets[g];
        H = offsets[g + 1] - o0 - drop;
    }
    if (H < 0) H = 0;
    if (H > E) {                                               // the most recent E
        o0 += H - E;
        H = E;
    }
    int32_t *row = out + b * (int64_t)ld;
    for (int e = threadIdx.x; e < E; e += ROW_THREADS) row[e] = e < H ? items[o0 + e] : -1;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------
// what b4c_cloze_batch and b4c_cloze_batch_windows check alike
static int cloze_check_args(const char *who, int B, int W, int mode, float masked_percentage, int max_masked, int ld_items, int ld_lab, int M) {
    if (const int rc = rows_check_args(who, B, W, ld_items, B4C_FEAT_CLOZE, 0, 0, 0)) return rc;
    B4C_REQUIRE(mode == 0 || mode == 1, "%s: mode %d (0 = TRAIN, 1 = EVAL)", who, mode);
    B4C_REQUIRE(M >= mode && M <= B4C_MAX_CLOZE_LABELS, "%s: M = %d (%d .. %d)", who, M, mode, B4C_MAX_CLOZE_LABELS);      // EVAL masks one position
    B4C_REQUIRE(mode == 1 || (max_masked >= 0 && max_masked <= M), "%s: max_masked = %d (0 .. M = %d)", who, max_masked, M);
    B4C_REQUIRE(mode == 1 || (masked_percentage >= 0.f && masked_percentage <= 1.f), "%s: masked_percentage %g outside [0, 1]", who,
                (double)masked_percentage);
    B4C_REQUIRE(ld_lab >= M, "%s: ld_lab = %d < M = %d", who, ld_lab, M);
    return B4C_OK;
}

extern "C" int b4c_cloze_batch(const int32_t *items, const int64_t *offsets, const int32_t *seq_idx, int B, int W, int mode,
                               float masked_percentage, int max_masked, uint64_t seed, int64_t *items_out, int ld_items,
                               float *labels_out, int ld_lab, int M, int32_t *n_masked_out, void *stream) {
    if (const int rc = cloze_check_args("cloze_batch", B, W, mode, masked_percentage, max_masked, ld_items, ld_lab, M)) return rc;
    if (B == 0) return B4C_OK;
    B4C_REQUIRE(items && offsets && seq_idx && items_out && (labels_out || M == 0), "cloze_batch: null pointer");
    cloze_batch_kernel<<<(unsigned)B, ROW_THREADS, 0, (hipStream_t)stream>>>(items, offsets, seq_idx, W, mode, masked_percentage,
                                                                              max_masked, seed, items_out, ld_items, labels_out,
                                                                              ld_lab, M, n_masked_out);
    return b4c_check_launch("cloze_batch");
}

// the TRAIN rule on the host: the n positions of [0, L) that the kernel masks for sequence g, ascending
extern "C" int b4c_cloze_choose(uint64_t seed, int64_t g, int L, int n, int32_t *pos) {
    B4C_REQUIRE(L >= 0 && L <= B4C_MAX_BATCH_WIDTH && n >= 0 && n <= L, "cloze_choose: L = %d (0 .. %d), n = %d (0 .. L)", L, B4C_MAX_BATCH_WIDTH, n);
    B4C_REQUIRE(g >= 0 && g < ((int64_t)1 << 54), "cloze_choose: g = %lld (0 .. 2^54)", (long long)g);
    B4C_REQUIRE(pos || n == 0, "cloze_choose: null pointer");
    uint64_t keys[1024];
    for (int p = 0; p < L; ++p) keys[p] = cloze_key(seed, (uint64_t)g, p);
    int k = 0;
    for (int p = 0; p < L && k < n; ++p)
        if (cloze_chosen(keys, L, p, n)) pos[k++] = p;
    return B4C_OK;
}

extern "C" int b4c_cloze_batch_windows(const int32_t *items, const int64_t *offsets, const int32_t *win_seq, const int32_t *win_start,
                                       const int32_t *win_len, const int32_t *row_win, int B, int W, int mode, float masked_percentage,
                                       int max_masked, uint64_t seed, uint32_t last_thr, int64_t *items_out, int ld_items,
                                       float *labels_out, int ld_lab, int M, int32_t *n_masked_out, void *stream) {
    if (const int rc = cloze_check_args("cloze_batch_windows", B, W, mode, masked_percentage, max_masked, ld_items, ld_lab, M)) return rc;
    B4C_REQUIRE(mode == 1 || last_thr <= (1u << 24), "cloze_batch_windows: last_thr = %u (0 .. 2^24 = %u)", last_thr, 1u << 24);
    B4C_REQUIRE(mode == 1 || last_thr == 0 || M >= 1, "cloze_batch_windows: last_thr = %u needs M >= 1 (a last-only row has one label), M = %d",
                last_thr, M);
    if (B == 0) return B4C_OK;
    B4C_REQUIRE(items && offsets && items_out && (labels_out || M == 0), "cloze_batch_windows: null pointer");
    if (const int rc = rows_check_table("cloze_batch_windows", B, B4C_FEAT_CLOZE, win_seq, win_start, win_len)) return rc;
    cloze_window_kernel<<<(unsigned)B, ROW_THREADS, 0, (hipStream_t)stream>>>(items, offsets, win_seq, win_start, win_len, row_win, W, mode,
                                                                               masked_percentage, max_masked, seed, last_thr, items_out,
                                                                               ld_items, labels_out, ld_lab, M, n_masked_out);
    return b4c_check_launch("cloze_batch_windows");
}

// the TRAIN rule of one window on the host: the masked positions of [0, L), ascending, and their count
extern "C" int b4c_cloze_choose_window(uint64_t seed, int64_t g, int64_t a, int L, float masked_percentage, int max_masked, uint32_t last_thr,
                                       int32_t *pos, int32_t *n_out) {
    B4C_REQUIRE(L >= 0 && L <= B4C_MAX_BATCH_WIDTH, "cloze_choose_window: L = %d (0 .. %d)", L, B4C_MAX_BATCH_WIDTH);
    B4C_REQUIRE(g >= 0 && g < ((int64_t)1 << 54) && a >= 0, "cloze_choose_window: g = %lld (0 .. 2^54), a = %lld (>= 0)", (long long)g, (long long)a);
    B4C_REQUIRE(max_masked >= 0 && max_masked <= B4C_MAX_CLOZE_LABELS && masked_percentage >= 0.f && masked_percentage <= 1.f,
                "cloze_choose_window: max_masked = %d (0 .. %d), masked_percentage %g (0 .. 1)", max_masked, B4C_MAX_CLOZE_LABELS, (double)masked_percentage);
    B4C_REQUIRE(last_thr <= (1u << 24), "cloze_choose_window: last_thr = %u (0 .. 2^24 = %u)", last_thr, 1u << 24);
    B4C_REQUIRE(pos && n_out, "cloze_choose_window: null pointer");
    const uint64_t seed_a = cloze_window_seed(seed, (uint64_t)a);
    if (cloze_last_only(seed_a, (uint64_t)g, L, last_thr)) {
        pos[0] = L - 1;
        n_out[0] = 1;
        return B4C_OK;
    }
    const int n = cloze_n_masked(L, masked_percentage, max_masked);
    uint64_t keys[1024];
    for (int p = 0; p < L; ++p) keys[p] = cloze_key(seed_a, (uint64_t)g, p);
    int k = 0;
    for (int p = 0; p < L && k < n; ++p)
        if (cloze_chosen(keys, L, p, n)) pos[k++] = p;
    n_out[0] = n;
    return B4C_OK;
}

extern "C" int b4c_cloze_history(const int32_t *items, const int64_t *offsets, const int32_t *seq_idx, int B, int drop, int E, int32_t *out,
                                 int ld, void *stream) {
    B4C_REQUIRE(B >= 0 && drop >= 1, "cloze_history: B = %d, drop = %d (>= 1)", B, drop);
    B4C_REQUIRE(E >= 1 && E <= B4C_MAX_EXCL && ld >= E, "cloze_history: E = %d (1 .. %d), ld = %d (>= E)", E, B4C_MAX_EXCL, ld);
    if (B == 0) return B4C_OK;
    B4C_REQUIRE(items && offsets && seq_idx && out, "cloze_history: null pointer");
    cloze_history_kernel<<<(unsigned)B, ROW_THREADS, 0, (hipStream_t)stream>>>(items, offsets, seq_idx, drop, E, out, ld);
    return b4c_check_launch("cloze_history");
}
