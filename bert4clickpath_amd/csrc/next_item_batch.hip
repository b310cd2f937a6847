// Next-item batches built on the device (include/b4c_next_item.h): per window the unmasked input row, the compact positions and
// shifted targets of every real position, and each target's own negatives -- none of them an item of the sequence.
//
// One 256-thread workgroup per batch row, four phases:
//   1. the window fetch and the rule's arithmetic (next_item_rule, shared with the host entry);
//   2. X_g, the at most 1024 items of the sequence's view, goes to LDS and is rank-sorted there by counting (duplicates kept: a
//      lower-bound search finds an item whether it is there once or five times) -- O(n^2) LDS broadcasts, 40 k at n = 200;
//   3. every thread writes its columns of the input row and its targets' flat_idx / labels;
//   4. the four waves take the row's targets in turn, one wave per target: b4c_sample_candidates' rule (64 attempts per step, the
//      accepted set in a per-wave LDS hash table, an earlier lane of the step wins a tie, acceptance order through a ballot
//      prefix count) against the SHARED sorted set.  Waves run different numbers of targets and steps: inside phase 4 only
//      wave-level ordering is used (LDS is in order per wave), never a workgroup barrier.
// The tail rows R .. rows of the compact outputs are written by the workgroups in turn.  Integer work beside a training step of
// milliseconds; nothing here is tuned further.
#include "common.h"

#define NEXT_MAX_W 1021      // S = W + 3 <= 1024, as the Cloze batches
#define NEXT_THREADS 256
#define NEXT_WAVES (NEXT_THREADS / 64)
#define NEXT_RESERVED 10     // NUM_RESERVED_TOKENS: input id = item index + 10
#define NEXT_INPUT_PAD 0

// ---- the rule: shared by the kernel and the host entry ---------------------------------------------------------------------
struct NextRow {
    int first;   // s_g[first + p] is input p
    int n_in;    // inputs
    int p_lo;    // the targets sit at the input positions p_lo .. n_in
    int view;    // X_g is drawn from s_g[max(0, view - B4C_MAX_EXCL) .. view)
};
__host__ __device__ __forceinline__ NextRow next_item_rule(int mode, int64_t a, int L, int64_t n_g, int holdout, int max_len, int W) {
    NextRow r = {0, 0, 0, 0};
    if (mode == B4C_NEXT_TRAIN) {
        const int64_t T = n_g - holdout > 0 ? n_g - holdout : 0;
        const int64_t first = a > 0 ? a - 1 : 0;
        int64_t n_in = a > 0 ? L : (L > 1 ? L - 1 : 0);
        if (n_in > W) n_in = W;
        if (n_in > T - first - 1) n_in = T - first - 1;        // a target never leaves the view
        if (n_in < 0 || a < 0) n_in = 0;
        r.first = (int)first;
        r.n_in = (int)n_in;
        r.view = (int)T;
    } else {
        const int64_t t = n_g - holdout;
        int64_t n_in = t < 1 ? 0 : t;
        if (n_in > max_len) n_in = max_len;
        if (n_in > W) n_in = W;
        r.first = (int)(t < 1 ? 0 : t - n_in);
        r.n_in = (int)n_in;
        r.p_lo = n_in > 0 ? (int)n_in - 1 : 0;
        r.view = (int)(t < 0 ? 0 : t);
    }
    return r;
}
// attempt j of the target token at CSR index i
__host__ __device__ __forceinline__ uint64_t next_item_draw(uint64_t seed, uint64_t i, uint32_t j) { return b4c_rand64(seed, (i << 20) | j); }
__host__ __device__ __forceinline__ uint64_t next_mulhi64(uint64_t x, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(x, v);
#else
    return (uint64_t)(((unsigned __int128)x * v) >> 64);
#endif
}
// the drawn item: uniform mulhi64(x, V), or min{i : cdf[i] > mulhi64(x, total)}; -1 when the cdf has no mass
__host__ __device__ __forceinline__ int next_item_of(uint64_t x, int V, const int64_t *cdf, uint64_t total) {
    if (!cdf) return (int)next_mulhi64(x, (uint64_t)V);
    if ((int64_t)total <= 0) return -1;
    const uint64_t u = next_mulhi64(x, total);
    int lo = 0, hi = V - 1;                                    // cdf[V - 1] = total > u
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint64_t)cdf[mid] > u) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// ---- LDS sets --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int next_hash_slot(int item, int hb) { return (int)(((uint32_t)item * 2654435761u) >> (32 - hb)); }
static inline int next_hash_bits(int n) {                      // at least 64 slots, at most half full
    int hb = 6;
    while ((1 << hb) < 2 * n) ++hb;
    return hb;
}
__device__ __forceinline__ bool next_hash_has(const int *tab, int hb, int item) {
    for (int s = next_hash_slot(item, hb);; s = (s + 1) & ((1 << hb) - 1)) {
        const int v = tab[s];
        if (v == item) return true;
        if (v < 0) return false;
    }
}
__device__ __forceinline__ void next_hash_put(int *tab, int hb, int item) {
    for (int s = next_hash_slot(item, hb);; s = (s + 1) & ((1 << hb) - 1))
        if (atomicCAS(&tab[s], -1, item) == -1) return;
}
__device__ __forceinline__ bool next_sorted_has(const int *sx, int n, int item) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sx[mid] < item) lo = mid + 1; else hi = mid;
    }
    return lo < n && sx[lo] == item;
}
// one wave's LDS writes are visible to its own later reads: order them for the compiler, the hardware keeps a wave's LDS in order
__device__ __forceinline__ void next_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one target's list by one wave: out[0] = y, then the negatives
__device__ __forceinline__ void next_sample_wave(const int *sx, int nx, int *tab, int hb, int y, int V, int N, uint64_t seed, uint64_t i,
                                                 const int64_t *__restrict__ cdf, uint64_t total, int32_t *__restrict__ out,
                                                 int32_t *__restrict__ short_count, int lane) {
    if (y < 0 || y >= V) {
        for (int p = lane; p <= N; p += 64) out[p] = -1;
        return;
    }
    for (int s = lane; s < (1 << hb); s += 64) tab[s] = -1;
    next_wave_sync();
    int count = 0;
    for (int t = 0; t < N && count < N; ++t) {
        const int item = next_item_of(next_item_draw(seed, i, (uint32_t)(t * 64 + lane)), V, cdf, total);
        bool ok = item >= 0 && item != y && !next_sorted_has(sx, nx, item) && !next_hash_has(tab, hb, item);
        const int mine = ok ? item : -1;
#pragma unroll 8
        for (int l = 0; l < 63; ++l) {                           // an earlier lane of the step with the same item comes first
            const int v = __builtin_amdgcn_readlane(mine, l);
            if (l < lane && v == item) ok = false;
        }
        const uint64_t m = __ballot(ok);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (ok && count + pre < N) {
            out[1 + count + pre] = item;
            next_hash_put(tab, hb, item);
        }
        count += __popcll(m);
        next_wave_sync();
    }
    if (count > N) count = N;
    for (int p = 1 + count + lane; p <= N; p += 64) out[p] = -1;
    if (lane == 0) {
        out[0] = y;
        if (count < N) atomicAdd(short_count, 1);
    }
}

// ---- kernel ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NEXT_THREADS) next_item_kernel(
    const int32_t *__restrict__ items, const int64_t *__restrict__ offsets, const int32_t *__restrict__ win_seq,
    const int32_t *__restrict__ win_start, const int32_t *__restrict__ win_len, const int32_t *__restrict__ row_win,
    const int32_t *__restrict__ row_off, int B, int W, int mode, int holdout, int max_len, int V, int N, uint64_t seed, int excl,
    const int64_t *__restrict__ cdf, int64_t *__restrict__ items_out, int ld_items, int32_t *__restrict__ flat_idx,
    int32_t *__restrict__ labels, int32_t *__restrict__ cand, int ld_c, int64_t rows, int32_t *__restrict__ short_count, int hb) {
    extern __shared__ int next_lds[];
    int *raw = next_lds, *sx = next_lds + B4C_MAX_EXCL, *tabs = next_lds + 2 * B4C_MAX_EXCL;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    // 1. the window and the rule
    const int64_t w = row_win ? (int64_t)row_win[b] : b;
    int64_t g = -1, a = 0;
    int len = 0;
    if (w >= 0) {
        if (mode == B4C_NEXT_TRAIN) {
            g = win_seq[w];
            a = win_start[w];
            len = win_len[w];
        } else {
            g = w;
        }
    }
    int64_t o0 = 0, n_g = 0;
    if (g >= 0) {
        o0 = offsets[g];
        n_g = offsets[g + 1] - o0;
    }
    const NextRow r = next_item_rule(mode, a, len, n_g, holdout, max_len, W);
    const int32_t *src = items + o0;
    // 2. X_g, sorted, in LDS (N == 0: nobody reads it)
    int nx = 0;
    if (N > 0 && excl == B4C_NEXT_EXCL_HISTORY) {
        nx = r.view > B4C_MAX_EXCL ? B4C_MAX_EXCL : r.view;
        const int x0 = r.view - nx;
        for (int e = tid; e < nx; e += NEXT_THREADS) raw[e] = src[x0 + e];
        __syncthreads();
        for (int e = tid; e < nx; e += NEXT_THREADS) {
            const int v = raw[e];
            int c = 0;
            for (int q = 0; q < nx; ++q) {
                const int u = raw[q];
                c += (u < v || (u == v && q < e)) ? 1 : 0;
            }
            sx[c] = v;
        }
    }
    // 3. the input row, the positions and the labels
    int64_t *row = items_out + b * (int64_t)ld_items;
    const int64_t r0 = row_off[b];
    const int S = W + 3;
    for (int p = tid; p < W; p += NEXT_THREADS) {
        int64_t id = NEXT_INPUT_PAD;
        if (p < r.n_in) {
            id = (int64_t)src[r.first + p] + NEXT_RESERVED;
            const int64_t cr = r0 + (p - r.p_lo);
            if (p >= r.p_lo && cr < rows) {
                flat_idx[cr] = (int32_t)(b * S + 2 + p);
                labels[cr] = src[r.first + p + 1];
            }
        }
        row[p] = id;
    }
    // the tail rows of the compact outputs, the workgroups in turn
    const int64_t R = row_off[B];
    for (int64_t cr = R + b; cr < rows; cr += B) {
        if (tid == 0) {
            flat_idx[cr] = -1;
            labels[cr] = -1;
        }
        if (N > 0)
            for (int p = tid; p <= N; p += NEXT_THREADS) cand[cr * (int64_t)ld_c + p] = -1;
    }
    if (N == 0) return;
    __syncthreads();                                           // sx is complete
    // 4. the negatives: one wave per target
    const int wave = tid >> 6, lane = tid & 63;
    int *tab = tabs + (wave << hb);
    const uint64_t total = cdf ? (uint64_t)cdf[V - 1] : 0;
    for (int p = r.p_lo + wave; p < r.n_in; p += NEXT_WAVES) {
        const int64_t cr = r0 + (p - r.p_lo);
        if (cr >= rows) break;
        const int y = src[r.first + p + 1];
        next_sample_wave(sx, nx, tab, hb, y, V, N, seed, (uint64_t)(o0 + r.first + p + 1), cdf, total, cand + cr * (int64_t)ld_c,
                         short_count, lane);
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------
extern "C" int b4c_next_item_batch(const int32_t *items, const int64_t *offsets, const int32_t *win_seq, const int32_t *win_start,
                                   const int32_t *win_len, const int32_t *row_win, const int32_t *row_off, int B, int W, int mode,
                                   int holdout, int max_len, int V, int N, uint64_t seed, int excl, const int64_t *cdf, int64_t *items_out,
                                   int ld_items, int32_t *flat_idx, int32_t *labels, int32_t *cand, int ld_c, int64_t rows,
                                   int32_t *short_count, void *stream) {
    B4C_REQUIRE(B >= 0 && W >= 1 && W <= NEXT_MAX_W, "next_item_batch: B = %d, W = %d (1 .. %d)", B, W, NEXT_MAX_W);
    B4C_REQUIRE(mode == B4C_NEXT_TRAIN || mode == B4C_NEXT_EVAL, "next_item_batch: mode %d (0 = TRAIN, 1 = EVAL)", mode);
    B4C_REQUIRE(excl == B4C_NEXT_EXCL_NONE || excl == B4C_NEXT_EXCL_HISTORY, "next_item_batch: excl %d (0 = none, 1 = history)", excl);
    B4C_REQUIRE(holdout >= 0 && (mode == B4C_NEXT_TRAIN || holdout >= 1), "next_item_batch: holdout / drop = %d (TRAIN: >= 0, EVAL: >= 1)",
                holdout);
    B4C_REQUIRE(mode == B4C_NEXT_TRAIN || max_len >= 1, "next_item_batch: max_len = %d (EVAL: >= 1)", max_len);
    B4C_REQUIRE(V > 0 && N >= 0 && N < B4C_MAX_CAND, "next_item_batch: V = %d, N = %d (0 .. %d)", V, N, B4C_MAX_CAND - 1);
    B4C_REQUIRE((int64_t)B * (W + 3) < ((int64_t)1 << 31), "next_item_batch: B (W + 3) = %lld does not fit flat_idx (int32)",
                (long long)B * (W + 3));
    B4C_REQUIRE(ld_items >= W && (N == 0 || ld_c >= N + 1), "next_item_batch: ld_items = %d < W = %d or ld_c = %d < N + 1 = %d", ld_items, W,
                ld_c, N + 1);
    B4C_REQUIRE(rows >= 0, "next_item_batch: rows = %lld", (long long)rows);
    B4C_REQUIRE(N == 0 || (cand && short_count), "next_item_batch: null pointer (cand / short_count with N = %d)", N);
    B4C_REQUIRE(B == 0 || (items && offsets && row_off && items_out && flat_idx && labels), "next_item_batch: null pointer");
    B4C_REQUIRE(B == 0 || mode == B4C_NEXT_EVAL || (win_seq && win_start && win_len), "next_item_batch: null pointer (window table)");
    B4C_REQUIRE(B == 0 || mode == B4C_NEXT_TRAIN || row_win, "next_item_batch: null pointer (row_win names the sequences of EVAL rows)");
    hipStream_t st = (hipStream_t)stream;
    if (short_count) (void)hipMemsetAsync(short_count, 0, 4, st);
    if (B == 0) return B4C_OK;
    const int hb = next_hash_bits(N);
    const size_t lds = N > 0 ? (size_t)(2 * B4C_MAX_EXCL + (NEXT_WAVES << hb)) * 4 : 0;
    next_item_kernel<<<(unsigned)B, NEXT_THREADS, lds, st>>>(items, offsets, win_seq, win_start, win_len, row_win, row_off, B, W, mode, holdout,
                                                             max_len, V, N, seed, excl, cdf, items_out, ld_items, flat_idx, labels, cand,
                                                             ld_c, rows, short_count, hb);
    return b4c_check_launch("next_item_batch");
}

// the rule of one row on the host
extern "C" int b4c_next_item_row(const int32_t *seq, int n_g, int64_t seq_off, int a, int L, int W, int mode, int holdout, int max_len, int V,
                                 int N, uint64_t seed, int excl, const int64_t *cdf, int64_t *inputs_out, int32_t *labels_out,
                                 int32_t *pos_out, int32_t *cand_out, int ld_c, int32_t *counts_out) {
    B4C_REQUIRE(W >= 1 && W <= NEXT_MAX_W && n_g >= 0 && seq_off >= 0, "next_item_row: W = %d (1 .. %d), n_g = %d, seq_off = %lld", W,
                NEXT_MAX_W, n_g, (long long)seq_off);
    B4C_REQUIRE(mode == B4C_NEXT_TRAIN || mode == B4C_NEXT_EVAL, "next_item_row: mode %d (0 = TRAIN, 1 = EVAL)", mode);
    B4C_REQUIRE(excl == B4C_NEXT_EXCL_NONE || excl == B4C_NEXT_EXCL_HISTORY, "next_item_row: excl %d (0 = none, 1 = history)", excl);
    B4C_REQUIRE(holdout >= 0 && (mode == B4C_NEXT_TRAIN || (holdout >= 1 && max_len >= 1)),
                "next_item_row: holdout / drop = %d, max_len = %d", holdout, max_len);
    B4C_REQUIRE(mode == B4C_NEXT_EVAL || (a >= 0 && L >= 0), "next_item_row: window (a = %d, L = %d)", a, L);
    B4C_REQUIRE(V > 0 && N >= 0 && N < B4C_MAX_CAND && (N == 0 || (cand_out && ld_c >= N + 1)),
                "next_item_row: V = %d, N = %d (0 .. %d), cand_out / ld_c = %d", V, N, B4C_MAX_CAND - 1, ld_c);
    B4C_REQUIRE((seq || n_g == 0) && inputs_out && labels_out && pos_out && counts_out, "next_item_row: null pointer");
    const NextRow r = next_item_rule(mode, a, L, n_g, holdout, max_len, W);
    for (int p = 0; p < W; ++p) inputs_out[p] = p < r.n_in ? (int64_t)seq[r.first + p] + NEXT_RESERVED : NEXT_INPUT_PAD;
    const int nx = excl == B4C_NEXT_EXCL_HISTORY ? (r.view > B4C_MAX_EXCL ? B4C_MAX_EXCL : r.view) : 0;
    const int32_t *xs = seq + (r.view - nx);
    const uint64_t total = cdf ? (uint64_t)cdf[V - 1] : 0;
    int n_t = 0, n_short = 0;
    for (int p = r.p_lo; p < r.n_in; ++p, ++n_t) {
        const int y = seq[r.first + p + 1];
        labels_out[n_t] = y;
        pos_out[n_t] = p;
        if (N == 0) continue;
        int32_t *out = cand_out + (int64_t)n_t * ld_c;
        for (int c = 0; c <= N; ++c) out[c] = -1;
        if (y < 0 || y >= V) continue;
        out[0] = y;
        const uint64_t i = (uint64_t)(seq_off + r.first + p + 1);
        int count = 0;
        for (uint32_t j = 0; j < 64u * (uint32_t)N && count < N; ++j) {
            const int item = next_item_of(next_item_draw(seed, i, j), V, cdf, total);
            bool ok = item >= 0 && item != y;
            for (int e = 0; ok && e < nx; ++e) ok = xs[e] != item;
            for (int c = 1; ok && c <= count; ++c) ok = out[c] != item;
            if (ok) out[++count] = item;
        }
        n_short += count < N ? 1 : 0;
    }
    counts_out[0] = r.n_in;
    counts_out[1] = n_t;
    counts_out[2] = n_short;
    return B4C_OK;
}
