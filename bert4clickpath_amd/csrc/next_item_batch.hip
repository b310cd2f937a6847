// Next-item batches built on the device (include/b4c.h): per window the unmasked input row, the compact positions and
// shifted targets of every real position, and each target's own negatives -- none of them an item of the sequence.
//
// One 256-thread workgroup per batch row, four phases:
//   1. the window fetch and the rule's arithmetic (batch_rows.h: row_window, and batch_row_rule, shared with the host entry);
//   2. X_g, the at most 1024 items of the sequence's view, goes to LDS and is rank-sorted there by counting (duplicates kept: a
//      lower-bound search finds an item whether it is there once or five times) -- O(n^2) LDS broadcasts, 40 k at n = 200;
//   3. every thread writes its columns of the input row and its targets' flat_idx / labels;
//   4. the four waves take the row's targets in turn, one wave per target: b4c_sample_candidates' own draw loop (sampler.h, the
//      accepted set in a per-wave LDS hash table) against the SHARED sorted set.  Waves run different numbers of targets and
//      steps: inside phase 4 only wave-level ordering is used (LDS is in order per wave), never a workgroup barrier.
// The tail rows R .. rows of the compact outputs are written by the workgroups in turn.  Integer work beside a training step of
// milliseconds; nothing here is tuned further.
#include "batch_rows.h"
#include "sampler.h"

#define NEXT_WAVES (ROW_THREADS / 64)

// ---- kernel ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ROW_THREADS) next_item_kernel(
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
    const RowWindow win = row_window(row_win, win_seq, win_start, win_len, offsets, b, mode == B4C_NEXT_TRAIN);
    const BatchRow r = batch_row_rule(next_item_layout(mode), win.a, win.len, win.n_g, holdout, max_len, W);
    const int32_t *src = items + win.o0;
    // 2. X_g, sorted, in LDS (N == 0: nobody reads it)
    int nx = 0;
    if (N > 0 && excl == B4C_NEXT_EXCL_HISTORY) {
        nx = r.view > B4C_MAX_EXCL ? B4C_MAX_EXCL : r.view;
        const int x0 = r.view - nx;
        for (int e = tid; e < nx; e += ROW_THREADS) raw[e] = src[x0 + e];
        __syncthreads();
        for (int e = tid; e < nx; e += ROW_THREADS) {
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
    for (int p = tid; p < W; p += ROW_THREADS) {
        int64_t id = ROW_INPUT_PAD;
        if (p < r.n) {
            id = (int64_t)src[r.first + p] + ROW_RESERVED;
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
            for (int p = tid; p <= N; p += ROW_THREADS) cand[cr * (int64_t)ld_c + p] = -1;
    }
    if (N == 0) return;
    __syncthreads();                                           // sx is complete
    // 4. the negatives: one wave per target
    const int wave = tid >> 6, lane = tid & 63;
    int *tab = tabs + (wave << hb);
    const uint64_t total = cdf ? (uint64_t)cdf[V - 1] : 0;
    for (int p = r.p_lo + wave; p < r.n; p += NEXT_WAVES) {
        const int64_t cr = r0 + (p - r.p_lo);
        if (cr >= rows) break;
        const int y = src[r.first + p + 1];
        sampler_wave(sx, nx, tab, hb, y, V, N, seed, (uint64_t)(win.o0 + r.first + p + 1), cdf, total, cand + cr * (int64_t)ld_c,
                     short_count, lane);
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------
extern "C" int b4c_next_item_batch(const int32_t *items, const int64_t *offsets, const int32_t *win_seq, const int32_t *win_start,
                                   const int32_t *win_len, const int32_t *row_win, const int32_t *row_off, int B, int W, int mode,
                                   int holdout, int max_len, int V, int N, uint64_t seed, int excl, const int64_t *cdf, int64_t *items_out,
                                   int ld_items, int32_t *flat_idx, int32_t *labels, int32_t *cand, int ld_c, int64_t rows,
                                   int32_t *short_count, void *stream) {
    B4C_REQUIRE(mode == B4C_NEXT_TRAIN || mode == B4C_NEXT_EVAL, "next_item_batch: mode %d (0 = TRAIN, 1 = EVAL)", mode);
    const int layout = next_item_layout(mode);                 // (TRAIN rows may hold out nothing)
    if (const int rc = rows_check_args("next_item_batch", B, W, ld_items, layout, holdout, mode == B4C_NEXT_EVAL ? 1 : 0, max_len)) return rc;
    B4C_REQUIRE(excl == B4C_NEXT_EXCL_NONE || excl == B4C_NEXT_EXCL_HISTORY, "next_item_batch: excl %d (0 = none, 1 = history)", excl);
    B4C_REQUIRE(V > 0 && N >= 0 && N < B4C_MAX_CAND, "next_item_batch: V = %d, N = %d (0 .. %d)", V, N, B4C_MAX_CAND - 1);
    B4C_REQUIRE((int64_t)B * (W + 3) < ((int64_t)1 << 31), "next_item_batch: B (W + 3) = %lld does not fit flat_idx (int32)",
                (long long)B * (W + 3));
    B4C_REQUIRE(N == 0 || ld_c >= N + 1, "next_item_batch: ld_c = %d < N + 1 = %d", ld_c, N + 1);
    B4C_REQUIRE(rows >= 0, "next_item_batch: rows = %lld", (long long)rows);
    B4C_REQUIRE(N == 0 || (cand && short_count), "next_item_batch: null pointer (cand / short_count with N = %d)", N);
    B4C_REQUIRE(B == 0 || (items && offsets && row_off && items_out && flat_idx && labels), "next_item_batch: null pointer");
    if (const int rc = rows_check_table("next_item_batch", B, layout, win_seq, win_start, win_len)) return rc;
    B4C_REQUIRE(B == 0 || mode == B4C_NEXT_TRAIN || row_win, "next_item_batch: null pointer (row_win names the sequences of EVAL rows)");
    hipStream_t st = (hipStream_t)stream;
    if (short_count) (void)hipMemsetAsync(short_count, 0, 4, st);
    if (B == 0) return B4C_OK;
    const int hb = sampler_hash_bits(N);
    const size_t lds = N > 0 ? (size_t)(2 * B4C_MAX_EXCL + (NEXT_WAVES << hb)) * 4 : 0;
    next_item_kernel<<<(unsigned)B, ROW_THREADS, lds, st>>>(items, offsets, win_seq, win_start, win_len, row_win, row_off, B, W, mode, holdout,
                                                             max_len, V, N, seed, excl, cdf, items_out, ld_items, flat_idx, labels, cand,
                                                             ld_c, rows, short_count, hb);
    return b4c_check_launch("next_item_batch");
}

// the rule of one row on the host
extern "C" int b4c_next_item_row(const int32_t *seq, int n_g, int64_t seq_off, int a, int L, int W, int mode, int holdout, int max_len, int V,
                                 int N, uint64_t seed, int excl, const int64_t *cdf, int64_t *inputs_out, int32_t *labels_out,
                                 int32_t *pos_out, int32_t *cand_out, int ld_c, int32_t *counts_out) {
    B4C_REQUIRE(mode == B4C_NEXT_TRAIN || mode == B4C_NEXT_EVAL, "next_item_row: mode %d (0 = TRAIN, 1 = EVAL)", mode);
    const int layout = next_item_layout(mode);                 // (TRAIN rows may hold out nothing)
    if (const int rc = rows_check_args("next_item_row", 1, W, W, layout, holdout, mode == B4C_NEXT_EVAL ? 1 : 0, max_len)) return rc;
    B4C_REQUIRE(n_g >= 0 && seq_off >= 0, "next_item_row: n_g = %d, seq_off = %lld", n_g, (long long)seq_off);
    B4C_REQUIRE(excl == B4C_NEXT_EXCL_NONE || excl == B4C_NEXT_EXCL_HISTORY, "next_item_row: excl %d (0 = none, 1 = history)", excl);
    B4C_REQUIRE(mode == B4C_NEXT_EVAL || (a >= 0 && L >= 0), "next_item_row: window (a = %d, L = %d)", a, L);
    B4C_REQUIRE(V > 0 && N >= 0 && N < B4C_MAX_CAND && (N == 0 || (cand_out && ld_c >= N + 1)),
                "next_item_row: V = %d, N = %d (0 .. %d), cand_out / ld_c = %d", V, N, B4C_MAX_CAND - 1, ld_c);
    B4C_REQUIRE((seq || n_g == 0) && inputs_out && labels_out && pos_out && counts_out, "next_item_row: null pointer");
    const BatchRow r = batch_row_rule(layout, a, L, n_g, holdout, max_len, W);
    for (int p = 0; p < W; ++p) inputs_out[p] = p < r.n ? (int64_t)seq[r.first + p] + ROW_RESERVED : ROW_INPUT_PAD;
    const int nx = excl == B4C_NEXT_EXCL_HISTORY ? (r.view > B4C_MAX_EXCL ? B4C_MAX_EXCL : r.view) : 0;
    const int32_t *xs = seq + (r.view - nx);
    const uint64_t total = cdf ? (uint64_t)cdf[V - 1] : 0;
    int n_t = 0, n_short = 0;
    for (int p = r.p_lo; p < r.n; ++p, ++n_t) {
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
            const int item = sampler_item_of(sampler_draw(seed, i, j), V, cdf, total);
            bool ok = item >= 0 && item != y;
            for (int e = 0; ok && e < nx; ++e) ok = xs[e] != item;
            for (int c = 1; ok && c <= count; ++c) ok = out[c] != item;
            if (ok) out[++count] = item;
        }
        n_short += count < N ? 1 : 0;
    }
    counts_out[0] = r.n;
    counts_out[1] = n_t;
    counts_out[2] = n_short;
    return B4C_OK;
}
