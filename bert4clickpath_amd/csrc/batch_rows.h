// What a row of a device-built batch is, for the three builders that must agree on it: cloze_batch.hip (windows), next_item_batch.hip
// and batch_features.hip -- a side feature sits beside the right item because all three call the functions below.
#pragma once
#include "common.h"

#define ROW_THREADS 256      // one workgroup per batch row
#define ROW_RESERVED 10      // NUM_RESERVED_TOKENS: id = item index (feature value) + 10
#define ROW_MASK_ID 1
#define ROW_INPUT_PAD 0

// The layouts are b4c_batch_features' codes (B4C_FEAT_*).  That of a next-item mode, one of two: a kernel that says so carries no Cloze branch.
__host__ __device__ __forceinline__ int next_item_layout(int mode) { return mode == B4C_NEXT_TRAIN ? B4C_FEAT_NEXT_TRAIN : B4C_FEAT_NEXT_EVAL; }

// ---- the window fetch --------------------------------------------------------------------------------------------------------
struct RowWindow {
    int64_t g, a;      // the sequence (-1: an empty row) and the window's start inside it
    int len;           // the window's items; 0 where the table is not read
    int64_t o0, n_g;   // offsets[g] and the sequence's length
};
// Row b names window (table) or sequence (no table) row_win[b], or b itself without row_win.  A negative index, or a negative g or
// start in the table, is an empty row: g = -1 and everything else 0, of which every layout's rule makes n = 0.  (The start is part
// of the test so that the table's entries are loaded together, in front of it, and offsets[g] is the only load behind them.)
__device__ __forceinline__ RowWindow row_window(const int32_t *__restrict__ row_win, const int32_t *__restrict__ win_seq,
                                                const int32_t *__restrict__ win_start, const int32_t *__restrict__ win_len,
                                                const int64_t *__restrict__ offsets, int64_t b, bool table) {
    const RowWindow empty = {-1, 0, 0, 0, 0};
    const int64_t w = row_win ? (int64_t)row_win[b] : b;
    if (w < 0) return empty;
    RowWindow r = {w, 0, 0, 0, 0};
    if (table) {
        r.g = win_seq[w];
        r.a = win_start[w];
        r.len = win_len[w];
    }
    if (r.g < 0 || r.a < 0) return empty;
    r.o0 = offsets[r.g];
    r.n_g = offsets[r.g + 1] - r.o0;
    return r;
}

// ---- the rule: shared by the kernels and the host entries ----------------------------------------------------------------------
struct BatchRow {
    int64_t first;   // token p of the row is s_g[first + p]
    int n;           // tokens (the next-item layouts: inputs)
    int p_lo;        // next-item: the targets sit at the input positions p_lo .. n
    int view;        // next-item: X_g is drawn from s_g[max(0, view - B4C_MAX_EXCL) .. view)
};
__host__ __device__ __forceinline__ BatchRow batch_row_rule(int layout, int64_t a, int L, int64_t n_g, int holdout, int max_len, int W) {
    BatchRow r = {0, 0, 0, 0};
    if (layout == B4C_FEAT_CLOZE) {
        r.first = a;
        r.n = L < 0 || a < 0 ? 0 : (L > W ? W : L);             // clamped: nothing leaves the row
    } else if (layout == B4C_FEAT_NEXT_TRAIN) {
        const int64_t T = n_g - holdout > 0 ? n_g - holdout : 0;
        const int64_t first = a > 0 ? a - 1 : 0;
        int64_t n = a > 0 ? L : (L > 1 ? L - 1 : 0);
        if (n > W) n = W;
        if (n > T - first - 1) n = T - first - 1;              // a target never leaves the view
        if (n < 0 || a < 0) n = 0;
        r.first = first;
        r.n = (int)n;
        r.view = (int)T;
    } else {
        const int64_t t = n_g - holdout;
        int64_t n = t < 1 ? 0 : t;
        if (n > max_len) n = max_len;
        if (n > W) n = W;
        r.first = t < 1 ? 0 : t - n;
        r.n = (int)n;
        r.p_lo = n > 0 ? (int)n - 1 : 0;
        r.view = (int)(t < 0 ? 0 : t);
    }
    return r;
}

// ---- what every builder's entry point checks; `who` is its name in the message ------------------------------------------------------
// holdout_min: the least holdout / drop of a next-item layout (the Cloze layout reads neither holdout nor max_len)
static int rows_check_args(const char *who, int B, int W, int ld_items, int layout, int holdout, int holdout_min, int max_len) {
    B4C_REQUIRE(B >= 0 && W >= 1 && W <= B4C_MAX_BATCH_WIDTH, "%s: B = %d, W = %d (1 .. %d)", who, B, W, B4C_MAX_BATCH_WIDTH);
    B4C_REQUIRE(layout == B4C_FEAT_CLOZE || layout == B4C_FEAT_NEXT_TRAIN || layout == B4C_FEAT_NEXT_EVAL,
                "%s: layout %d (0 = CLOZE, 1 = NEXT_TRAIN, 2 = NEXT_EVAL)", who, layout);
    B4C_REQUIRE(layout == B4C_FEAT_CLOZE || holdout >= holdout_min, "%s: holdout / drop = %d (>= %d)", who, holdout, holdout_min);
    B4C_REQUIRE(layout != B4C_FEAT_NEXT_EVAL || max_len >= 1, "%s: max_len = %d (NEXT_EVAL: >= 1)", who, max_len);
    B4C_REQUIRE(ld_items >= W, "%s: ld_items = %d < W = %d", who, ld_items, W);
    return B4C_OK;
}
// the window table of a launch that reads it
static int rows_check_table(const char *who, int B, int layout, const int32_t *win_seq, const int32_t *win_start, const int32_t *win_len) {
    B4C_REQUIRE(B == 0 || layout == B4C_FEAT_NEXT_EVAL || (win_seq && win_start && win_len), "%s: null pointer (window table)", who);
    return B4C_OK;
}
