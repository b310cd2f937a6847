// Side features beside the items of a device-built batch (include/b4c.h): per batch row the ids of up to four
// further features -- gathered by token (EVENT) or through the item (ITEM) -- with [MASK] copied from the item row where the
// feature asks for it.  A pure gather: B W 8 bytes read, n_feat B W 8 written, 4 n (1 + n_feat) gathered; no LDS, no atomics.
//
// One 256-thread workgroup per batch row.  The row's geometry is wave-uniform arithmetic on three or four scalar loads.  Lanes
// run along p, two columns each: the item row is read and every feature row written 16 bytes per lane where the row starts on a
// 16-byte boundary (an odd pitch puts every other row off it), 8 bytes per lane otherwise and for the last column of an odd W.
// The sources' pointers and codes travel by value in the kernel arguments; the feature loop is unrolled over B4C_MAX_FEATURES so
// that they are never indexed by a register.
#include "batch_rows.h"

// one column of one feature; value: the feature's value at the token (read only where p < n)
__host__ __device__ __forceinline__ int64_t feat_id(bool real, bool masked_here, int value) {
    return !real ? ROW_INPUT_PAD : (masked_here ? ROW_MASK_ID : (int64_t)value + ROW_RESERVED);
}

// ---- kernel ----------------------------------------------------------------------------------------------------------------
struct FeatArgs {
    const int32_t *src[B4C_MAX_FEATURES];
    int64_t *out[B4C_MAX_FEATURES];
    int kind[B4C_MAX_FEATURES];
    int on_mask[B4C_MAX_FEATURES];
};
struct alignas(16) FeatPair {
    int64_t x, y;
};

__global__ void __launch_bounds__(ROW_THREADS) batch_features_kernel(
    const int32_t *__restrict__ items, const int64_t *__restrict__ offsets, const int32_t *__restrict__ win_seq,
    const int32_t *__restrict__ win_start, const int32_t *__restrict__ win_len, const int32_t *__restrict__ row_win, int W, int layout,
    int holdout, int max_len, const int64_t *__restrict__ items_in, int ld_items, int n_feat, FeatArgs fa, int ld_out) {
    const int64_t b = blockIdx.x;
    // the row's geometry
    const RowWindow win = row_window(row_win, win_seq, win_start, win_len, offsets, b, layout != B4C_FEAT_NEXT_EVAL);
    const BatchRow r = batch_row_rule(layout, win.a, win.len, win.n_g, holdout, max_len, W);
    const int n = r.n;
    const int64_t base = win.o0 + r.first;                     // CSR index of the row's first token
    bool any_masked = false, any_item = false;
#pragma unroll
    for (int f = 0; f < B4C_MAX_FEATURES; ++f)
        if (f < n_feat) {
            any_masked |= fa.on_mask[f] == B4C_FEAT_MASKED;
            any_item |= fa.kind[f] == B4C_FEAT_ITEM;
        }
    const int64_t *in_row = items_in + b * (int64_t)ld_items;
    const bool in_vec = ((uintptr_t)in_row & 15) == 0;
    // two columns per lane
    for (int p0 = 2 * (int)threadIdx.x; p0 < W; p0 += 2 * ROW_THREADS) {
        const bool two = p0 + 1 < W;
        const bool real0 = p0 < n, real1 = p0 + 1 < n;         // (n <= W: real1 implies two)
        bool m0 = false, m1 = false;
        if (any_masked) {
            if (in_vec && two) {
                const FeatPair v = *reinterpret_cast<const FeatPair *>(in_row + p0);
                m0 = v.x == ROW_MASK_ID;
                m1 = v.y == ROW_MASK_ID;
            } else {
                m0 = in_row[p0] == ROW_MASK_ID;
                m1 = two && in_row[p0 + 1] == ROW_MASK_ID;
            }
        }
        int item0 = 0, item1 = 0;
        if (any_item) {
            if (real0) item0 = items[base + p0];
            if (real1) item1 = items[base + p0 + 1];
        }
#pragma unroll
        for (int f = 0; f < B4C_MAX_FEATURES; ++f) {
            if (f >= n_feat) break;
            const int32_t *__restrict__ src = fa.src[f];
            const bool by_item = fa.kind[f] == B4C_FEAT_ITEM;
            const bool masks = fa.on_mask[f] == B4C_FEAT_MASKED;
            int v0 = 0, v1 = 0;
            if (real0) v0 = src[by_item ? (int64_t)item0 : base + p0];
            if (real1) v1 = src[by_item ? (int64_t)item1 : base + p0 + 1];
            FeatPair o;
            o.x = feat_id(real0, masks && m0, v0);
            o.y = feat_id(real1, masks && m1, v1);
            int64_t *out_row = fa.out[f] + b * (int64_t)ld_out;
            if (two && ((uintptr_t)out_row & 15) == 0) {
                *reinterpret_cast<FeatPair *>(out_row + p0) = o;
            } else {
                out_row[p0] = o.x;
                if (two) out_row[p0 + 1] = o.y;
            }
        }
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------
extern "C" int b4c_batch_features(const int32_t *items, const int64_t *offsets, const int32_t *win_seq, const int32_t *win_start,
                                  const int32_t *win_len, const int32_t *row_win, int B, int W, int layout, int holdout, int max_len, int V,
                                  const int64_t *items_in, int ld_items, int n_feat, const int32_t *const *src, const int *kind,
                                  const int *on_mask, int64_t *const *out, int ld_out, void *stream) {
    if (const int rc = rows_check_args("batch_features", B, W, ld_items, layout, holdout, 1, max_len)) return rc;
    B4C_REQUIRE(n_feat >= 1 && n_feat <= B4C_MAX_FEATURES, "batch_features: n_feat = %d (1 .. %d)", n_feat, B4C_MAX_FEATURES);
    B4C_REQUIRE(ld_out >= W, "batch_features: ld_out = %d < W = %d", ld_out, W);
    if (B == 0) return B4C_OK;
    B4C_REQUIRE(items && offsets && items_in && src && kind && on_mask && out, "batch_features: null pointer");
    if (const int rc = rows_check_table("batch_features", B, layout, win_seq, win_start, win_len)) return rc;
    FeatArgs fa = {};
    for (int f = 0; f < n_feat; ++f) {
        B4C_REQUIRE(src[f] && out[f], "batch_features: null pointer (src / out of feature %d)", f);
        B4C_REQUIRE(kind[f] == B4C_FEAT_EVENT || kind[f] == B4C_FEAT_ITEM, "batch_features: kind %d of feature %d (0 = EVENT, 1 = ITEM)",
                    kind[f], f);
        B4C_REQUIRE(on_mask[f] == B4C_FEAT_MASKED || on_mask[f] == B4C_FEAT_KEPT, "batch_features: on_mask %d of feature %d (0 = MASKED, 1 = KEPT)",
                    on_mask[f], f);
        B4C_REQUIRE(kind[f] == B4C_FEAT_EVENT || V > 0, "batch_features: V = %d with the ITEM table of feature %d", V, f);
        fa.src[f] = src[f];
        fa.out[f] = out[f];
        fa.kind[f] = kind[f];
        fa.on_mask[f] = on_mask[f];
    }
    batch_features_kernel<<<(unsigned)B, ROW_THREADS, 0, (hipStream_t)stream>>>(items, offsets, win_seq, win_start, win_len, row_win, W, layout,
                                                                                holdout, max_len, items_in, ld_items, n_feat, fa, ld_out);
    return b4c_check_launch("batch_features");
}

// the rule of one row and one feature on the host
extern "C" int b4c_batch_features_row(const int32_t *seq, int n_g, int64_t seq_off, int a, int L, int W, int layout, int holdout, int max_len,
                                      int V, const int32_t *src, int kind, int on_mask, const int64_t *items_in, int64_t *out,
                                      int32_t *geom_out) {
    if (const int rc = rows_check_args("batch_features_row", 1, W, W, layout, holdout, 1, max_len)) return rc;
    B4C_REQUIRE(n_g >= 0 && seq_off >= 0, "batch_features_row: n_g = %d, seq_off = %lld", n_g, (long long)seq_off);
    B4C_REQUIRE(kind == B4C_FEAT_EVENT || kind == B4C_FEAT_ITEM, "batch_features_row: kind %d (0 = EVENT, 1 = ITEM)", kind);
    B4C_REQUIRE(on_mask == B4C_FEAT_MASKED || on_mask == B4C_FEAT_KEPT, "batch_features_row: on_mask %d (0 = MASKED, 1 = KEPT)", on_mask);
    B4C_REQUIRE(layout == B4C_FEAT_NEXT_EVAL || (a >= 0 && L >= 0), "batch_features_row: window (a = %d, L = %d)", a, L);
    B4C_REQUIRE(kind == B4C_FEAT_EVENT || V > 0, "batch_features_row: V = %d with an ITEM table", V);
    B4C_REQUIRE((seq || n_g == 0) && src && items_in && out && geom_out, "batch_features_row: null pointer");
    const BatchRow r = batch_row_rule(layout, a, L, n_g, holdout, max_len, W);
    B4C_REQUIRE(r.first + r.n <= n_g, "batch_features_row: the row [%lld, %lld) leaves its sequence of %d items", (long long)r.first,
                (long long)r.first + r.n, n_g);
    for (int p = 0; p < r.n; ++p)
        B4C_REQUIRE(kind == B4C_FEAT_EVENT || (seq[r.first + p] >= 0 && seq[r.first + p] < V), "batch_features_row: item %d outside [0, V = %d)",
                    seq[r.first + p], V);
    for (int p = 0; p < W; ++p) {
        const bool real = p < r.n;
        int value = 0;
        if (real) value = kind == B4C_FEAT_ITEM ? src[seq[r.first + p]] : src[seq_off + r.first + p];
        out[p] = feat_id(real, on_mask == B4C_FEAT_MASKED && items_in[p] == ROW_MASK_ID, value);
    }
    geom_out[0] = (int32_t)r.first;
    geom_out[1] = r.n;
    return B4C_OK;
}
