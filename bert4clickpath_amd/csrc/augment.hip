// Contrastive views of a device-built batch (include/b4c.h, whose comment is the definition): per (row, view) one of item
// crop, item mask, item reorder (CL4SRec) or the row of another sequence in front of the same target item (DuoRec).
//
// One 256-thread workgroup per (row, view), grid (B, n_views).  The row's geometry (batch_rows.h) and the view's plan -- the op, its
// lengths and starts, the same-target partner found by two binary searches -- are wave-uniform arithmetic that every thread
// repeats.  MASK and REORDER put their keys in LDS (8 KB) and rank by counting, as cloze_row does; REORDER's span threads scatter
// their source positions through a second LDS array (4 KB).  Then every thread writes its columns.  The one atomic is self_count.
// O(n^2) compares per row at most: integer work beside a training step of milliseconds; nothing here is tuned further.
#include "batch_rows.h"
#include "sampler.h"

#define AUG_OPS (B4C_AUG_CROP | B4C_AUG_MASK | B4C_AUG_REORDER | B4C_AUG_SAME_TARGET)

// ---- the rule: shared by the kernel and the host entry ---------------------------------------------------------------------
struct AugParams {
    uint32_t ops_mask;
    float crop_ratio, mask_ratio, reorder_ratio;
    int layout, W, max_len, V;
    const int64_t *tgt_first, *tgt_tok;
    const int32_t *tgt_seq;
};
// What one (row, view) does.  Output position p < n_out comes from the token src0 + p, except inside REORDER's span.
struct AugPlan {
    uint32_t op;       // the op's bit; 0: an empty row
    int n_out;
    int at, len;       // MASK: len = m; REORDER: the span [at, at + len)
    int64_t src0;
    int self;          // a same-target row without a partner
    int target;
    uint64_t seed_v;
};
__host__ __device__ __forceinline__ uint64_t aug_view_seed(uint64_t seed, int v) { return b4c_rand64(seed ^ 0xA0761D6478BD642Full, (uint64_t)v); }
__host__ __device__ __forceinline__ uint64_t aug_key(uint64_t seed_v, uint64_t i, int p) { return b4c_rand64(seed_v, (i << 10) | (uint64_t)(uint32_t)p); }
// float32 product, then truncation (cloze_n_masked's form)
__host__ __device__ __forceinline__ int aug_share(int n, float ratio) {
    const int k = (int)((float)n * ratio);
    return k < 0 ? 0 : (k > n ? n : k);
}
// the e-th set bit of mask, ascending
__host__ __device__ __forceinline__ uint32_t aug_nth_bit(uint32_t mask, int e) {
    for (uint32_t bit = 1; bit <= B4C_AUG_SAME_TARGET; bit <<= 1)
        if ((mask & bit) && e-- == 0) return bit;
    return 0;
}
// entries of the ascending list[0 .. cnt) below t
__host__ __device__ __forceinline__ int64_t aug_lower_bound(const int64_t *list, int64_t cnt, int64_t t) {
    int64_t lo = 0, hi = cnt;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (list[mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// (ka, a) < (kb, b), lexicographic: cloze_batch.hip's order (cloze_before), ties of the key go to the lower position
__host__ __device__ __forceinline__ bool aug_before(uint64_t ka, int a, uint64_t kb, int b) { return ka < kb || (ka == kb && a < b); }
// (k_q, q) pairs of the span [lo, hi) in front of (k_p, p); keys is indexed by position
__host__ __device__ __forceinline__ int aug_rank(const uint64_t *keys, int lo, int hi, int p) {
    const uint64_t kp = keys[p];
    int c = 0;
    for (int q = lo; q < hi; ++q) c += aug_before(keys[q], q, kp, p) ? 1 : 0;
    return c;
}

// i: the CSR index of the row's first token, n: its tokens (batch_row_rule)
__host__ __device__ __forceinline__ AugPlan aug_plan(const int32_t *__restrict__ items, const int64_t *__restrict__ offsets, int64_t i, int n,
                                                     uint64_t seed, int v, const AugParams &P) {
    AugPlan pl = {0, 0, 0, 0, i, 0, -1, 0};
    if (n <= 0) return pl;
    pl.seed_v = aug_view_seed(seed, v);
    const uint64_t h_op = b4c_rand64(pl.seed_v ^ 0xE7037ED1A0B428DBull, (uint64_t)i);
    const uint64_t h_at = b4c_rand64(pl.seed_v ^ 0x8EBC6AF09C88C6E3ull, (uint64_t)i);
    int m = 0;
    for (uint32_t bit = 1; bit <= B4C_AUG_SAME_TARGET; bit <<= 1) m += (P.ops_mask & bit) ? 1 : 0;
    pl.op = aug_nth_bit(P.ops_mask, (int)sampler_mulhi64(h_op, (uint64_t)m));
    pl.n_out = n;
    if (P.layout == B4C_FEAT_NEXT_TRAIN) pl.target = items[i + n];
    if (pl.op == B4C_AUG_CROP) {
        const int Lc = aug_share(n, P.crop_ratio) < 1 ? 1 : aug_share(n, P.crop_ratio);
        pl.src0 = i + (int64_t)sampler_mulhi64(h_at, (uint64_t)(n - Lc + 1));
        pl.n_out = Lc;
    } else if (pl.op == B4C_AUG_MASK) {
        pl.len = aug_share(n, P.mask_ratio);
    } else if (pl.op == B4C_AUG_REORDER) {
        pl.len = aug_share(n, P.reorder_ratio);
        pl.at = (int)sampler_mulhi64(h_at, (uint64_t)(n - pl.len + 1));
    } else {
        const int64_t t = i + n;
        const int y = pl.target;
        int64_t lo = 0, cnt = 0;
        if (y >= 0 && y < P.V) {
            lo = P.tgt_first[y];
            cnt = P.tgt_first[y + 1] - lo;
        }
        const int64_t own = aug_lower_bound(P.tgt_tok + lo, cnt, t);
        const bool found = own < cnt && P.tgt_tok[lo + own] == t;
        const int64_t others = cnt - (found ? 1 : 0);
        if (others <= 0) {
            pl.self = 1;
        } else {
            const int64_t u = (int64_t)sampler_mulhi64(h_at, (uint64_t)others);
            const int64_t k = lo + u + (found && u >= own ? 1 : 0);
            const int64_t j = P.tgt_tok[k];
            int64_t q = j - offsets[P.tgt_seq[k]];
            if (q < 0) q = 0;
            int64_t no = q < P.W ? q : P.W;
            if (P.max_len > 0 && no > P.max_len) no = P.max_len;
            pl.n_out = (int)no;
            pl.src0 = j - no;
        }
    }
    return pl;
}

// ---- kernel ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ROW_THREADS) augment_views_kernel(
    const int32_t *__restrict__ items, const int64_t *__restrict__ offsets, const int32_t *__restrict__ win_seq,
    const int32_t *__restrict__ win_start, const int32_t *__restrict__ win_len, const int32_t *__restrict__ row_win, int B, int holdout,
    uint64_t seed, AugParams P, int64_t *__restrict__ items_out, int ld_items, int64_t *__restrict__ src_tok, int ld_src,
    int32_t *__restrict__ n_out, int32_t *__restrict__ op_out, int32_t *__restrict__ target_out, int32_t *__restrict__ self_count) {
    __shared__ uint64_t keys[1024];
    __shared__ int from[1024];                                 // REORDER: the source position of an output position of the span
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int v = blockIdx.y;                                  // the grid's second dimension selects the view, nothing else
    const RowWindow win = row_window(row_win, win_seq, win_start, win_len, offsets, b, true);
    const BatchRow r = batch_row_rule(P.layout, win.a, win.len, win.n_g, holdout, P.max_len, P.W);
    const int n = r.n;
    const int64_t i = win.o0 + r.first;
    const AugPlan pl = aug_plan(items, offsets, i, n, seed, v, P);
    const int lo = pl.op == B4C_AUG_MASK ? 0 : pl.at, hi = pl.op == B4C_AUG_MASK ? n : pl.at + pl.len;
    const bool ranked = (pl.op == B4C_AUG_MASK || pl.op == B4C_AUG_REORDER) && pl.len > 0;      // (uniform: the barriers are too)
    if (ranked) {
        for (int p = lo + tid; p < hi; p += ROW_THREADS) keys[p] = aug_key(pl.seed_v, (uint64_t)i, p);
        __syncthreads();
        if (pl.op == B4C_AUG_REORDER) {
            for (int p = lo + tid; p < hi; p += ROW_THREADS) from[lo + aug_rank(keys, lo, hi, p)] = p;
            __syncthreads();
        }
    }
    const int64_t row = (int64_t)v * B + b;
    int64_t *out = items_out + row * ld_items;
    int64_t *tok = src_tok ? src_tok + row * ld_src : nullptr;
    for (int p = tid; p < P.W; p += ROW_THREADS) {
        int64_t id = ROW_INPUT_PAD, s = -1;
        if (p < pl.n_out) {
            s = pl.src0 + p;
            bool masked = false;
            if (ranked) {
                if (pl.op == B4C_AUG_MASK) masked = aug_rank(keys, 0, n, p) < pl.len;
                else if (p >= lo && p < hi) s = pl.src0 + from[p];
            }
            id = masked ? ROW_MASK_ID : (int64_t)items[s] + ROW_RESERVED;
        }
        out[p] = id;
        if (tok) tok[p] = s;
    }
    if (tid == 0) {
        n_out[row] = pl.n_out;
        op_out[row] = (int32_t)pl.op;
        if (target_out) target_out[row] = pl.target;
        if (pl.self) atomicAdd(self_count, 1);
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------
// what b4c_augment_views and b4c_augment_row check alike, before any pointer is looked at
static int aug_check_args(const char *who, int B, int W, int layout, int holdout, int ld_items, int n_views, uint32_t ops_mask, float crop_ratio,
                          float mask_ratio, float reorder_ratio) {
    if (const int rc = rows_check_args(who, B, W, ld_items, layout, holdout, 0, 1)) return rc;      // (max_len: NEXT_EVAL's, refused next)
    B4C_REQUIRE(layout != B4C_FEAT_NEXT_EVAL, "%s: layout %d (0 = CLOZE, 1 = NEXT_TRAIN; views of evaluation rows are not built)", who, layout);
    B4C_REQUIRE(n_views >= 1 && n_views <= B4C_AUG_MAX_VIEWS, "%s: n_views = %d (1 .. %d)", who, n_views, B4C_AUG_MAX_VIEWS);
    B4C_REQUIRE(ops_mask != 0 && (ops_mask & ~(uint32_t)AUG_OPS) == 0, "%s: ops_mask = 0x%x (a non-empty subset of 0x%x)", who, ops_mask,
                (unsigned)AUG_OPS);
    B4C_REQUIRE(crop_ratio > 0.f && crop_ratio <= 1.f, "%s: crop_ratio %g outside (0, 1]", who, (double)crop_ratio);      // (a NaN fails both)
    B4C_REQUIRE(mask_ratio >= 0.f && mask_ratio <= 1.f, "%s: mask_ratio %g outside [0, 1]", who, (double)mask_ratio);
    B4C_REQUIRE(reorder_ratio >= 0.f && reorder_ratio <= 1.f, "%s: reorder_ratio %g outside [0, 1]", who, (double)reorder_ratio);
    B4C_REQUIRE(!(ops_mask & B4C_AUG_SAME_TARGET) || layout == B4C_FEAT_NEXT_TRAIN,
                "%s: ops_mask has SAME_TARGET with layout %d (a Cloze row has no target: NEXT_TRAIN = 1 only)", who, layout);
    return B4C_OK;
}

extern "C" int b4c_augment_views(const int32_t *items, const int64_t *offsets, const int32_t *win_seq, const int32_t *win_start,
                                 const int32_t *win_len, const int32_t *row_win, int B, int W, int layout, int holdout, int max_len,
                                 int n_views, uint32_t ops_mask, float crop_ratio, float mask_ratio, float reorder_ratio, uint64_t seed,
                                 const int64_t *tgt_first, const int64_t *tgt_tok, const int32_t *tgt_seq, int V, int64_t *items_out,
                                 int ld_items, int64_t *src_tok, int ld_src, int32_t *n_out, int32_t *op_out, int32_t *target_out,
                                 int32_t *self_count, void *stream) {
    if (const int rc = aug_check_args("augment_views", B, W, layout, holdout, ld_items, n_views, ops_mask, crop_ratio, mask_ratio, reorder_ratio))
        return rc;
    B4C_REQUIRE(!src_tok || ld_src >= W, "augment_views: ld_src = %d < W = %d", ld_src, W);
    if (B == 0) return B4C_OK;
    const bool same = (ops_mask & B4C_AUG_SAME_TARGET) != 0;
    B4C_REQUIRE(!same || (tgt_first && tgt_tok && tgt_seq && V > 0 && self_count),
                "augment_views: null pointer (SAME_TARGET needs the index tgt_first, tgt_tok, tgt_seq, V = %d > 0, and self_count)", V);
    B4C_REQUIRE(items && offsets && items_out && n_out && op_out, "augment_views: null pointer");
    if (const int rc = rows_check_table("augment_views", B, layout, win_seq, win_start, win_len)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (self_count) (void)hipMemsetAsync(self_count, 0, 4, st);
    const AugParams P = {ops_mask, crop_ratio, mask_ratio, reorder_ratio, layout, W, max_len, same ? V : 0, tgt_first, tgt_tok, tgt_seq};
    augment_views_kernel<<<dim3((unsigned)B, (unsigned)n_views), ROW_THREADS, 0, st>>>(items, offsets, win_seq, win_start, win_len, row_win, B,
                                                                                      holdout, seed, P, items_out, ld_items, src_tok, ld_src,
                                                                                      n_out, op_out, target_out, self_count);
    return b4c_check_launch("augment_views");
}

// the rule of one (row, view) on the host
extern "C" int b4c_augment_row(const int32_t *items, const int64_t *offsets, int64_t n_seq, int64_t g, int a, int L, int W, int layout,
                               int holdout, int max_len, int view, uint32_t ops_mask, float crop_ratio, float mask_ratio,
                               float reorder_ratio, uint64_t seed, const int64_t *tgt_first, const int64_t *tgt_tok, const int32_t *tgt_seq,
                               int V, int64_t *out, int64_t *src_tok_out, int32_t *head_out) {
    if (const int rc = aug_check_args("augment_row", 1, W, layout, holdout, W, 1, ops_mask, crop_ratio, mask_ratio, reorder_ratio)) return rc;
    B4C_REQUIRE(view >= 0 && view < B4C_AUG_MAX_VIEWS, "augment_row: view = %d (0 .. %d)", view, B4C_AUG_MAX_VIEWS - 1);
    B4C_REQUIRE(n_seq >= 0 && g < n_seq, "augment_row: g = %lld of n_seq = %lld sequences", (long long)g, (long long)n_seq);
    const bool same = (ops_mask & B4C_AUG_SAME_TARGET) != 0;
    B4C_REQUIRE(!same || (tgt_first && tgt_tok && tgt_seq && V > 0), "augment_row: null pointer (SAME_TARGET needs the index, V = %d > 0)", V);
    B4C_REQUIRE(items && offsets && out && src_tok_out && head_out, "augment_row: null pointer");
    int64_t o0 = 0, n_g = 0;
    if (g < 0 || a < 0) {                                      // an empty row, as row_window makes it
        a = 0;
        L = 0;
    } else {
        o0 = offsets[g];
        n_g = offsets[g + 1] - o0;
    }
    const BatchRow r = batch_row_rule(layout, a, L, n_g, holdout, max_len, W);
    B4C_REQUIRE(r.first + r.n + (layout == B4C_FEAT_NEXT_TRAIN && r.n > 0 ? 1 : 0) <= n_g,
                "augment_row: the row [%lld, %lld) leaves its sequence of %lld items", (long long)r.first, (long long)r.first + r.n,
                (long long)n_g);
    const AugParams P = {ops_mask, crop_ratio, mask_ratio, reorder_ratio, layout, W, max_len, same ? V : 0, tgt_first, tgt_tok, tgt_seq};
    const int n = r.n;
    const int64_t i = o0 + r.first;
    const AugPlan pl = aug_plan(items, offsets, i, n, seed, view, P);
    uint64_t keys[1024];
    const int lo = pl.op == B4C_AUG_MASK ? 0 : pl.at, hi = pl.op == B4C_AUG_MASK ? n : pl.at + pl.len;
    const bool ranked = (pl.op == B4C_AUG_MASK || pl.op == B4C_AUG_REORDER) && pl.len > 0;
    for (int p = 0; p < W; ++p) {
        out[p] = ROW_INPUT_PAD;
        src_tok_out[p] = -1;
    }
    if (ranked)
        for (int p = lo; p < hi; ++p) keys[p] = aug_key(pl.seed_v, (uint64_t)i, p);
    for (int p = 0; p < pl.n_out; ++p) {
        int at = p;                                            // the output position of source position p
        bool masked = false;
        if (ranked) {
            if (pl.op == B4C_AUG_MASK) masked = aug_rank(keys, 0, n, p) < pl.len;
            else if (p >= lo && p < hi) at = lo + aug_rank(keys, lo, hi, p);
        }
        out[at] = masked ? ROW_MASK_ID : (int64_t)items[pl.src0 + p] + ROW_RESERVED;
        src_tok_out[at] = pl.src0 + p;
    }
    head_out[0] = pl.n_out;
    head_out[1] = (int32_t)pl.op;
    head_out[2] = pl.target;
    head_out[3] = pl.self;
    return B4C_OK;
}
