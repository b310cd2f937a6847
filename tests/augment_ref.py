"""Host restatement of the contrastive views (include/b4c.h), written from the header's definition in numpy and Python
integers: ops.rand64_host for the random stream, a stable argsort on (k, p) for the ranks, float32 products for the shares.  It does
not call b4c_augment_row.  Used by test_augment_cpu.py and test_gpu_augment.py."""
import functools

import numpy as np

from bert4clickpath_amd.ops import rand64_host

CLOZE, NEXT_TRAIN, NEXT_EVAL = 0, 1, 2
CROP, MASK, REORDER, SAME_TARGET = 1, 2, 4, 8
OPS = {'crop': CROP, 'mask': MASK, 'reorder': REORDER, 'same_target': SAME_TARGET}
RESERVED, MASK_ID, PAD = 10, 1, 0
C_VIEW, C_OP, C_AT = 0xA0761D6478BD642F, 0xE7037ED1A0B428DB, 0x8EBC6AF09C88C6E3
M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def rand64(seed, ctr):
    return int(rand64_host(seed & M64, np.array([ctr & M64], np.uint64))[0])


def row_keys(seed_v, i, n):
    """k_p = rand64(seed_v, (i << 10) | p) for p in [0, n)"""
    return rand64_host(seed_v, (np.uint64(i) << np.uint64(10)) | np.arange(n, dtype=np.uint64))


def mulhi(x, m):
    return (x * m) >> 64


def share(n, ratio):
    """(int)((float)n * r): a float32 product, then truncation"""
    return int(np.float32(n) * np.float32(ratio))


def ops_mask(names):
    m = 0
    for name in ([names] if isinstance(names, str) else names):
        m |= OPS[name]
    return m


def row_rule(layout, n_g, a, L, holdout, W):
    """-> (first, n) of the header's "Source" """
    if layout == CLOZE:
        return a, max(min(L, W), 0)
    T = max(n_g - holdout, 0)
    first = a - 1 if a > 0 else 0
    return first, max(min(L if a > 0 else L - 1, W, T - first - 1), 0)


def target_index(items, offsets, holdout, V):
    """(tgt_first int64 [V + 1], tgt_tok int64 [n], tgt_seq int32 [n]): every token at position q of its sequence with
    1 <= q < T_g = max(n_g - holdout, 0), in the order (item, token index)"""
    items, offsets = np.asarray(items, np.int64), np.asarray(offsets, np.int64)
    tok, seq = [], []
    for g in range(len(offsets) - 1):
        T = max(int(offsets[g + 1] - offsets[g]) - holdout, 0)
        for q in range(1, T):
            tok.append(int(offsets[g]) + q)
            seq.append(g)
    tok, seq = np.array(tok, np.int64), np.array(seq, np.int32)
    order = np.argsort(items[tok], kind='stable') if len(tok) else np.zeros(0, np.int64)
    tok, seq = tok[order], seq[order]
    first = np.concatenate([[0], np.cumsum(np.bincount(items[tok], minlength=V))]).astype(np.int64)
    return first, tok, seq


def one_view(items, offsets, g, a, L, layout, W, v, mask, seed, holdout=1, max_len=0, crop_ratio=0.6, mask_ratio=0.3, reorder_ratio=0.6,
             index=None, V=0):
    """-> dict(items int64 [W], src_tok int64 [W], n_out, op, target, self, partner_q): one (row, view) of the definition.
    g < 0: an empty row.  partner_q: the partner's position in its sequence (same-target rows with a partner), else None."""
    items, offsets = np.asarray(items, np.int64), np.asarray(offsets, np.int64)
    out, tok = np.full(W, PAD, np.int64), np.full(W, -1, np.int64)
    res = {'items': out, 'src_tok': tok, 'n_out': 0, 'op': 0, 'target': -1, 'self': 0, 'partner_q': None}
    if g < 0 or a < 0:
        return res
    o0, n_g = int(offsets[g]), int(offsets[g + 1] - offsets[g])
    first, n = row_rule(layout, n_g, a, L, holdout, W)
    if n == 0:
        return res
    i = o0 + first
    seed_v = rand64(seed ^ C_VIEW, v)
    h_op, h_at = rand64(seed_v ^ C_OP, i), rand64(seed_v ^ C_AT, i)
    enabled = [bit for bit in (CROP, MASK, REORDER, SAME_TARGET) if mask & bit]
    op = enabled[mulhi(h_op, len(enabled))]
    keys = row_keys(seed_v, i, n) if op in (MASK, REORDER) else None
    src = np.arange(i, i + n)                                   # CSR indices of the source row
    masked = np.zeros(0, bool)
    if op == CROP:
        Lc = max(1, share(n, crop_ratio))
        c = mulhi(h_at, n - Lc + 1)
        sel = src[c:c + Lc]
    elif op == MASK:
        m = min(n, share(n, mask_ratio))
        order = np.argsort(keys, kind='stable')                     # ascending (k_p, p): ties of the key go to the lower p
        sel = src
        masked = np.zeros(n, bool)
        masked[order[:m]] = True
    elif op == REORDER:
        Lr = min(n, share(n, reorder_ratio))
        r0 = mulhi(h_at, n - Lr + 1)
        order = r0 + np.argsort(keys[r0:r0 + Lr], kind='stable')      # rho(order[k]) = k
        sel = src.copy()
        sel[r0:r0 + Lr] = src[order]
    else:
        t = i + n
        y = int(items[t])
        first_y, tgt_tok, tgt_seq = index
        lst = tgt_tok[first_y[y]:first_y[y + 1]] if 0 <= y < V else tgt_tok[:0]
        own = int(np.searchsorted(lst, t, side='left'))
        found = own < len(lst) and int(lst[own]) == t
        others = len(lst) - int(found)
        if others == 0:
            sel = src
            res['self'] = 1
        else:
            u = mulhi(h_at, others)
            k = int(first_y[y]) + u + (1 if found and u >= own else 0)
            j, g2 = int(tgt_tok[k]), int(tgt_seq[k])
            q = j - int(offsets[g2])
            n_out = min(q, W) if max_len <= 0 else min(q, W, max_len)
            sel = np.arange(j - n_out, j)
            res['partner_q'] = q
    n_out = len(sel)
    out[:n_out] = items[sel] + RESERVED
    if len(masked):
        out[:n_out][masked] = MASK_ID
    tok[:n_out] = sel
    res.update(n_out=n_out, op=op, target=int(items[i + n]) if layout == NEXT_TRAIN else -1)
    return res


def batch(items, offsets, windows, row_idx, layout, W, n_views, mask, seed, **kw):
    """the views of the rows row_idx (indices into windows = (seq, start, len); negative: an empty row) -> dict(items, src_tok
    [n_views, B, W], n_out, op, target [n_views, B], self_count, rows: the per-(view, row) dicts)"""
    B = len(row_idx)
    got = {'items': np.zeros((n_views, B, W), np.int64), 'src_tok': np.zeros((n_views, B, W), np.int64),
           'n_out': np.zeros((n_views, B), np.int32), 'op': np.zeros((n_views, B), np.int32), 'target': np.zeros((n_views, B), np.int32),
           'self_count': 0, 'rows': {}}
    for v in range(n_views):
        for b, w in enumerate(np.asarray(row_idx, np.int64).tolist()):
            g, a, L = (-1, 0, 0) if w < 0 else (int(windows[0][w]), int(windows[1][w]), int(windows[2][w]))
            r = one_view(items, offsets, g, a, L, layout, W, v, mask, seed, **kw)
            got['items'][v, b], got['src_tok'][v, b] = r['items'], r['src_tok']
            got['n_out'][v, b], got['op'][v, b], got['target'][v, b] = r['n_out'], r['op'], r['target']
            got['self_count'] += r['self']
            got['rows'][v, b] = r
    return got


# ---- the case list both test files share ---------------------------------------------------------------------------------------
MAX_LEN = 5
SEEDS = (11, 2024, 77)
# (ops, {ratio: value}): each op alone over the ratios {0, 0.3, 0.6, 1} it may take, the same-target row, the three-op mix
CONFIGS = ([(('crop',), {'crop_ratio': r}) for r in (0.3, 0.6, 1.0)] + [(('mask',), {'mask_ratio': r}) for r in (0.0, 0.3, 0.6, 1.0)]
           + [(('reorder',), {'reorder_ratio': r}) for r in (0.0, 0.3, 0.6, 1.0)] + [(('same_target',), {}), (('crop', 'mask', 'reorder'), {})])


def config_id(c):
    return '+'.join(c[0]) + ''.join('-%g' % r for r in c[1].values())


def case_table(offsets, holdout):
    """window_table's windows at max_len = stride = 5, and one window of no items (L = 0) of sequence 1 at the end"""
    from bert4clickpath_amd.cloze_batches import window_table
    w = window_table(np.diff(offsets), MAX_LEN, MAX_LEN, holdout)
    return tuple(np.concatenate([x, np.array([v], np.int32)]) for x, v in zip(w, (1, 0, 0)))


def case_rows(table):
    """<= 16 rows for one launch: every window of the short sequences and of the repeated-item sequence, the long sequence's
    window at 0, one in its middle and its last, an empty row (negative index), the L = 0 window"""
    seq, start, _ = table
    pick = [int(w) for w in np.flatnonzero(np.isin(seq[:-1], [2, 3, 5, 6, 10]))]
    long_w = np.flatnonzero(seq[:-1] == 7)
    four = np.flatnonzero(seq[:-1] == 4)
    pick += [int(long_w[np.argmin(start[long_w])]), int(long_w[len(long_w) // 2]), int(long_w[0]), int(four[0]), int(four[-1]), -1,
             len(seq) - 1]
    assert len(pick) <= 16
    return np.array(pick, np.int64)
