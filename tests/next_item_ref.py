"""Host restatement of the next-item batch rule (include/b4c.h), in numpy and Python integers: rows, flat_idx, labels,
row_off, X_g; the negatives through tests/candidates_ref.sample_rows, called per target with row_base = the target token's CSR
index.  Used by test_next_item_cpu.py and test_gpu_next_item.py."""
import numpy as np

import candidates_ref as cref

TRAIN, EVAL = 0, 1
RESERVED, MAX_EXCL = 10, 1024


def row_rule(mode, n_g, a=0, L=0, holdout=1, max_len=None, W=1021):
    """-> (first, n_in, p_lo, view): inputs s_g[first .. first + n_in), targets at the input positions p_lo .. n_in, X_g from
    s_g[max(0, view - 1024) .. view).  EVAL: holdout is the split's drop."""
    if mode == TRAIN:
        T = max(n_g - holdout, 0)
        first = a - 1 if a > 0 else 0
        n_in = L if a > 0 else max(L - 1, 0)
        n_in = max(min(n_in, W, T - first - 1), 0)
        return first, n_in, 0, T
    t = n_g - holdout
    if t < 1:
        return 0, 0, 0, max(t, 0)
    n_in = min(t, W if max_len is None else min(max_len, W))
    return t - n_in, n_in, n_in - 1, t


def x_set(seq, view, exclude):
    return set() if exclude is None else set(int(v) for v in seq[max(0, view - MAX_EXCL):view])


def one_row(seq, seq_off, mode, V, a=0, L=0, holdout=1, max_len=None, W=1021, N=0, seed=0, exclude='history', cdf=None):
    """-> dict(inputs int64 [W], pos [n], labels [n], candidates [n, 1 + N] or None, n_in, short, X): one row of the rule"""
    seq = np.asarray(seq, np.int64)
    first, n_in, p_lo, view = row_rule(mode, len(seq), a, L, holdout, max_len, W)
    inputs = np.zeros(W, np.int64)
    inputs[:n_in] = seq[first:first + n_in] + RESERVED
    pos = np.arange(p_lo, n_in, dtype=np.int64)
    labels = seq[first + pos + 1] if len(pos) else np.zeros(0, np.int64)
    X = x_set(seq, view, exclude)
    cand, short = None, 0
    if N > 0:
        cand = np.full((len(pos), N + 1), -1, np.int32)
        for q, p in enumerate(pos.tolist()):
            y = int(labels[q])
            if cdf is not None and int(cdf[-1]) <= 0:             # a cdf without mass draws nothing: the row stays short
                c, s = np.array([[y] + [-1] * N], np.int32), 1
            else:
                c, s = cref.sample_rows([y], V, N, seed, row_base=int(seq_off) + first + p + 1, exclude=[X - {y}], cdf=cdf)
            cand[q] = c[0]
            short += s
    return {'inputs': inputs, 'pos': pos, 'labels': labels.astype(np.int32), 'candidates': cand, 'n_in': n_in, 'short': short, 'X': X}


def batch(items, offsets, mode, row_idx, V, windows=None, holdout=1, max_len=None, W=None, N=0, seed=0, exclude='history', cdf=None, rows=None):
    """The batch of the rows row_idx -- TRAIN: indices into windows = (seq, start, len); EVAL: sequences; negative: an empty row.
    -> dict(items [B, W], flat_idx [rows], labels [rows], candidates [rows, 1 + N] or None, row_off [B + 1], short, n_targets,
    n_real_tokens, X: per compact row its X_g, csr: per compact row the target token's CSR index)."""
    items, offsets = np.asarray(items, np.int64), np.asarray(offsets, np.int64)
    per = []
    for w in np.asarray(row_idx, np.int64).tolist():
        if w < 0:
            per.append((None, 0, one_row(np.zeros(0, np.int64), 0, EVAL, V, W=1021, holdout=1, N=N)))
            continue
        g, a, L = (int(windows[0][w]), int(windows[1][w]), int(windows[2][w])) if mode == TRAIN else (w, 0, 0)
        seq = items[offsets[g]:offsets[g + 1]]
        first = row_rule(mode, len(seq), a, L, holdout, max_len)[0]
        per.append((g, int(offsets[g]) + first, one_row(seq, offsets[g], mode, V, a, L, holdout, max_len, 1021, N, seed, exclude, cdf)))
    B = len(per)
    longest = max([r['n_in'] for _, _, r in per] + [1])
    W = longest if W is None else W
    assert W >= longest
    counts = np.array([len(r['pos']) for _, _, r in per], np.int64)
    row_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    R = int(row_off[-1])
    rows = R if rows is None else rows
    out = np.zeros((B, W), np.int64)
    flat, lab = np.full(rows, -1, np.int32), np.full(rows, -1, np.int32)
    cand = np.full((rows, N + 1), -1, np.int32) if N > 0 else None
    X, csr, short = [], [], 0
    for b, (g, base, r) in enumerate(per):
        out[b] = r['inputs'][:W]
        lo, hi = row_off[b], row_off[b + 1]
        flat[lo:hi] = b * (W + 3) + 2 + r['pos']
        lab[lo:hi] = r['labels']
        if cand is not None:
            cand[lo:hi] = r['candidates']
        short += r['short']
        X += [r['X']] * len(r['pos'])
        csr += [base + int(p) + 1 for p in r['pos']]
    return {'items': out, 'flat_idx': flat, 'labels': lab, 'candidates': cand, 'row_off': row_off, 'short': short, 'n_targets': R,
            'n_real_tokens': int(sum(r['n_in'] for _, _, r in per)) + 3 * B, 'X': X, 'csr': csr}


def case_data():
    """The case list's data set: V = 500 items.  Sequences by index:
      0: empty; 1: one item; 2: two; 3: three; 4: 12 items (windows at a > 0 with max_len 5); 5: exactly max_len + 1;
      6: repeated items (target equal to input, duplicates in X_g); 7: 1100 items (the 1024 cap of X_g: early windows lie in
      front of it); 8: max_len + 7 items (EVAL t = max_len + 5 at drop 2); 9: max_len + 6 items (the same at drop 1); 10: four items."""
    rng = np.random.default_rng(20)
    seqs = [[], [7], [3, 9], [4, 4, 8], rng.integers(0, 500, 12).tolist(), rng.integers(0, 500, 6).tolist(),
            [5, 5, 6, 5, 6, 6, 7, 5, 5, 9], rng.integers(0, 500, 1100).tolist(), rng.integers(0, 500, 12).tolist(),
            rng.integers(0, 500, 11).tolist(), [1, 2, 3, 1]]
    items = np.array([v for s in seqs for v in s], np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return items, offsets, 500
