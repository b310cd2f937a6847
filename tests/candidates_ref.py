"""Host restatements of the candidate-list definitions (include/b4c.h, "candidate lists"), in numpy / float64 / Python integers:
the sampler (bit for bit), and rank / top-k of a per-row list over given scores.  Used by test_candidates_cpu.py and
test_gpu_candidates.py."""
import numpy as np

from bert4clickpath_amd import ops


def sample_rows(labels, V, N, seed, row_base=0, exclude=None, cdf=None):
    """-> (cand int32 [R, 1 + N], short): b4c_sample_candidates restated.  exclude: per-row iterables of ids (or None);
    cdf: int64 [V] inclusive prefix sum of item counts (None: uniform)."""
    labels = np.asarray(labels, np.int64)
    R = labels.shape[0]
    out = np.full((R, N + 1), -1, np.int32)
    short = 0
    total = int(cdf[-1]) if cdf is not None else 0
    cdf_u = np.asarray(cdf, np.int64).astype(np.uint64) if cdf is not None else None
    for r in range(R):
        y = int(labels[r])
        if y < 0 or y >= V:
            continue
        out[r, 0] = y
        if N == 0:
            continue
        j = np.arange(64 * N, dtype=np.uint64)
        x = ops.rand64_host(seed, (np.uint64(row_base + r) << np.uint64(20)) | j)
        if cdf is None:
            items = ops.mulhi64_host(x, V).astype(np.int64)
        else:
            items = np.searchsorted(cdf_u, ops.mulhi64_host(x, total), side='right').astype(np.int64)   # min{i : cdf[i] > u}
        ex = set(int(e) for e in exclude[r]) if exclude is not None else set()
        acc, seen = [], set()
        for it in items.tolist():
            if it != y and it not in ex and it not in seen:
                acc.append(it)
                seen.add(it)
                if len(acc) == N:
                    break
        out[r, 1:1 + len(acc)] = acc
        short += len(acc) < N
    return out, short


def rank_rows(s_list, cand, s_label, labels, V):
    """rank of the definition: s_list [R, C] scores at the list positions, s_label [R] the label's score"""
    R, C = cand.shape
    rank = np.full(R, -1, np.int64)
    for r in range(R):
        y = int(labels[r])
        if y < 0 or y >= V:
            continue
        seen, n = set(), 0
        for p in range(C):
            c = int(cand[r, p])
            if c < 0 or c >= V or c == y or c in seen:
                continue
            seen.add(c)
            if s_list[r, p] > s_label[r] or (s_list[r, p] == s_label[r] and c < y):
                n += 1
        rank[r] = n
    return rank


def topk_rows(s_list, cand, V, k):
    """the k best distinct present items of each list (score descending, ties -> lower id), -1 past the last"""
    R, C = cand.shape
    idx = np.full((R, k), -1, np.int64)
    for r in range(R):
        best = {}
        for p in range(C):
            c = int(cand[r, p])
            if 0 <= c < V and c not in best:
                best[c] = s_list[r, p]
        order = sorted(best.items(), key=lambda t: (-t[1], t[0]))[:k]
        idx[r, :len(order)] = [c for c, _ in order]
    return idx
