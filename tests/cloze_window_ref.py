"""Host restatement of the windowed Cloze-batch rule of include/b4c.h ("Cloze batches over windows"), written from the header's
text with numpy and ops.rand64_host only: the window seed, the last-only draw, the keys of an ordinary row, the evaluation rows
of a split, the history lists, and the window table of cloze_batches.DeviceCloze as a plain loop over the sequences."""
import numpy as np

from cloze_batch_ref import EVAL, INPUT_PAD, LABEL_PAD, MASK_ID, RESERVED, TRAIN, n_masked, synthetic_csr  # noqa: F401

WINDOW_SALT, LAST_SALT = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
LAST_ONE = 1 << 24
MASK64 = (1 << 64) - 1


def _rand64(seed, ctr):
    from bert4clickpath_amd import ops
    return int(ops.rand64_host(seed & MASK64, np.array([ctr], dtype=np.uint64))[0])


def window_seed(seed, a):
    return seed & MASK64 if a == 0 else _rand64(seed ^ WINDOW_SALT, a)


def last_only(seed, g, a, L, last_thr):
    return L > 0 and (_rand64(window_seed(seed, a) ^ LAST_SALT, g) >> 40) < last_thr


def choose_window(seed, g, a, L, masked_percentage=0.4, max_masked=10, last_thr=0):
    """the masked positions of the TRAIN window of L items at start a of sequence g, ascending"""
    from bert4clickpath_amd import ops
    if last_only(seed, g, a, L, last_thr):
        return np.array([L - 1], np.int32)
    n = n_masked(L, masked_percentage, max_masked)
    p = np.arange(L, dtype=np.uint64)
    k = ops.rand64_host(window_seed(seed, a), (np.uint64(g) << np.uint64(10)) | p)
    return np.sort(np.lexsort((p, k))[:n]).astype(np.int32)


def window_table(lengths, max_len=None, stride=None, holdout=1):
    """-> (seq, start, len) int32 arrays, a loop over the sequences: the training view of n items is [0, T), T = max(n - holdout,
    0); T <= max_len: one window (0, T), none for T = 0 when max_len is set; T > max_len: starts T - max_len - j stride while
    positive, then 0, each of max_len items"""
    rows = []
    for g, n in enumerate(lengths):
        T = max(int(n) - holdout, 0)
        if max_len is None:
            rows.append((g, 0, T))
        elif T <= max_len:
            if T > 0:
                rows.append((g, 0, T))
        else:
            s = stride if stride is not None else max_len
            a = T - max_len
            while a > 0:
                rows.append((g, a, max_len))
                a -= s
            rows.append((g, 0, max_len))
    t = np.array(rows, dtype=np.int32).reshape(-1, 3)
    return t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy()


def eval_window(n, split, max_len=None):
    """(start, L) of the evaluation row of a sequence of n items: the last min(t + 1, max_len) positions ending at the target
    t = n - 1 ('test') or n - 2 ('valid'); (0, 0) when the sequence has no such item"""
    t = n - (2 if split == 'valid' else 1)
    if t < 0:
        return 0, 0
    L = t + 1 if max_len is None else min(t + 1, max_len)
    return t + 1 - L, L


def batch(items, offsets, windows, W, mode, seed, masked_percentage=0.4, max_masked=10, M=None, last_thr=0):
    """windows: (g, a, L) triples, g < 0 an empty row -> (items_out int64 [B, W], labels_padded float32 [B, M], n_masked
    int32 [B]) of the header's definition"""
    B = len(windows)
    M = (max_masked if mode == TRAIN else 1) if M is None else M
    out = np.full((B, W), INPUT_PAD, np.int64)
    lab = np.full((B, M), LABEL_PAD, np.float32)
    nm = np.zeros(B, np.int32)
    for b, (g, a, L) in enumerate(windows):
        if g < 0:
            continue
        L = min(max(int(L), 0), W)
        o = int(offsets[g]) + int(a)
        assert o + L <= offsets[g + 1]
        seq = np.asarray(items[o:o + L], dtype=np.int64)
        if mode == TRAIN:
            pos = choose_window(seed, int(g), int(a), L, masked_percentage, max_masked, last_thr)
        else:
            pos = np.arange(L - 1, L) if L else np.zeros(0, np.int64)
        out[b, :L] = seq + RESERVED
        out[b, pos] = MASK_ID
        lab[b, :len(pos)] = seq[pos]
        nm[b] = len(pos)
    return out, lab, nm


def history(items, offsets, seq_idx, E, drop):
    """[B, E] int32: the items of every named sequence in front of item n - drop, the most recent E of them, then -1"""
    out = np.full((len(seq_idx), E), -1, np.int32)
    for b, g in enumerate(seq_idx):
        if g < 0:
            continue
        h = np.asarray(items[offsets[g]:max(offsets[g + 1] - drop, offsets[g])])[-E:]
        out[b, :len(h)] = h
    return out
