"""Host restatement of the Cloze-batch rule of include/b4c.h ("Cloze batches"): numpy and ops.rand64_host only, written from
the header's text -- keys k_p = rand64(seed, (g << 10) | p), the n positions smallest in (k_p, p) order, ascending."""
import numpy as np

TRAIN, EVAL = 0, 1
MASK_ID, INPUT_PAD, LABEL_PAD, RESERVED = 1, 0, -1.0, 10


def n_masked(L, masked_percentage=0.4, max_masked=10):
    return int(min(max(int(np.int32(np.float32(L) * np.float32(masked_percentage))), 0), max_masked))


def choose(seed, g, L, n):
    """the n masked positions of [0, L) for sequence g, ascending"""
    from bert4clickpath_amd import ops
    p = np.arange(L, dtype=np.uint64)
    k = ops.rand64_host(seed, (np.uint64(g) << np.uint64(10)) | p)
    return np.sort(np.lexsort((p, k))[:n]).astype(np.int32)


def batch(items, offsets, seq_idx, W, mode, seed, masked_percentage=0.4, max_masked=10, M=None):
    """-> (items_out int64 [B, W], labels_padded float32 [B, M], n_masked int32 [B]) of the header's definition"""
    B = len(seq_idx)
    M = (max_masked if mode == TRAIN else 1) if M is None else M
    out = np.full((B, W), INPUT_PAD, np.int64)
    lab = np.full((B, M), LABEL_PAD, np.float32)
    nm = np.zeros(B, np.int32)
    for b, g in enumerate(seq_idx):
        seq = np.asarray(items[offsets[g]:offsets[g + 1]], dtype=np.int64)
        if mode == TRAIN:
            seq = seq[:-1]
            pos = choose(seed, int(g), len(seq), n_masked(len(seq), masked_percentage, max_masked))
        else:
            pos = np.arange(len(seq) - 1, len(seq)) if len(seq) else np.zeros(0, np.int64)
        assert len(seq) <= W
        out[b, :len(seq)] = seq + RESERVED
        out[b, pos] = MASK_ID
        lab[b, :len(pos)] = seq[pos]
        nm[b] = len(pos)
    return out, lab, nm


def synthetic_csr(lengths, V, seed):
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rng.integers(0, V, int(offsets[-1])).astype(np.int32), offsets
