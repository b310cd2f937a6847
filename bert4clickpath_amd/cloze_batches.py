"""Cloze training and evaluation batches built on the device (ops.cloze_batch, include/b4c.h "Cloze batches").

input_pipeline.BeautyCloze walks every batch row by row on the host and the training loop then uploads ids and labels;
DeviceCloze keeps the data set's CSR form on the device and leaves `items` and `labels_padded` there, in the layout
model.cloze_loss(items, labels_padded, max_masked_per_row=M, n_real_tokens=n) takes without a read-back.  The host keeps the
offsets: row widths and the token count n_real_tokens come from them with numpy, nothing is read back from the device.
The masking rule is a pure function of (seed, sequence index, sequence): a row does not depend on the batch it is in, on the
rank or on the batch size.  The random stream is this build's own (the reference's shuffle is unseeded)."""
import numpy as np
import torch

from . import ops
from .input_pipeline import EVAL, MASKED_PERCENTAGE, MAX_MASKED_ITEMS, TRAIN

_MODES = {TRAIN: ops.CLOZE_TRAIN, EVAL: ops.CLOZE_EVAL, ops.CLOZE_TRAIN: ops.CLOZE_TRAIN, ops.CLOZE_EVAL: ops.CLOZE_EVAL}


class DeviceCloze:
    """items: item indices of every sequence back to back (label space: input id = 10 + index), offsets [n_seq + 1]: their
    CSR bounds -- numpy arrays or CPU tensors, as data/beauty_sequences.npz holds them.  V: vocabulary size (labels are float32,
    the reference's format, and must be exact: V <= 2^24).  device=None keeps the host side only (no batches can be built)."""

    def __init__(self, items, offsets, V=None, max_masked=MAX_MASKED_ITEMS, masked_percentage=MASKED_PERCENTAGE, device='cuda'):
        items = np.ascontiguousarray(np.asarray(items), dtype=np.int32)
        offsets = np.ascontiguousarray(np.asarray(offsets), dtype=np.int64)
        if items.ndim != 1 or offsets.ndim != 1 or len(offsets) < 1:
            raise ValueError('DeviceCloze: items [N] and offsets [n_seq + 1] are one-dimensional')
        lengths = np.diff(offsets)
        if offsets[0] != 0 or offsets[-1] != len(items) or (lengths < 0).any():
            raise ValueError('DeviceCloze: offsets must rise from 0 to len(items) = %d' % len(items))
        self.V = int(V) if V is not None else (int(items.max()) + 1 if len(items) else 0)
        if self.V > 2 ** 24:
            raise ValueError('DeviceCloze: V = %d > 2**24: float32 labels (the reference\'s format) would not be exact' % self.V)
        if len(items) and (items.min() < 0 or items.max() >= self.V):
            raise ValueError('DeviceCloze: item indices outside [0, V = %d)' % self.V)
        if not 0 <= int(max_masked) <= ops.CLOZE_MAX_LABELS:
            raise ValueError('DeviceCloze: max_masked = %d (0 .. %d)' % (max_masked, ops.CLOZE_MAX_LABELS))
        self.max_masked, self.masked_percentage = int(max_masked), float(masked_percentage)
        self.offsets, self.lengths = offsets, lengths
        self.n_seq = len(lengths)
        self.items_dev = self.offsets_dev = None
        if device is not None:
            self.items_dev = torch.from_numpy(items).to(device)
            self.offsets_dev = torch.from_numpy(offsets).to(device)

    @classmethod
    def from_npz(cls, path, **kw):
        z = np.load(path, allow_pickle=False)
        return cls(z['items'], z['offsets'], V=int(z['vocab'].shape[0]), **kw)

    def row_lengths(self, seq_idx, mode):
        """host: L of every named sequence (TRAIN: without the held-out last item)"""
        n = self.lengths[np.asarray(seq_idx, dtype=np.int64)]
        return np.maximum(n - 1, 0) if _MODES[mode] == ops.CLOZE_TRAIN else n

    def n_real_tokens(self, seq_idx, mode):
        """host int: non-pad positions of the chained batch = sum of the row lengths + [CLS] [SEP] .. [SEP] per row"""
        L = self.row_lengths(seq_idx, mode)
        return int(L.sum()) + 3 * len(L)

    def _width(self, L, width):
        longest = int(L.max()) if len(L) else 0
        if width is None:
            return max(longest, 1)
        if int(width) < longest:
            raise ValueError('DeviceCloze: width = %d is shorter than a row of %d items' % (width, longest))
        return int(width)

    def _batch(self, seq_host, seq_dev, mode, seed, width):
        L = self.row_lengths(seq_host, mode)
        W = self._width(L, width)
        if W > ops.CLOZE_MAX_WIDTH:
            raise ValueError('DeviceCloze: a row of %d items; at most %d' % (W, ops.CLOZE_MAX_WIDTH))
        self._need_device()
        items, lab, nm = ops.cloze_batch(self.items_dev, self.offsets_dev, seq_dev, W, _MODES[mode], seed, self.masked_percentage,
                                         self.max_masked)
        return {'items': items, 'labels_padded': lab, 'n_masked': nm, 'seq_idx': seq_dev, 'n_real_tokens': int(L.sum()) + 3 * len(L)}

    def _need_device(self):
        if self.items_dev is None:
            raise ValueError('DeviceCloze: built with device=None (host side only)')

    def _check_seq(self, seq_idx):
        seq = np.asarray(seq_idx, dtype=np.int64).reshape(-1)
        if len(seq) and (seq.min() < 0 or seq.max() >= self.n_seq):
            raise ValueError('DeviceCloze: sequence indices outside [0, %d)' % self.n_seq)
        return seq

    def batch(self, seq_idx, mode, seed=0, width=None):
        """One batch of the sequences seq_idx (host integers, any order, repeats allowed) -> dict(items (B, W) int64,
        labels_padded (B, M) float32 -- M = max_masked for TRAIN, 1 for EVAL --, n_masked (B,) int32, seq_idx int32: device
        tensors; n_real_tokens: host int).  width None: the batch's longest row (as BeautyCloze pads); an int fixes W."""
        seq = self._check_seq(seq_idx)
        dev = None if self.items_dev is None else torch.from_numpy(seq.astype(np.int32)).to(self.items_dev.device)
        return self._batch(seq, dev, mode, seed, width)

    def epoch_order(self, seed, epoch):
        return np.random.default_rng([int(seed), int(epoch)]).permutation(self.n_seq)

    def rank_slices(self, batch_size, seed, epoch, rank=0, world=1):
        """host: (order, [(lo, hi), ...]) -- epoch `epoch`'s permutation and rank `rank`'s slice of every full global batch of
        batch_size * world consecutive entries (the remainder is dropped, as BeautyCloze does)"""
        if not (batch_size > 0 and 0 <= rank < world):
            raise ValueError('DeviceCloze: batch_size = %d, rank %d of %d' % (batch_size, rank, world))
        order = self.epoch_order(seed, epoch)
        G = batch_size * world
        return order, [(s + rank * batch_size, s + (rank + 1) * batch_size) for s in range(0, self.n_seq - G + 1, G)]

    def train_batches(self, batch_size, seed, steps, rank=0, world=1, width=None):
        """`steps` TRAIN batches of batch_size sequences for rank `rank` of `world`: one seeded permutation per epoch (uploaded
        once), the mask seed of epoch e is rand64_host(seed, e)."""
        self._need_device()
        order, slices = self.rank_slices(batch_size, seed, 0, rank, world)
        if steps > 0 and not slices:
            raise ValueError('DeviceCloze: %d sequences do not fill one batch of %d x %d' % (self.n_seq, batch_size, world))
        done = epoch = 0
        while done < steps:
            if epoch:
                order, slices = self.rank_slices(batch_size, seed, epoch, rank, world)
            order_dev = torch.from_numpy(order.astype(np.int32)).to(self.items_dev.device)
            mask_seed = int(ops.rand64_host(seed, epoch))
            for lo, hi in slices:
                yield self._batch(order[lo:hi], order_dev[lo:hi], TRAIN, mask_seed, width)
                done += 1
                if done >= steps:
                    return
            epoch += 1

    def eval_batches(self, batch_size, limit=None, width=None):
        """EVAL batches of the sequences 0 .. limit in order, the last one partial.  An empty sequence gives a row without a
        [MASK] whose label column is -1: compact labels taken from labels_padded then need the rows with n_masked == 1."""
        self._need_device()
        n = self.n_seq if limit is None else min(int(limit), self.n_seq)
        seq = np.arange(n, dtype=np.int64)
        seq_dev = torch.arange(n, dtype=torch.int32, device=self.items_dev.device)
        for s in range(0, n, batch_size):
            yield self._batch(seq[s:s + batch_size], seq_dev[s:s + batch_size], EVAL, 0, width)
