"""Cloze training and evaluation batches built on the device (ops.cloze_batch_windows, include/b4c.h "Cloze batches").

input_pipeline.BeautyCloze walks every batch row by row on the host and the training loop then uploads ids and labels;
DeviceCloze keeps the data set's CSR form on the device and leaves `items` and `labels_padded` there, in the layout
model.cloze_loss(items, labels_padded, max_masked_per_row=M, n_real_tokens=n) takes without a read-back.  The host keeps the
offsets: row widths and the token count n_real_tokens come from them with numpy, nothing is read back from the device.
The masking rule is a pure function of (seed, sequence index, window start, the window's items): a row does not depend on the
batch it is in, on the rank or on the batch size.  The random stream is this build's own (the reference's shuffle is unseeded,
SURVEY.md D9).

A row is a WINDOW of a sequence.  By default every sequence is one window (all but its last item for training, all of it for
evaluation).  The BERT4Rec paper's data protocol is four constructor arguments: max_len / stride cut the training view of a long
sequence into sliding windows and keep the most recent max_len positions for evaluation, holdout=2 holds out the penultimate
item for validation and the last for test, last_item_rate adds training rows whose only masked position is the last one.  The
window table is built once with numpy and uploaded once; a batch names its windows by index.

The next_item_* methods build the left-to-right objective over the same windows (ops.next_item_batch, include/b4c.h): rows
without a [MASK], every real position's target the item after it, each target's own sampled negatives; model.next_item_loss takes
such a batch.

features={name: Feature(...)} hands over side columns of the click paths -- one value per event (an action, a dwell bucket) or one
per item (a category, a brand).  They are validated and uploaded once; every batch dict then carries 'features': {name: (B, W)
int64 ids} built from the item row in one launch (ops.batch_features, include/b4c.h), [MASK] where the item row has
it unless the feature says on_mask='keep'.  inputs(batch, item_feature) is the dict the model's entry points take.

views(batch, seed, ...) builds contrastive views of a training batch's rows on the device (ops.augment_views, include/b4c.h):
CL4SRec's item crop / mask / reorder and DuoRec's same-target row, each with the host-known n_real_tokens that lets
model.contrastive_loss(..., inputs_b=, n_real_tokens_b=) encode the view padding-free."""
import collections

import numpy as np
import torch

from . import ops
from . import ops as _ops            # (DeviceCloze.views has an argument called ops)
from .input_pipeline import EVAL, MASKED_PERCENTAGE, MAX_MASKED_ITEMS, TRAIN

_MODES = {TRAIN: ops.CLOZE_TRAIN, EVAL: ops.CLOZE_EVAL, ops.CLOZE_TRAIN: ops.CLOZE_TRAIN, ops.CLOZE_EVAL: ops.CLOZE_EVAL}


_SPLITS = ('test', 'valid')
Windows = collections.namedtuple('Windows', 'seq start len')       # host int32 arrays [n_windows]


def window_table(lengths, max_len=None, stride=None, holdout=1):
    """-> Windows: the training windows of sequences of `lengths` items, sequence by sequence.  The training view of a sequence
    of n items is [0, T), T = max(n - holdout, 0).  max_len None: one window (0, T) each.  Otherwise T <= max_len: one window
    (0, T), none for T = 0; T > max_len: windows of max_len items at the starts T - max_len - j stride, j = 0, 1, .. while
    positive, then at 0 -- 1 + ceil((T - max_len) / stride) of them, the first ending at T.  No Python loop over sequences."""
    lengths = np.asarray(lengths, dtype=np.int64)
    T = np.maximum(lengths - holdout, 0)
    if max_len is None:
        return Windows(np.arange(len(T), dtype=np.int32), np.zeros(len(T), np.int32), T.astype(np.int32))
    count = np.where(T > 0, 1 + -(-np.maximum(T - max_len, 0) // stride), 0)
    seq = np.repeat(np.arange(len(T), dtype=np.int64), count)
    j = np.arange(len(seq), dtype=np.int64) - (np.cumsum(count) - count)[seq]
    start = np.maximum(T[seq] - max_len - j * stride, 0)
    return Windows(seq.astype(np.int32), start.astype(np.int32), np.minimum(T[seq], max_len).astype(np.int32))


class Feature:
    """One side feature of the click paths, categorical: values are integers in [0, size).
    per='event': one value per token, aligned with the data set's `items` array (an action type, a dwell bucket);
    per='item': a table of V values, one per item (a category, a brand, a popularity bucket).
    on_mask='mask' (default): a [MASK] position of the item row is [MASK] in this feature too -- what a function of the item needs,
    or it gives the target away; 'keep': the value stays visible there (a feature of the event usually should).
    The model's vocabulary of the feature has `size` tokens: id = value + 10, as for items."""

    def __init__(self, values, size, per='event', on_mask='mask'):
        if per not in ops.FEAT_KINDS:
            raise ValueError("Feature: per = %r ('event' or 'item')" % (per,))
        if on_mask not in ops.FEAT_ON_MASK:
            raise ValueError("Feature: on_mask = %r ('mask' or 'keep')" % (on_mask,))
        self.values, self.size, self.per, self.on_mask = np.asarray(values), int(size), per, on_mask


class DeviceCloze:
    """items: item indices of every sequence back to back (label space: input id = 10 + index), offsets [n_seq + 1]: their
    CSR bounds -- numpy arrays or CPU tensors, as data/beauty_sequences.npz holds them.  V: vocabulary size (labels are float32,
    the reference's format, and must be exact: V <= 2^24).  device=None keeps the host side only (no batches can be built).
    max_len (None: whole sequences), stride (None: max_len; 1 .. max_len): the training windows (window_table) and the
    evaluation rows' length; holdout 1 (the last item is the test target) or 2 (the penultimate is the validation target too);
    last_item_rate in [0, 1]: the share of training rows that mask only their last position.
    features: {name: Feature}, at most B4C_MAX_FEATURES - 1 side features beside the items; every batch dict then has 'features'."""

    def __init__(self, items, offsets, V=None, max_masked=MAX_MASKED_ITEMS, masked_percentage=MASKED_PERCENTAGE, device='cuda',
                 max_len=None, stride=None, holdout=1, last_item_rate=0.0, features=None):
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
        if max_len is not None and not 1 <= int(max_len) <= ops.CLOZE_MAX_WIDTH:
            raise ValueError('DeviceCloze: max_len = %d (1 .. %d, or None)' % (max_len, ops.CLOZE_MAX_WIDTH))
        if stride is not None and (max_len is None or not 1 <= int(stride) <= int(max_len)):
            raise ValueError('DeviceCloze: stride = %d (1 .. max_len = %s)' % (stride, max_len))
        if holdout not in (1, 2):
            raise ValueError('DeviceCloze: holdout = %r (1: test item, 2: validation and test items)' % (holdout,))
        if not 0.0 <= float(last_item_rate) <= 1.0:
            raise ValueError('DeviceCloze: last_item_rate = %g outside [0, 1]' % last_item_rate)
        if float(last_item_rate) > 0.0 and int(max_masked) < 1:
            raise ValueError('DeviceCloze: last_item_rate = %g needs max_masked >= 1' % last_item_rate)
        self.max_masked, self.masked_percentage = int(max_masked), float(masked_percentage)
        self.max_len = None if max_len is None else int(max_len)
        self.stride = self.max_len if stride is None else int(stride)
        self.holdout, self.last_item_rate = int(holdout), float(last_item_rate)
        self.last_thr = ops.cloze_last_thr(self.last_item_rate)
        self.items, self.offsets, self.lengths = items, offsets, lengths
        self.n_seq = len(lengths)
        self.windows = window_table(lengths, self.max_len, self.stride, self.holdout)
        self.n_windows = len(self.windows.seq)
        self._win_count = np.bincount(self.windows.seq, minlength=self.n_seq)
        self._win_first = np.cumsum(self._win_count) - self._win_count
        self._eval = {}                                              # split -> (Windows, device tensors)
        self._next_tr, self._next_ev = None, {}                      # the next-item rows' target counts: TRAIN table, split -> EVAL tables
        self._tgt_index = None                                       # the same-target index of views(): host arrays, device tensors
        self.features = self._check_features(features)              # name -> (int32 host values, Feature)
        self.items_dev = self.offsets_dev = self.windows_dev = None
        self._feature_sources = []                                   # (device values, per, on_mask) in the order of self.features
        if device is not None:
            self.items_dev = torch.from_numpy(items).to(device)
            self.offsets_dev = torch.from_numpy(offsets).to(device)
            self.windows_dev = tuple(torch.from_numpy(a).to(device) for a in self.windows)
            self._feature_sources = [(torch.from_numpy(v).to(device), f.per, f.on_mask) for v, f in self.features.values()]

    @classmethod
    def from_npz(cls, path, **kw):
        z = np.load(path, allow_pickle=False)
        return cls(z['items'], z['offsets'], V=int(z['vocab'].shape[0]), **kw)

    # ---- side features ------------------------------------------------------------------------------------------------------------
    def _check_features(self, features):
        """{name: Feature} -> {name: (int32 host values, Feature)}: every check the device does not make, once, on the host"""
        out = collections.OrderedDict()
        if not features:
            return out
        if len(features) > ops.L.MAX_FEATURES - 1:
            raise ValueError('DeviceCloze: %d features %s; at most %d beside the items (B4C_MAX_FEATURES = %d)'
                             % (len(features), sorted(features), ops.L.MAX_FEATURES - 1, ops.L.MAX_FEATURES))
        for name, f in features.items():
            if not isinstance(name, str) or not isinstance(f, Feature):
                raise ValueError('DeviceCloze: features maps names to cloze_batches.Feature objects, got %r: %s' % (name, type(f).__name__))
            v = f.values
            want = len(self.items) if f.per == 'event' else self.V
            if v.ndim != 1 or len(v) != want:
                raise ValueError("DeviceCloze: feature %r is per %r: %s values, %d %s" % (
                    name, f.per, 'x'.join(str(d) for d in v.shape), want, 'tokens in items' if f.per == 'event' else 'items (V)'))
            if v.dtype.kind not in 'iu':
                raise ValueError('DeviceCloze: feature %r: values of dtype %s; integers are needed' % (name, v.dtype))
            if f.size < 1 or (len(v) and (int(v.min()) < 0 or int(v.max()) >= f.size)):
                raise ValueError('DeviceCloze: feature %r: values outside [0, size = %d)' % (name, f.size))
            out[name] = (np.ascontiguousarray(v, dtype=np.int32), f)
        return out

    def _features(self, layout, table_dev, row_dev, W, items_in, holdout=1):
        """{name: (B, W) int64 ids} of the rows whose item rows items_in were just built (one launch: ops.batch_features)"""
        win = table_dev if table_dev is not None else (None, None, None)
        outs = ops.batch_features(self.items_dev, self.offsets_dev, win[0], win[1], win[2], row_dev, W, layout, items_in,
                                  self._feature_sources, holdout=holdout, max_len=self.max_len)
        return dict(zip(self.features, outs))

    @staticmethod
    def inputs(batch, item_feature):
        """the model's input dict of a batch: its items under the model's name for them, beside its side features -- what forward,
        cloze_loss, candidate_loss and predict_topk take"""
        return {item_feature: batch['items'], **batch.get('features', {})}

    # ---- the evaluation rows: one per sequence and split ------------------------------------------------------------------
    def _drop(self, split):
        """items from the sequence's end to the split's target, the target included"""
        if split not in _SPLITS or (split == 'valid' and self.holdout != 2):
            raise ValueError('DeviceCloze: split %r (holdout = %d: %s)' % (split, self.holdout, "'valid' or 'test'" if self.holdout == 2
                                                                           else "'test' only; 'valid' needs holdout=2"))
        return 2 if split == 'valid' else 1

    def _eval_table(self, split):
        """(Windows, device tensors) of the split: sequence g's row is the last min(t + 1, max_len) positions ending at its
        target t = n_g - drop, empty when the sequence is too short to have one"""
        if split not in self._eval:
            end = np.maximum(self.lengths - self._drop(split) + 1, 0)
            start = np.zeros_like(end) if self.max_len is None else np.maximum(end - self.max_len, 0)
            table = Windows(np.arange(self.n_seq, dtype=np.int32), start.astype(np.int32), (end - start).astype(np.int32))
            dev = None if self.items_dev is None else tuple(torch.from_numpy(a).to(self.items_dev.device) for a in table)
            self._eval[split] = (table, dev)
        return self._eval[split]

    def row_lengths(self, seq_idx, mode, split='test'):
        """host: L of the row of every named sequence (TRAIN: of each of its windows; EVAL: of the split's row)"""
        seq = np.asarray(seq_idx, dtype=np.int64)
        if _MODES[mode] == ops.CLOZE_EVAL:
            return self._eval_table(split)[0].len[seq].astype(np.int64)
        T = np.maximum(self.lengths[seq] - self.holdout, 0)
        return T if self.max_len is None else np.minimum(T, self.max_len)

    def n_real_tokens(self, seq_idx, mode, split='test'):
        """host int: non-pad positions of the chained batch = sum of the row lengths + [CLS] [SEP] .. [SEP] per row"""
        L = self.row_lengths(seq_idx, mode, split)
        return int(L.sum()) + 3 * len(L)

    def _width(self, L, width):
        longest = int(L.max()) if len(L) else 0
        if width is not None and int(width) < longest:
            raise ValueError('DeviceCloze: width = %d is shorter than a row of %d items' % (width, longest))
        W = max(longest, 1) if width is None else int(width)
        if W > ops.CLOZE_MAX_WIDTH:
            raise ValueError('DeviceCloze: a row of %d items; at most %d' % (W, ops.CLOZE_MAX_WIDTH))
        return W

    def _batch(self, table, row_host, row_dev, seq_dev, mode, seed, width):
        """rows row_host (window indices of `table` = (Windows, device tensors); negative: an empty row) -> the batch dict"""
        host, dev = table
        row_host = np.asarray(row_host, dtype=np.int64)
        L = np.where(row_host >= 0, host.len[np.maximum(row_host, 0)], 0).astype(np.int64)
        W = self._width(L, width)
        self._need_device()
        items, lab, nm = ops.cloze_batch_windows(self.items_dev, self.offsets_dev, dev[0], dev[1], dev[2], row_dev, W, _MODES[mode], seed,
                                                 self.masked_percentage, self.max_masked, last_thr=self.last_thr)
        row_dev._host_rows = (_MODES[mode] == ops.CLOZE_TRAIN, row_host)       # (what views() computes its host counts from)
        out = {'items': items, 'labels_padded': lab, 'n_masked': nm, 'seq_idx': seq_dev, 'win_idx': row_dev,
               'n_real_tokens': int(L.sum()) + 3 * len(L)}
        if self.features:
            out['features'] = self._features(ops.FEAT_CLOZE, dev, row_dev, W, items)
        return out

    def _need_device(self):
        if self.items_dev is None:
            raise ValueError('DeviceCloze: built with device=None (host side only)')

    def _check_seq(self, seq_idx):
        seq = np.asarray(seq_idx, dtype=np.int64).reshape(-1)
        if len(seq) and (seq.min() < 0 or seq.max() >= self.n_seq):
            raise ValueError('DeviceCloze: sequence indices outside [0, %d)' % self.n_seq)
        return seq

    def _upload(self, a):
        return None if self.items_dev is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.items_dev.device)

    def batch(self, seq_idx, mode, seed=0, width=None, split='test'):
        """One batch of the sequences seq_idx (host integers, any order, repeats allowed) -> dict(items (B, W) int64,
        labels_padded (B, M) float32 -- M = max_masked for TRAIN, 1 for EVAL --, n_masked (B,) int32, seq_idx, win_idx int32:
        device tensors; n_real_tokens: host int).  width None: the batch's longest row (as BeautyCloze pads); an int fixes W.
        TRAIN: the one window of every sequence (a sequence cut into several windows: window_batch); EVAL: the row of `split`."""
        seq = self._check_seq(seq_idx)
        if _MODES[mode] == ops.CLOZE_EVAL:
            return self._batch(self._eval_table(split), seq, self._upload(seq), self._upload(seq), mode, seed, width)
        count = self._win_count[seq]
        if (count > 1).any():
            g = int(seq[np.argmax(count > 1)])
            raise ValueError('DeviceCloze: sequence %d has %d training windows (max_len = %d); name them with window_batch'
                             % (g, self._win_count[g], self.max_len))
        rows = np.where(count == 1, self._win_first[seq], -1)
        return self._batch((self.windows, self.windows_dev), rows, self._upload(rows), self._upload(seq), mode, seed, width)

    def window_batch(self, win_idx, seed=0, width=None):
        """One TRAIN batch of the windows win_idx (host indices into self.windows, any order, repeats allowed)"""
        win = np.asarray(win_idx, dtype=np.int64).reshape(-1)
        if len(win) and (win.min() < 0 or win.max() >= self.n_windows):
            raise ValueError('DeviceCloze: window indices outside [0, %d)' % self.n_windows)
        return self._batch((self.windows, self.windows_dev), win, self._upload(win), self._upload(self.windows.seq[win]), TRAIN, seed, width)

    def epoch_order(self, seed, epoch):
        return np.random.default_rng([int(seed), int(epoch)]).permutation(self.n_windows)

    def rank_slices(self, batch_size, seed, epoch, rank=0, world=1):
        """host: (order, [(lo, hi), ...]) -- epoch `epoch`'s permutation of the windows and rank `rank`'s slice of every full
        global batch of batch_size * world consecutive entries (the remainder is dropped, as BeautyCloze does)"""
        if not (batch_size > 0 and 0 <= rank < world):
            raise ValueError('DeviceCloze: batch_size = %d, rank %d of %d' % (batch_size, rank, world))
        order = self.epoch_order(seed, epoch)
        G = batch_size * world
        return order, [(s + rank * batch_size, s + (rank + 1) * batch_size) for s in range(0, self.n_windows - G + 1, G)]

    def _epoch_steps(self, batch_size, seed, steps, rank, world, seq_of):
        """`steps` times (order, order_dev, seq_dev, epoch seed): rank `rank`'s slice of the next global batch of the epoch's
        seeded permutation of the windows -- uploaded once per epoch, seq_dev = seq_of(the uploaded order) sliced with it -- and
        the epoch's seed rand64_host(seed, e)"""
        self._need_device()
        order, slices = self.rank_slices(batch_size, seed, 0, rank, world)
        if steps > 0 and not slices:
            raise ValueError('DeviceCloze: %d %s do not fill one batch of %d x %d'
                             % (self.n_windows, 'sequences' if self.max_len is None else 'windows', batch_size, world))
        done = epoch = 0
        while done < steps:
            if epoch:
                order, slices = self.rank_slices(batch_size, seed, epoch, rank, world)
            order_dev = self._upload(order)
            seq_dev = seq_of(order_dev)
            epoch_seed = int(ops.rand64_host(seed, epoch))
            for lo, hi in slices[:steps - done]:
                yield order[lo:hi], order_dev[lo:hi], seq_dev[lo:hi], epoch_seed
            done += len(slices)
            epoch += 1

    def train_batches(self, batch_size, seed, steps, rank=0, world=1, width=None):
        """`steps` TRAIN batches of batch_size windows for rank `rank` of `world`: one seeded permutation per epoch (uploaded
        once), the mask seed of epoch e is rand64_host(seed, e)."""
        table = (self.windows, self.windows_dev)
        seq_of = lambda o: o if self.max_len is None else self.windows_dev[0][o.long()]      # (a window's sequence)
        for order, order_dev, seq_dev, mask_seed in self._epoch_steps(batch_size, seed, steps, rank, world, seq_of):
            yield self._batch(table, order, order_dev, seq_dev, TRAIN, mask_seed, width)

    def eval_batches(self, batch_size, limit=None, width=None, split='test'):
        """EVAL batches of the sequences 0 .. limit in order, the last one partial; split 'test' (the last item) or, with
        holdout=2, 'valid' (the penultimate).  An empty sequence, or one too short to have the target, gives a row without a
        [MASK] whose label column is -1: compact labels taken from labels_padded then need the rows with n_masked == 1."""
        table = self._eval_table(split)
        self._need_device()
        n = self.n_seq if limit is None else min(int(limit), self.n_seq)
        seq = np.arange(n, dtype=np.int64)
        seq_dev = torch.arange(n, dtype=torch.int32, device=self.items_dev.device)
        for s in range(0, n, batch_size):
            yield self._batch(table, seq[s:s + batch_size], seq_dev[s:s + batch_size], seq_dev[s:s + batch_size], EVAL, 0, width)

    # ---- next-item batches: every real position predicts the item after it (include/b4c.h) -------------------------
    def next_item_counts(self, win_idx):
        """host int64: inputs (= targets) of the TRAIN next-item row of every named window; a negative index: 0.  A window at
        a > 0 takes one extra input in front, the first window of a sequence gives up its last item as a target only."""
        win = np.asarray(win_idx, dtype=np.int64).reshape(-1)
        return np.where(win >= 0, self._next_train()[0][np.maximum(win, 0)], 0)

    def next_item_sizes(self, win_idx):
        """host (n_targets, n_real_tokens) of the TRAIN next-item batch of the named windows"""
        n_in = self.next_item_counts(win_idx)
        return int(n_in.sum()), int(n_in.sum()) + 3 * len(n_in)

    def _next_train(self):
        """(host int64 [n_windows], device int32 [n_windows]): the target count of every window's row, uploaded once"""
        if self._next_tr is None:
            w = self.windows
            n_in = np.where(w.start > 0, w.len, np.maximum(w.len - 1, 0)).astype(np.int64)
            self._next_tr = (n_in, self._upload(n_in))
        return self._next_tr

    def _next_eval(self, split):
        """split -> (n_in host [n_seq], has-target host [n_seq], has-target device int32, first compact row of every sequence
        host [n_seq + 1], the sequences that have a target device int32): sequence g's row is the most recent
        min(t, max_len) items in front of its target t = n_g - drop; t < 1: no target"""
        if split not in self._next_ev:
            t = self.lengths - self._drop(split)
            n_in = np.maximum(t, 0) if self.max_len is None else np.minimum(np.maximum(t, 0), self.max_len)
            has = (t >= 1).astype(np.int64)
            first = np.concatenate([[0], np.cumsum(has)])
            self._next_ev[split] = (n_in.astype(np.int64), has, self._upload(has), first, self._upload(np.flatnonzero(has)))
        return self._next_ev[split]

    def _next_batch(self, mode, row_host, row_dev, seq_dev, n_in, n_tgt, cnt_dev, seed, width, num_negatives, exclude, item_cdf, rows,
                    holdout):
        """rows row_host (TRAIN: window indices, EVAL: sequences; negative: an empty row) with their host-known input and target
        counts, and the device table cnt_dev of target counts that row_dev indexes -> the batch dict"""
        W = self._width(n_in, width)
        R = int(n_tgt.sum())
        if rows is not None and int(rows) < R:
            raise ValueError('DeviceCloze: rows = %d for a batch of %d targets' % (rows, R))
        self._need_device()
        B = len(row_host)
        cnt = cnt_dev[row_dev.clamp(min=0).long()] * (row_dev >= 0)
        row_off = torch.zeros(B + 1, dtype=torch.int32, device=row_dev.device)
        row_off[1:] = torch.cumsum(cnt, 0)
        win = self.windows_dev if mode == ops.NEXT_TRAIN else (None, None, None)
        items, flat, lab, cand, short = ops.next_item_batch(
            self.items_dev, self.offsets_dev, win[0], win[1], win[2], row_dev, row_off, W, mode, R, self.V, holdout=holdout,
            max_len=self.max_len, num_negatives=num_negatives, seed=seed, exclude=exclude, item_cdf=item_cdf, rows=rows)
        row_dev._host_rows = (mode == ops.NEXT_TRAIN, np.asarray(row_host, dtype=np.int64))
        out = {'items': items, 'flat_idx': flat, 'labels': lab, 'candidates': cand, 'row_offsets': row_off, 'short': short,
               'seq_idx': seq_dev, 'win_idx': row_dev, 'n_targets': R, 'n_real_tokens': int(n_in.sum()) + 3 * B}
        if self.features:
            train = mode == ops.NEXT_TRAIN
            out['features'] = self._features(ops.FEAT_NEXT_TRAIN if train else ops.FEAT_NEXT_EVAL, self.windows_dev if train else None,
                                             row_dev, W, items, holdout)
        return out

    def next_item_window_batch(self, win_idx, seed=0, width=None, num_negatives=0, exclude='history', item_cdf=None, rows=None):
        """One TRAIN next-item batch of the windows win_idx (host indices into self.windows, any order, repeats allowed; negative:
        an empty row) -> dict(items (B, W) int64 -- no [MASK] --, flat_idx [R] int32, labels [R] int32, candidates [R, 1 + N]
        int32 or None, row_offsets [B + 1] int32, short int32 [1], seq_idx, win_idx: device tensors; n_targets = R,
        n_real_tokens: host ints): what model.next_item_loss takes.  rows: a fixed compact row count >= R (the rest all -1).
        num_negatives, exclude ('history': never an item of the sequence's training view; None), item_cdf (device int64 [V]):
        each target's own negatives, a pure function of (seed, the target token)."""
        win = np.asarray(win_idx, dtype=np.int64).reshape(-1)
        if len(win) and win.max() >= self.n_windows:
            raise ValueError('DeviceCloze: window indices outside [0, %d)' % self.n_windows)
        n_in = self.next_item_counts(win)
        seq = np.where(win >= 0, self.windows.seq[np.maximum(win, 0)] if self.n_windows else 0, -1)
        return self._next_batch(ops.NEXT_TRAIN, win, self._upload(win), self._upload(seq), n_in, n_in, self._next_train()[1], seed, width,
                                num_negatives, exclude, item_cdf, rows, self.holdout)

    def next_item_batches(self, batch_size, seed, steps, rank=0, world=1, width=None, num_negatives=0, exclude='history', item_cdf=None,
                          rows=None):
        """`steps` TRAIN next-item batches of batch_size windows for rank `rank` of `world`: train_batches' epoch permutation
        (uploaded once per epoch), rank slices and per-epoch seed rand64_host(seed, e); no per-batch upload."""
        seq_of = lambda o: self.windows_dev[0][o.long()]
        for order, order_dev, seq_dev, draw_seed in self._epoch_steps(batch_size, seed, steps, rank, world, seq_of):
            n_in_all, cnt_dev = self._next_train()
            n_in = n_in_all[order]
            yield self._next_batch(ops.NEXT_TRAIN, order, order_dev, seq_dev, n_in, n_in, cnt_dev, draw_seed, width, num_negatives, exclude,
                                   item_cdf, rows, self.holdout)

    def next_item_eval_batches(self, batch_size, limit=None, width=None, split='test'):
        """EVAL next-item batches of the sequences 0 .. limit in order, the last one partial: every row is the most recent
        max_len items in front of the split's target, unmasked, and has ONE compact row -- at its last input -- whose label is
        the target; a sequence with nothing in front of its target has none.  Beside next_item_window_batch's keys:
        'target_seq_idx' int32 [R], the sequence of every compact row (history(b['target_seq_idx'], split) is their exclude=)."""
        n_in_all, has, has_dev, first, tgt_seq_dev = self._next_eval(split)
        drop = self._drop(split)
        self._need_device()
        n = self.n_seq if limit is None else min(int(limit), self.n_seq)
        seq = np.arange(n, dtype=np.int64)
        seq_dev = torch.arange(n, dtype=torch.int32, device=self.items_dev.device)
        for s in range(0, n, batch_size):
            e = min(s + batch_size, n)
            b = self._next_batch(ops.NEXT_EVAL, seq[s:e], seq_dev[s:e], seq_dev[s:e], n_in_all[s:e], has[s:e], has_dev, 0, width, 0, None,
                                 None, None, drop)
            b['target_seq_idx'] = tgt_seq_dev[int(first[s]):int(first[e])]
            yield b

    # ---- contrastive views of a training batch (include/b4c.h) ---------------------------------------------------------------
    VIEW_OBJECTIVES = {'cloze': ops.FEAT_CLOZE, 'next_item': ops.FEAT_NEXT_TRAIN}

    def target_index(self):
        """host (tgt_first int64 [V + 1], tgt_tok int64 [n], tgt_seq int32 [n], key int64 [n]): the same-target index -- every
        token at position q of its sequence with 1 <= q < T_g (a target of the training view with an input in front of it), in the
        order (item, token index); item y's list is tgt_tok[tgt_first[y] .. tgt_first[y + 1]).  key = item * (n_tok + 1) + token,
        ascending: the host's search array.  Built once, with numpy, and uploaded once."""
        if self._tgt_index is None:
            n_tok = len(self.items)
            pos = np.arange(n_tok, dtype=np.int64) - np.repeat(self.offsets[:-1], self.lengths)
            tok = np.flatnonzero((pos >= 1) & (pos < np.repeat(np.maximum(self.lengths - self.holdout, 0), self.lengths))).astype(np.int64)
            tok = tok[np.argsort(self.items[tok], kind='stable')]
            seq = np.repeat(np.arange(self.n_seq, dtype=np.int32), self.lengths)[tok]
            y = self.items[tok].astype(np.int64)
            first = np.concatenate([[0], np.cumsum(np.bincount(y, minlength=self.V))]).astype(np.int64)
            host = (first, tok, seq, y * (n_tok + 1) + tok)
            dev = None
            if self.items_dev is not None:
                dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.items_dev.device) for a in host[:3])
            self._tgt_index = (host, dev)
        return self._tgt_index[0]

    def _view_rows(self, win, layout, W):
        """host int64 [B]: (i, n) of the named windows' source rows -- the CSR index of the first token and the token count of
        the row rule of include/b4c.h (an empty row: n = 0)"""
        ok = win >= 0
        w = np.where(ok, win, 0)
        if not self.n_windows:
            return np.zeros(len(win), np.int64), np.zeros(len(win), np.int64)
        g, a, L = (t[w].astype(np.int64) for t in self.windows)
        if layout == ops.FEAT_CLOZE:
            first, n = a, np.minimum(L, W)
        else:
            T = np.maximum(self.lengths[g] - self.holdout, 0)
            first = np.where(a > 0, a - 1, 0)
            n = np.maximum(np.minimum(np.minimum(np.where(a > 0, L, L - 1), W), T - first - 1), 0)
        return self.offsets[g] + first, np.where(ok, n, 0)

    def view_lengths(self, win_idx, seed, ops=('crop', 'mask', 'reorder'), n_views=2, objective='next_item', width=None, crop_ratio=0.6,
                     mask_ratio=0.3, reorder_ratio=0.6):
        """host int64 [n_views, B]: the item count of every view views() builds of the windows win_idx at width W (None: the longest
        source row) -- the rule of include/b4c.h as far as the lengths need it (the op, then the length), evaluated with
        ops.rand64_host and numpy from the window table, the offsets and the same-target index: no loop over rows, no device work."""
        who = 'DeviceCloze.view_lengths'
        if objective not in self.VIEW_OBJECTIVES:
            raise ValueError("DeviceCloze: objective %r ('cloze' or 'next_item')" % (objective,))
        layout = self.VIEW_OBJECTIVES[objective]
        win = np.asarray(win_idx, dtype=np.int64).reshape(-1)
        if len(win) and win.max() >= self.n_windows:
            raise ValueError('DeviceCloze: window indices outside [0, %d)' % self.n_windows)
        W = int(width) if width is not None else max(int(self._view_rows(win, layout, _ops.CLOZE_MAX_WIDTH)[1].max()) if len(win) else 0, 1)
        W, layout, _, max_len, n_views, mask, crop_ratio, mask_ratio, reorder_ratio = _ops._augment_args(
            who, W, layout, self.holdout, self.max_len, n_views, ops, seed, crop_ratio, mask_ratio, reorder_ratio)
        i, n = self._view_rows(win, layout, W)
        ctr = i.astype(np.uint64)
        enabled = np.array([bit for bit in _ops.AUG_OPS.values() if mask & bit], dtype=np.int64)
        share = lambda ratio: (n.astype(np.float32) * np.float32(ratio)).astype(np.int64)
        same = bool(mask & _ops.L.AUG_SAME_TARGET)
        if same:
            first, tok, seq, key = self.target_index()
            t = np.where(n > 0, i + n, 0)
            y = self.items[t].astype(np.int64) if len(self.items) else np.zeros(len(t), np.int64)
            want = y * (len(self.items) + 1) + t
            at = np.searchsorted(key, want, side='left')
            found = (at < len(key)) & (key[np.minimum(at, max(len(key) - 1, 0))] == want) if len(key) else np.zeros(len(t), bool)
            own = at - first[y]
            others = first[y + 1] - first[y] - found
        out = np.zeros((n_views, len(win)), np.int64)
        for v in range(n_views):
            seed_v = int(_ops.rand64_host(int(seed) ^ 0xA0761D6478BD642F, np.array([v], np.uint64))[0])
            op = enabled[_ops.mulhi64_host(_ops.rand64_host(seed_v ^ 0xE7037ED1A0B428DB, ctr), len(enabled)).astype(np.int64)]
            length = np.where(op == _ops.L.AUG_CROP, np.maximum(share(crop_ratio), 1), n)
            if same and len(key):
                h_at = _ops.rand64_host(seed_v ^ 0x8EBC6AF09C88C6E3, ctr)
                u = _ops.mulhi64_host(h_at, np.maximum(others, 1)).astype(np.int64)
                k = np.minimum(first[y] + u + (found & (u >= own)), len(key) - 1)
                q = tok[k] - self.offsets[seq[k]]
                length = np.where((op == _ops.L.AUG_SAME_TARGET) & (others > 0), np.minimum(np.minimum(q, W), max_len), length)
            out[v] = np.where(n > 0, length, 0)
        return out

    def views(self, batch, seed, ops=('crop', 'mask', 'reorder'), n_views=2, objective=None, crop_ratio=0.6, mask_ratio=0.3, reorder_ratio=0.6,
              win_idx=None):
        """n_views contrastive views of a TRAIN batch's rows, built on the device in one launch (ops.augment_views, include/b4c.h)
        -> a list of n_views dicts(items (B, W) int64 -- W the batch's own width --, n_items, op, target (B,) int32, src_tok (B, W)
        int64: device tensors; n_real_tokens: host int; features {name: (B, W) int64} when the data set has side features; self_count
        int32 [1], shared: the 'same_target' rows that had no partner).
        ops: the operators one of which is drawn per (row, view) -- CL4SRec: ('crop', 'mask', 'reorder'); DuoRec's supervised
        positive: ('same_target',), next-item batches only: the inputs in front of another occurrence of the row's target.
        objective 'cloze' (the views are cut from the batch's UNMASKED windows) or 'next_item'; None: 'next_item' for a batch with
        'row_offsets'.  A view is a pure function of (seed, view, window); the training generators' per-epoch seed is
        rand64_host(seed, epoch).  contrastive_loss(inputs, inputs_b={name: view['items'], ...}, n_real_tokens_b=view['n_real_tokens'])
        takes a view; 'target' is its same_target=.
        The batch's windows are read from batch['win_idx'] on the device; the host count needs them on the host: the batches this
        class builds remember them, for any other batch pass win_idx (host integers)."""
        self._need_device()
        if objective is None:
            objective = 'next_item' if 'row_offsets' in batch else 'cloze'
        if objective not in self.VIEW_OBJECTIVES:
            raise ValueError("DeviceCloze: objective %r ('cloze' or 'next_item')" % (objective,))
        row_dev = batch['win_idx']
        if win_idx is None:
            train, win_idx = getattr(row_dev, '_host_rows', (True, None))
            if win_idx is None:
                raise ValueError("DeviceCloze.views: batch['win_idx'] was not built by this class; pass win_idx (host integers)")
            if not train:
                raise ValueError('DeviceCloze.views: an evaluation batch; views are built of training rows')
        win = np.asarray(win_idx, dtype=np.int64).reshape(-1)
        B, W = batch['items'].shape
        if len(win) != B or row_dev.shape[0] != B:
            raise ValueError('DeviceCloze.views: %d window indices for a batch of %d rows' % (len(win), B))
        n_items = self.view_lengths(win, seed, ops, n_views, objective, W, crop_ratio, mask_ratio, reorder_ratio)
        view_ops = (ops,) if isinstance(ops, str) else tuple(ops)
        index = None
        if 'same_target' in view_ops:
            self.target_index()
            index = self._tgt_index[1]
        tab = self.windows_dev
        items, tok, n_out, op, target, self_count = _ops.augment_views(
            self.items_dev, self.offsets_dev, tab[0], tab[1], tab[2], row_dev, W, self.VIEW_OBJECTIVES[objective], view_ops, seed,
            n_views=n_views, holdout=self.holdout, max_len=self.max_len, crop_ratio=crop_ratio, mask_ratio=mask_ratio,
            reorder_ratio=reorder_ratio, target_index=index, V=self.V)
        out = []
        for v in range(int(n_views)):
            view = {'items': items[v], 'n_items': n_out[v], 'op': op[v], 'target': target[v], 'src_tok': tok[v],
                    'n_real_tokens': int(n_items[v].sum()) + 3 * B, 'self_count': self_count}
            if self.features:
                view['features'] = self._view_features(items[v], tok[v])
            out.append(view)
        return out

    def _view_features(self, items, src_tok):
        """{name: (B, W) int64 ids} of one view, gathered in torch through src_tok (the CSR index of every position's token, -1 at
        pad): per 'event' values[src_tok], per 'item' table[items[src_tok]]; id = value + 10, pad 0, [MASK] where the item row has
        it unless the feature keeps its value there"""
        real = src_tok >= 0
        at = src_tok.clamp(min=0)
        out = {}
        for name, (values, per, on_mask) in zip(self.features, self._feature_sources):
            src = values[at] if per == 'event' else values[self.items_dev[at].long()]
            ids = torch.where(real, src.to(torch.int64) + 10, torch.zeros_like(src_tok))
            if on_mask == 'mask':
                ids = torch.where(items == 1, torch.ones_like(ids), ids)
            out[name] = ids
        return out

    # ---- filtered evaluation ---------------------------------------------------------------------------------------------------
    def history(self, seq_idx_dev, split='test', width=None):
        """(B, E) int32 device tensor: every item of the sequences seq_idx_dev (a batch's 'seq_idx') in front of the split's
        target, whether the row's window holds it or not -- the `exclude=` of predict_topk, of the ranking metrics and of
        cloze.sample_candidates.  width None: E = the longest history of the data set, at most ops.L.MAX_EXCL; more items than E:
        the most recent E."""
        drop = self._drop(split)
        self._need_device()
        if width is None:
            width = min(max(int(self.lengths.max()) - drop if self.n_seq else 0, 1), ops.L.MAX_EXCL)
        return ops.cloze_history(self.items_dev, self.offsets_dev, seq_idx_dev, width, drop)

    def item_counts(self, split='train'):
        """host int64 [V]: how often every item occurs in the training views (all but the `holdout` last items of every
        sequence) -- the popularity the negative sampler draws by, free of held-out items"""
        if split != 'train':
            raise ValueError("DeviceCloze: item_counts(split=%r): 'train' only" % (split,))
        pos = np.arange(len(self.items), dtype=np.int64) - np.repeat(self.offsets[:-1], self.lengths)
        return np.bincount(self.items[pos < np.repeat(self.lengths - self.holdout, self.lengths)], minlength=self.V).astype(np.int64)
