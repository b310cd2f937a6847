"""Cloze (masked-item) loss and ranking metrics of the BERT4Rec example
(reference examples/BERT4Rec/source/utils.py:56-259), over the HIP kernels.

y_true: (B, M) labels padded with -1;  y_pred: (B, M, V) probabilities (or any monotone score for
the metrics).  All accumulators live on the device; ``result()`` returns a 0-d tensor."""
import math
import weakref

import torch

from . import ops
from .clickstream_transformer.constants import LABEL_PAD, NUM_RESERVED_TOKENS
from .clickstream_transformer.losses import MaskedLoss


def cloze_output_adaptor(y_true, y_pred):
    """Flatten to (B*M, 1) / (B*M, V) and drop rows whose label is the pad (utils.py:104-113)."""
    V = y_pred.shape[-1]
    yp = y_pred.reshape(-1, V)
    yt = torch.as_tensor(y_true, device=y_pred.device).reshape(-1, 1)
    keep = yt[:, 0] != LABEL_PAD
    return yt[keep], yp[keep]


class ClozeMaskedLoss:
    def __init__(self, item_wise_loss_fn, label_pad=LABEL_PAD):
        self.masked_loss = MaskedLoss(item_wise_loss_fn=item_wise_loss_fn, label_pad=label_pad)

    def __call__(self, y_true, y_pred):
        # MaskedLoss already ignores pad labels; dropping the rows first (as the reference does)
        # changes nothing numerically and would cost a copy of the (B*M, V) tensor.
        return self.masked_loss(torch.as_tensor(y_true, device=y_pred.device).reshape(-1), y_pred.reshape(-1, y_pred.shape[-1]))


def seen_items(item_ids, label_offset=NUM_RESERVED_TOKENS):
    """(B, S) input ids of a batch -> (B, S) int64 label-space history (input id - label_offset), -1 where the id is a
    reserved token ([PAD], [MASK], [CLS], [SEP], ...): the `exclude=` of predict_topk / the ranking metrics that leaves out
    the items a sequence already holds ("filtered" evaluation)."""
    ids = torch.as_tensor(item_ids)
    if ids.dtype.is_floating_point or ids.dtype == torch.bool:
        raise TypeError('seen_items: integer item ids are needed, got %s' % ids.dtype)
    ids = ids.to(torch.int64)
    return torch.where(ids >= label_offset, ids - label_offset, torch.full_like(ids, -1))


def _exclude_key(exclude):
    if exclude is None:
        return None
    if isinstance(exclude, torch.Tensor):
        return (exclude.data_ptr(), exclude._version, tuple(exclude.shape), exclude.dtype)
    return ('host', id(exclude))


def _row_exclusions(exclude, n_rows, y_true, V, lab, device):
    """update_state's `exclude` -> ops.exclusions lists, one per row of the flattened y_pred: (B*M, E) per row, or (B, E) per
    sequence of a (B, M) y_true (each of its M positions)"""
    ex = exclude if isinstance(exclude, torch.Tensor) else ops.exclusions(exclude, 1 << 30)
    if ex.dim() != 2:
        raise ValueError('exclude must be (rows, E) or (B, E), got shape %s' % (tuple(ex.shape),))
    ex = ex.to(device)
    if ex.shape[0] != n_rows:
        yt = torch.as_tensor(y_true)
        if yt.dim() != 2 or ex.shape[0] != yt.shape[0]:
            raise ValueError('exclude has %d lists for %d rows' % (ex.shape[0], n_rows))
        ex = ex.repeat_interleave(yt.shape[1], dim=0)
    return ops.exclusions(ex, V, lab)


def item_counts(ids, V, label_offset=NUM_RESERVED_TOKENS):
    """int64 [V] counts of each label-space item (input id - label_offset) among input ids -- the training split's, for the
    popularity sampler of sample_candidates.  Reserved tokens, padding and ids past the vocabulary are not counted."""
    t = torch.as_tensor(ids)
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError('item_counts: integer item ids are needed, got %s' % t.dtype)
    V = int(V)
    if V <= 0:
        raise ValueError('item_counts: V = %d' % V)
    t = t.reshape(-1).to(torch.int64) - int(label_offset)
    t = t[(t >= 0) & (t < V)]
    return torch.bincount(t.cpu(), minlength=V).to(torch.int64)


def log_expected_count(item_counts=None, num_items=None, num_negatives=1, device=None):
    """fp32 [V]: log of the expected number of times each item stands among the num_negatives drawn negatives of one list -- the
    logQ correction of the sampled softmax, for candidate_loss(logq=...) / next_item_loss(logq=...).  item_counts (int [V], the
    counts sample_candidates draws by: item_counts() of the training split, DeviceCloze.item_counts): log(N * count_v / total),
    and 0.0 for an item of count 0, which is never drawn and so never read.  None: uniform over num_items = V items, the constant
    log(N / V).  `device`: where the tensor is put (default: the CPU; the loss takes a device tensor).
    AN APPROXIMATION, the one TensorFlow's sampled_softmax_loss makes: the sampler rejects the row's label and its excluded
    items and draws DISTINCT items, so an item's true inclusion probability depends on the row; the correction uses the
    unconditional N * q_v.  The target stands in its list with probability 1, not N * q_y: the losses leave its score
    uncorrected unless correct_target=True."""
    N = int(num_negatives)
    if N < 1:
        raise ValueError('log_expected_count: num_negatives = %d' % N)
    if item_counts is not None:
        cnt = torch.as_tensor(item_counts)
        if cnt.dim() != 1 or cnt.dtype.is_floating_point or cnt.dtype == torch.bool:
            raise ValueError('log_expected_count: item_counts must be an integer [V] tensor')
        cnt = cnt.to(torch.int64).cpu()
        if num_items is not None and int(num_items) != cnt.shape[0]:
            raise ValueError('log_expected_count: %d item counts for num_items = %d' % (cnt.shape[0], num_items))
        if bool((cnt < 0).any()) or int(cnt.sum()) <= 0:
            raise ValueError('log_expected_count: item counts must be >= 0 with a positive total')
        q = cnt.to(torch.float64) * (float(N) / float(int(cnt.sum())))
        out = torch.where(cnt > 0, torch.log(q.clamp(min=1e-300)), torch.zeros_like(q)).to(torch.float32)
    elif num_items is None:
        raise ValueError('log_expected_count: give item_counts (popularity) or num_items (uniform)')
    else:
        V = int(num_items)
        if V <= 0:
            raise ValueError('log_expected_count: num_items = %d' % V)
        out = torch.full((V,), math.log(float(N) / V), dtype=torch.float32)
    return out if device is None else out.to(device)


def _labels_i32(y_true, device):
    yt = torch.as_tensor(y_true, device=device).reshape(-1)
    valid = yt != LABEL_PAD
    return torch.where(valid, yt, torch.full_like(yt, -1)).to(torch.int32).contiguous(), valid


def sample_candidates(y_true, num_negatives=100, exclude=None, item_counts=None, seed=0, row_base=0, num_items=None):
    """(R, 1 + N) int32 device candidate lists for the flattened rows of y_true (R = y_true.numel(), (B, M) padded with -1):
    column 0 the label, then num_negatives distinct items of [0, V) that are neither the label nor excluded -- the BERT4Rec
    paper's protocol (100 negatives ranked with the held-out item).  item_counts (int [V], e.g. item_counts() of the training
    split): drawn by popularity, items of count 0 never; None: uniform over num_items = V items.  exclude: (B, E) per sequence
    or (R, E) per row (cloze.seen_items), as update_state's.  Rows of a pad label are -1 throughout.  ops.sample_candidates
    (b4c_sample_candidates) with seed and row_base: the lists are a pure function of (seed, row_base + row, ...), so a
    data-parallel rank passes the global index of its first row as row_base."""
    cdf = None
    if item_counts is not None:
        cnt = torch.as_tensor(item_counts)
        if cnt.dim() != 1 or cnt.dtype.is_floating_point or cnt.dtype == torch.bool:
            raise ValueError('sample_candidates: item_counts must be an integer [V] tensor')
        cnt = cnt.to(torch.int64)
        if num_items is not None and int(num_items) != cnt.shape[0]:
            raise ValueError('sample_candidates: %d item counts for num_items = %d' % (cnt.shape[0], num_items))
        if bool((cnt < 0).any()) or int(cnt.sum()) <= 0:
            raise ValueError('sample_candidates: item counts must be >= 0 with a positive total')
        V = cnt.shape[0]
        cdf = torch.cumsum(cnt, 0)
    elif num_items is None:
        raise ValueError('sample_candidates: give item_counts (popularity) or num_items (uniform)')
    else:
        V = int(num_items)
    dev = torch.device('cuda')
    lab, _ = _labels_i32(y_true, dev)
    ex = None if exclude is None else _row_exclusions(exclude, lab.shape[0], y_true, V, lab, dev)
    cand, _ = ops.sample_candidates(lab, V, num_negatives, seed, row_base, exclude=ex,
                                    item_cdf=None if cdf is None else cdf.to(dev))
    return cand


def _cand_key(c):
    return None if c is None else (c.data_ptr(), c._version, tuple(c.shape), c.dtype)


def _row_candidates(candidates, n_rows, y_true, device):
    """update_state's `candidates` -> int32 (rows, C) device lists: (B*M, C) per row, or (B, C) per sequence of a (B, M) y_true"""
    c = torch.as_tensor(candidates)
    if c.dim() != 2 or c.dtype.is_floating_point or c.dtype == torch.bool:
        raise ValueError('candidates must be an integer (rows, C) or (B, C) tensor, got %s %s' % (c.dtype, tuple(c.shape)))
    if c.dtype != torch.int32:
        c = torch.where((c >= 0) & (c < (1 << 31)), c, torch.full_like(c, -1)).to(torch.int32)
    c = c.to(device)
    if c.shape[0] != n_rows:
        yt = torch.as_tensor(y_true)
        if yt.dim() != 2 or c.shape[0] != yt.shape[0]:
            raise ValueError('candidates have %d lists for %d rows' % (c.shape[0], n_rows))
        c = c.repeat_interleave(yt.shape[1], dim=0)
    return c.contiguous()


_last_rank = {'key': None, 'val': None}     # Recall@k and NDCG@k of one (y_true, y_pred) pair share one top-k pass


class _ClozeRankMetric:
    def __init__(self, k, name):
        self.k, self.name = k, name
        self.n_examples = None
        self.total = None

    def _rows(self, y_true, y_pred, exclude=None, candidates=None):
        if candidates is not None and exclude is not None:
            raise ValueError('candidates and exclude together: leave the excluded items out of the lists '
                             '(cloze.sample_candidates(..., exclude=))')
        if candidates is not None:
            return self._cand_rows(y_true, y_pred, candidates)
        if hasattr(y_pred, 'rank_of'):
            # head.ClozeScores (model(x, scores='lazy')): rank of the true item through the logits-free sweep; one sweep
            # serves every k and both metrics (the scores object caches the rank of a label tensor)
            yt = torch.as_tensor(y_true, device=y_pred.device).reshape(-1)
            key = ('lazy', id(y_pred), yt.data_ptr(), yt._version, tuple(yt.shape), _exclude_key(exclude))
            if _last_rank['key'] == key and _last_rank['ref']() is y_pred:
                lab, valid, ex = _last_rank['val']
            else:
                valid = yt != LABEL_PAD
                lab = torch.where(valid, yt, torch.full_like(yt, -1)).to(torch.int32).contiguous()
                ex = None if exclude is None else _row_exclusions(exclude, yt.shape[0], y_true, y_pred.shape[-1], lab, y_pred.device)
                _last_rank.update(key=key, val=(lab, valid, ex), ref=weakref.ref(y_pred))
            hit, ndcg = ops.rank_metrics(y_pred.rank_of(lab) if ex is None else y_pred.rank_of(lab, exclude=ex), self.k)
            if y_pred.flag is not None:
                ops.poison_rows(hit.view(-1, 1), y_pred.flag)
                ops.poison_rows(ndcg.view(-1, 1), y_pred.flag)
            return hit, ndcg, valid
        ops._cuda(y_pred)
        V = y_pred.shape[-1]
        yp = y_pred.reshape(-1, V)
        if yp.stride(1) != 1 or yp.stride(0) % 8 != 0:
            buf = torch.zeros(yp.shape[0], ops.rup8(V), dtype=yp.dtype, device=yp.device)
            buf[:, :V] = yp
            yp = buf
        yt = torch.as_tensor(y_true, device=y_pred.device).reshape(-1)
        key = (yp.data_ptr(), yp._version, tuple(yp.shape), yp.stride(0), yp.dtype, yt.data_ptr(), yt._version, tuple(yt.shape),
               self.k, torch.cuda.current_stream().cuda_stream, _exclude_key(exclude))
        if _last_rank['key'] == key and _last_rank['ref']() is y_pred:
            return _last_rank['val']
        valid = yt != LABEL_PAD
        lab = torch.where(valid, yt, torch.full_like(yt, -1)).to(torch.int32).contiguous()
        if exclude is None:
            _, hit, ndcg = ops.topk_rows(yp, V, self.k, lab)
        else:          # y_pred is only read
            _, hit, ndcg = ops.topk_rows(yp, V, self.k, lab,
                                         exclude=_row_exclusions(exclude, yp.shape[0], y_true, V, lab, yp.device))
        _last_rank.update(key=key, val=(hit, ndcg, valid), ref=weakref.ref(y_pred))     # same object, same version -> same scores
        return hit, ndcg, valid

    def _cand_rows(self, y_true, y_pred, candidates):
        """hit / ndcg of the label's rank among each row's candidate list: through the head's candidate scores (lazy y_pred,
        b4c_candidate_score) or gathered from the materialised probabilities (b4c_candidate_rank_rows); one rank serves
        Recall@k and NDCG@k of the same triple"""
        dev = y_pred.device
        yt = torch.as_tensor(y_true, device=dev).reshape(-1)
        lazy = hasattr(y_pred, 'rank_of')
        if lazy:
            yp, V = None, y_pred.shape[-1]
            pkey = ('lazy', id(y_pred))
        else:
            ops._cuda(y_pred)
            V = y_pred.shape[-1]
            yp = y_pred.reshape(-1, V)
            if yp.stride(1) != 1:
                yp = yp.contiguous()
            pkey = (yp.data_ptr(), yp._version, tuple(yp.shape), yp.stride(0), yp.dtype)
        ckey = _cand_key(candidates) if isinstance(candidates, torch.Tensor) else ('host', id(candidates))
        key = ('cand',) + pkey + (yt.data_ptr(), yt._version, tuple(yt.shape), ckey, torch.cuda.current_stream().cuda_stream)
        if _last_rank['key'] == key and _last_rank['ref']() is y_pred:
            rank, valid = _last_rank['val'][:2]
        else:
            lab, valid = _labels_i32(yt, dev)
            cand = _row_candidates(candidates, yt.shape[0], y_true, dev)
            if lazy:
                rank = y_pred.rank_of(lab, candidates=cand)
            else:          # y_pred is only read
                rank, _ = ops.candidate_rank_rows(yp, V, cand, lab)
            # the key names the lists and labels by address (or id()): the entry holds them, so that no later list or label
            # tensor can take the same address while the entry stands and be answered with this rank
            _last_rank.update(key=key, val=(rank, valid, candidates, y_true, yt), ref=weakref.ref(y_pred))
        hit, ndcg = ops.rank_metrics(rank, self.k)
        if lazy and y_pred.flag is not None:
            ops.poison_rows(hit.view(-1, 1), y_pred.flag)
            ops.poison_rows(ndcg.view(-1, 1), y_pred.flag)
        return hit, ndcg, valid

    def _add(self, value, n):
        if self.total is None:
            self.total, self.n_examples = value.clone(), n.clone()
        else:
            self.total += value
            self.n_examples += n

    def result(self):
        return self.total / self.n_examples

    def reset_states(self):
        self.total = self.n_examples = None

    def all_reduce(self, group=None):
        """Data-parallel evaluation: accumulators are sums, one tiny all-reduce merges the ranks."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and self.total is not None:
            buf = torch.stack([self.total, self.n_examples])
            dist.all_reduce(buf, group=group)
            self.total, self.n_examples = buf[0], buf[1]


class ClozeMaskedRecall(_ClozeRankMetric):
    """HitRate@k: was the true item among the top k of V (utils.py:137-194)."""

    def __init__(self, k, name=None):
        super().__init__(k, name or 'Recall_at_%d' % k)

    def update_state(self, y_true, y_pred, sample_weight=None, exclude=None, candidates=None):
        """exclude: items left out of each row's ranking (cloze.seen_items for the filtered protocol): (B, E) per sequence
        or (B*M, E) per row, integer ids padded with negatives, or host lists; the label is never excluded.
        candidates: rank among a list of items per row instead of all V (cloze.sample_candidates: the sampled-negative
        protocol): (B*M, C) per row or (B, C) per sequence, label-space ids, < 0 absent; not together with exclude"""
        hit, _, valid = self._rows(y_true, y_pred, exclude, candidates)
        self._add((hit * valid).sum(), valid.sum().to(torch.float32))


class ClozeMaskedNDCG(_ClozeRankMetric):
    """NDCG@k with a single relevant item: 1/log2(rank+1) if ranked within k else 0 (utils.py:197-259)."""

    def __init__(self, k, name=None):
        super().__init__(k, name or 'NDCG_at_%d' % k)

    def update_state(self, y_true, y_pred, sample_weight=None, exclude=None, candidates=None):
        """exclude: items left out of each row's ranking (cloze.seen_items for the filtered protocol): (B, E) per sequence
        or (B*M, E) per row, integer ids padded with negatives, or host lists; the label is never excluded.
        candidates: rank among a list of items per row instead of all V (cloze.sample_candidates: the sampled-negative
        protocol): (B*M, C) per row or (B, C) per sequence, label-space ids, < 0 absent; not together with exclude"""
        _, ndcg, valid = self._rows(y_true, y_pred, exclude, candidates)
        self._add((ndcg * valid).sum(), valid.sum().to(torch.float32))
