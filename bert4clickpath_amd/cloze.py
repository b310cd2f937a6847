"""Cloze (masked-item) loss and ranking metrics of the BERT4Rec example
(reference examples/BERT4Rec/source/utils.py:56-259), over the HIP kernels.

y_true: (B, M) labels padded with -1;  y_pred: (B, M, V) probabilities (or any monotone score for
the metrics).  All accumulators live on the device; ``result()`` returns a 0-d tensor."""
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


_last_rank = {'key': None, 'val': None}     # Recall@k and NDCG@k of one (y_true, y_pred) pair share one top-k pass


class _ClozeRankMetric:
    def __init__(self, k, name):
        self.k, self.name = k, name
        self.n_examples = None
        self.total = None

    def _rows(self, y_true, y_pred, exclude=None):
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

    def update_state(self, y_true, y_pred, sample_weight=None, exclude=None):
        """exclude: items left out of each row's ranking (cloze.seen_items for the filtered protocol): (B, E) per sequence
        or (B*M, E) per row, integer ids padded with negatives, or host lists; the label is never excluded"""
        hit, _, valid = self._rows(y_true, y_pred, exclude)
        self._add((hit * valid).sum(), valid.sum().to(torch.float32))


class ClozeMaskedNDCG(_ClozeRankMetric):
    """NDCG@k with a single relevant item: 1/log2(rank+1) if ranked within k else 0 (utils.py:197-259)."""

    def __init__(self, k, name=None):
        super().__init__(k, name or 'NDCG_at_%d' % k)

    def update_state(self, y_true, y_pred, sample_weight=None, exclude=None):
        """exclude: items left out of each row's ranking (cloze.seen_items for the filtered protocol): (B, E) per sequence
        or (B*M, E) per row, integer ids padded with negatives, or host lists; the label is never excluded"""
        _, ndcg, valid = self._rows(y_true, y_pred, exclude)
        self._add((ndcg * valid).sum(), valid.sum().to(torch.float32))
