#!/usr/bin/env python3
"""Amazon-Beauty BERT4Rec on the MI355X hot path: the reference example's configuration
(examples/BERT4Rec/source/main.py: d_model 64, 2 layers, 2 heads, dff 100, head [1024,512,256,128] -> V,
Adam 1e-3/.9/.999/1e-9, dropout 0.1, 512 sequences per step), trained for a bounded number of steps, then
HitRate@10 / NDCG@10 with the reference's evaluation protocol (mask the last item, rank over ALL V items).
--negatives N adds the BERT4Rec paper's protocol beside it: the held-out item ranked against N sampled items the user has not
seen (uniform, or by popularity counted on the training split), HR@10 / NDCG@10 over those 1 + N candidates.
--paper_model builds the paper's MODEL instead of the reference's (no reference oracle): learned positions, GELU feed-forward of width
4 d, drop(LayerNorm(E + P)) at the input, attention dropout, the tied head LayerNorm(gelu(Dense(d -> d))) . E^T + b; with the paper's
recipe (--clipnorm 5 --warmup 100 --weight_decay 0.01) and --negatives 100 its sampled-negative numbers stand beside the published ones.
--device_batches with --max_len / --stride / --holdout / --last_item_rate is the paper's DATA protocol: sliding training windows, the
penultimate item held out for validation and the last for test (both reported), last-item training rows; the filtered and the
sampled-negative figures then exclude a user's whole history (DeviceCloze.history), not only the row's window.
--device_batches --popularity_buckets K trains a TWO-feature model: beside the item, the bucket (of K, equally filled by rank) of its
count in the training split -- a feature of the item, so it is [MASK] wherever the item is (DeviceCloze(features=), Feature(per='item')).

    python examples/beauty_hitrate.py --steps 3000 --dtype f32
Prints one JSON line.  The CPU counterpart on the oracle is oracle/train_beauty_cpu.py (same seeds, batches,
initial weights and dropout masks)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


POPULARITY = 'popularity'         # the side feature of --popularity_buckets: its name in the batches and in the model's inputs


def popularity_buckets(counts, K):
    """int32 [V]: the bucket 0 .. K - 1 of every item, the items ranked by their count (most frequent first, ties by index) and
    cut into K runs of equal length"""
    order = np.argsort(-np.asarray(counts, dtype=np.int64), kind='stable')
    bucket = np.empty(len(order), dtype=np.int32)
    bucket[order] = (np.arange(len(order), dtype=np.int64) * K // max(len(order), 1)).astype(np.int32)
    return bucket


def build_model(V, dropout, dtype, seed=1234, paper_positions=None, attention='bidirectional', tied_head=False, buckets=0, norm='post'):
    """paper_positions (the longest encoder input): the BERT4Rec paper's model, one constructor call.
    buckets K > 0: a second embedded feature of K values, summed with the item's embedding (the width stays 64).
    attention='causal': left-to-right self-attention (SASRec, the paper's unidirectional arm).
    norm='pre': pre-LN encoder blocks and a final LayerNorm (the common SASRec re-implementations; the reference's blocks are post-LN).
    tied_head: score an item by the dot product of the encoder output with its embedding (SASRec's head), in place of the reference's
    dense stack -- the sampled-negative losses (--train_loss bce / softmax / bpr / gbce) need a projection stored per item."""
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, ClozeMaskedItemPrediction, SoftMaxHead
    torch.manual_seed(seed)            # CPU generator: identical initial weights on any machine
    vocab = ['item%d' % i for i in range(V)]
    kw = {'attention': attention} if attention != 'bidirectional' else {}
    if norm != 'post':
        kw['norm'] = norm
    if paper_positions is not None:
        return ClickstreamTransformer({'items': ['asin']}, {'items': vocab}, {'items': 64},
                                      ClozeMaskedItemPrediction([], V, transform='gelu_tanh'), value_to_head='[MASK]',
                                      num_encoder_layers=2, num_attention_heads=2, encoder_ff_dim=256, dropout_rate=dropout,
                                      attention_dropout_rate=dropout, compute_dtype=dtype, ffn_activation='gelu_tanh',
                                      position_encoding='learned', max_positions=paper_positions, embedding_layernorm=True,
                                      embedding_scale=1.0, **kw)
    head = ClozeMaskedItemPrediction([], V) if tied_head else SoftMaxHead([1024, 512, 256, 128], V)
    chains, vocabs, dims = {'items': ['asin']}, {'items': vocab}, {'items': 64}
    if buckets:
        chains['buckets'], vocabs['buckets'], dims['buckets'] = [POPULARITY], ['bucket%d' % i for i in range(buckets)], 64
        kw['feature_combine'] = 'sum'
    return ClickstreamTransformer(chains, vocabs, dims, head, value_to_head='[MASK]',
                                  num_encoder_layers=2, num_attention_heads=2, dropout_rate=dropout, compute_dtype=dtype, **kw)


def add_train_loss_arguments(ap):
    ap.add_argument('--train_loss', default='full', choices=['full', 'bce', 'softmax', 'bpr', 'gbce'],
                    help='full: the softmax over all V items (cloze_loss); bce / softmax / bpr / gbce: each target against '
                         '--train_negatives sampled items that its sequence does not hold (model.candidate_loss) -- binary '
                         'cross-entropy per item (SASRec), the list-wise softmax, the pairwise BPR loss, or gSASRec\'s generalised BCE '
                         '(--gbce_t); the head is then the tied dot product with the item embedding.  SASRec\'s recipe: '
                         '--device_batches --attention causal --objective next_item --train_loss bce --train_negatives 1')
    ap.add_argument('--train_negatives', type=int, default=1, help='with a sampled --train_loss: negatives drawn per target')
    ap.add_argument('--gbce_t', type=float, default=0.75,
                    help='with --train_loss gbce: the calibration parameter t in [0, 1] (0: plain bce; gSASRec uses 0.75 with 256 negatives)')
    ap.add_argument('--logq', action='store_true',
                    help='with a sampled --train_loss and --device_batches: draw the training negatives by popularity (the item counts of '
                         'the training views) and subtract the matching log expected count from every negative\'s score -- the '
                         'sampled-softmax logQ correction (cloze.log_expected_count)')


def add_objective_argument(ap):
    ap.add_argument('--objective', default='cloze', choices=['cloze', 'next_item'],
                    help='cloze: masked positions predict their own item; next_item (needs --device_batches, meant for --attention '
                         'causal): every real position of an unmasked row predicts the item after it, with --train_loss bce / softmax '
                         'against --train_negatives items the user never touched (DeviceCloze.next_item_batches, model.next_item_loss); '
                         'evaluation rows end at the item in front of the target: no [MASK] in training or in evaluation')


def add_contrastive_arguments(ap):
    ap.add_argument('--contrastive_weight', type=float, default=0.0, metavar='LAM',
                    help='LAM > 0 adds LAM * model.contrastive_loss to the training loss: in-batch InfoNCE between two dropout views of '
                         'every sequence of the batch, read at its last item (the auxiliary loss of DuoRec / CL4SRec; needs --dropout > '
                         '0; two more encoder passes per step).  With every objective and --train_loss')
    ap.add_argument('--contrastive_views', default='dropout', metavar='dropout|crop,mask,reorder|same_target',
                    help="with --contrastive_weight: where the two views come from.  'dropout' (default): two dropout passes over the "
                         "batch's inputs (needs --dropout > 0).  A comma list of crop, mask, reorder (CL4SRec): two augmented views of "
                         "every row, one operator drawn per row and view.  'same_target' (DuoRec, --objective next_item): the batch's "
                         "inputs against the inputs in front of another occurrence of each row's target item, rows with the same target "
                         "not each other's negatives.  The last two are built on the device (DeviceCloze.views: --device_batches), "
                         "encoded padding-free, and work at --dropout 0")
    ap.add_argument('--contrastive_temperature', type=float, default=1.0, help='with --contrastive_weight: the temperature')
    ap.add_argument('--contrastive_sim', default='dot', choices=['dot', 'cos'], help='with --contrastive_weight: dot product or cosine')
    ap.add_argument('--contrastive_same_target', action='store_true',
                    help='with --contrastive_weight: two sequences with the same (last) target item are not each other\'s negatives (DuoRec)')


def check_contrastive_arguments(ap, a):
    if a.contrastive_weight < 0 or a.contrastive_temperature <= 0:
        ap.error('--contrastive_weight must be >= 0 and --contrastive_temperature > 0')
    a.contrastive_ops = None if a.contrastive_views == 'dropout' else tuple(a.contrastive_views.split(','))
    if a.contrastive_ops is None:
        if a.contrastive_weight > 0 and a.dropout <= 0:
            ap.error('--contrastive_weight takes its two views from dropout: it needs --dropout > 0 (or --contrastive_views crop,mask,reorder)')
        return
    if a.contrastive_ops != ('same_target',) and not set(a.contrastive_ops) <= {'crop', 'mask', 'reorder'}:
        ap.error("--contrastive_views: 'dropout', 'same_target', or a comma list of crop, mask, reorder")
    if not getattr(a, 'device_batches', False) and getattr(a, 'objective', 'cloze') != 'next_item':
        ap.error('--contrastive_views %s builds its views on the device: it needs --device_batches' % a.contrastive_views)
    if a.contrastive_ops == ('same_target',) and getattr(a, 'objective', 'cloze') != 'next_item':
        ap.error('--contrastive_views same_target needs --objective next_item (a Cloze row has no target)')


def last_targets(labels_padded=None, labels=None, row_offsets=None):
    """the last target of every sequence of a batch, on the device (-1: none): of the padded (B, M) Cloze labels, or of the compact
    labels of a next-item batch and their per-sequence offsets"""
    if labels_padded is not None:
        lab = labels_padded.to(torch.int64)
        n = (lab >= 0).sum(1)
        return torch.where(n > 0, lab.gather(1, (n - 1).clamp(min=0)[:, None])[:, 0], torch.full_like(n, -1))
    off = row_offsets.long()
    if labels.numel() == 0:
        return torch.full((off.shape[0] - 1,), -1, dtype=torch.int64, device=off.device)
    return torch.where(off[1:] > off[:-1], labels.long()[(off[1:] - 1).clamp(min=0, max=labels.shape[0] - 1)], torch.full_like(off[1:], -1))


def contrastive_term(model, a, inputs, same_target=None, dev_data=None, batch=None, view_seed=0, **kw):
    """--contrastive_weight times the in-batch contrastive loss of two views of the batch (0.0 without the option): two dropout
    passes over `inputs`, or (--contrastive_views) views of `batch` that dev_data builds on the device"""
    if a.contrastive_weight <= 0:
        return 0.0
    if a.contrastive_ops == ('same_target',):        # DuoRec's supervised positive beside the batch's own inputs
        (view,) = dev_data.views(batch, view_seed, ops='same_target', n_views=1)
        return a.contrastive_weight * model.contrastive_loss(inputs, dev_data.inputs(view, 'asin'), temperature=a.contrastive_temperature,
                                                             similarity=a.contrastive_sim, same_target=view['target'],
                                                             n_real_tokens_b=view['n_real_tokens'], **kw)
    if a.contrastive_ops is not None:                # CL4SRec: two augmented views
        one, two = dev_data.views(batch, view_seed, ops=a.contrastive_ops, n_views=2)
        return a.contrastive_weight * model.contrastive_loss(dev_data.inputs(one, 'asin'), dev_data.inputs(two, 'asin'),
                                                             temperature=a.contrastive_temperature, similarity=a.contrastive_sim,
                                                             same_target=same_target if a.contrastive_same_target else None,
                                                             n_real_tokens=one['n_real_tokens'], n_real_tokens_b=two['n_real_tokens'])
    return a.contrastive_weight * model.contrastive_loss(inputs, temperature=a.contrastive_temperature, similarity=a.contrastive_sim,
                                                         same_target=same_target if a.contrastive_same_target else None, **kw)


def check_train_loss_arguments(ap, a):
    if a.logq and (a.train_loss == 'full' or not a.device_batches):
        ap.error('--logq corrects sampled negatives drawn from the device data set\'s counts: it needs --device_batches and a '
                 '--train_loss other than full')
    if not 0.0 <= a.gbce_t <= 1.0:
        ap.error('--gbce_t must be in [0, 1]')


def train_sampling(dev_data, a):
    """how the training negatives are drawn and corrected -> dict(item_cdf=, logq=): both None (uniform, no correction) without
    --logq; with it the prefix sum of the training views' item counts, which the sampler draws by, and the log expected count of every
    item among the --train_negatives negatives of a list, on the device"""
    if not a.logq:
        return dict(item_cdf=None, logq=None)
    from bert4clickpath_amd import cloze
    counts = dev_data.item_counts('train')
    return dict(item_cdf=torch.from_numpy(np.cumsum(counts)).cuda(),
                logq=cloze.log_expected_count(counts, num_negatives=a.train_negatives, device='cuda'))


def next_item_train_batches(dev_data, a, steps, item_cdf=None):
    """the --objective next_item training batches: negatives only where --train_loss reads them (item_cdf: drawn by popularity)"""
    return dev_data.next_item_batches(a.batch, a.seed, steps, num_negatives=0 if a.train_loss == 'full' else a.train_negatives,
                                      item_cdf=item_cdf)


def next_item_training_loss(model, a, batch, logq=None):
    """model.next_item_loss with what --train_loss, --gbce_t and --logq select"""
    if a.train_loss == 'full':
        return model.next_item_loss(batch, loss='full')
    return model.next_item_loss(batch, loss=a.train_loss, gbce_t=a.gbce_t, logq=logq)


def training_loss(model, a, feats, labels, item_cdf=None, logq=None, **kw):
    """the loss --train_loss selects; item_cdf, logq: train_sampling's; kw: cloze_loss's flat_idx / max_masked_per_row /
    n_real_tokens"""
    if a.train_loss == 'full':
        return model.cloze_loss(feats, labels, training=True, **kw)
    from bert4clickpath_amd import cloze
    seen = cloze.seen_items(feats['asin'])                   # (B, S): a sequence's own items are never its negatives
    if kw.get('flat_idx') is not None:                       # rows are named by position: one exclusion list per row
        seen = seen[(kw['flat_idx'].long() // (feats['asin'].shape[1] + 3))]       # [CLS] [SEP] items [SEP]
    return model.candidate_loss(feats, labels, num_negatives=a.train_negatives, loss=a.train_loss, exclude=seen, training=True,
                                item_cdf=item_cdf, gbce_t=a.gbce_t, logq=logq, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3000)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
    ap.add_argument('--dropout', type=float, default=0.1)
    ap.add_argument('--seed', type=int, default=4321)
    ap.add_argument('--eval_limit', type=int, default=None)
    ap.add_argument('--data', default=os.path.join(ROOT, 'data', 'beauty_sequences.npz'))
    ap.add_argument('--exclude_seen', action='store_true',
                    help='also report the filtered protocol: the held-out item ranked against the items absent from the history')
    ap.add_argument('--negatives', type=int, default=0,
                    help='also report the sampled-negative protocol of the BERT4Rec paper: the held-out item against N '
                         'sampled unseen items (100 in the paper)')
    ap.add_argument('--sampler', default='popularity', choices=['uniform', 'popularity'],
                    help='how the negatives are drawn; popularity counts come from the training split only')
    ap.add_argument('--clipnorm', type=float, default=None,
                    help='clip the gradient by its global L2 norm (the BERT4Rec paper uses 5.0); default: no clipping')
    ap.add_argument('--warmup', type=int, default=0,
                    help='linear warm-up of the learning rate over this many steps, then linear decay to 0 at --steps (the '
                         'paper\'s shape, training_utils.WarmupLinearDecay); default 0: the constant 1e-3 of the reference')
    ap.add_argument('--weight_decay', type=float, default=None,
                    help='decoupled weight decay (AdamW; the paper uses 0.01) on every weight matrix and embedding table, not on '
                         'biases and LayerNorm vectors (optim.no_decay_params); default: none.  The paper\'s recipe in full: '
                         '--clipnorm 5 --warmup 100 --weight_decay 0.01')
    ap.add_argument('--paper_model', action='store_true',
                    help='the BERT4Rec paper\'s model (learned positions, GELU, normalised input stage, attention dropout, tied head '
                         'with its transform) instead of the reference\'s; a measurement, no reference oracle')
    ap.add_argument('--device_batches', action='store_true',
                    help='build the training and evaluation batches on the device (cloze_batches.DeviceCloze): no per-row host '
                         'work and no upload per step; the masks are that kernel\'s own stream, so losses differ from the default')
    ap.add_argument('--max_len', type=int, default=None,
                    help='with --device_batches: rows of at most this many items -- long training sequences are cut into sliding '
                         'windows, evaluation keeps the most recent ones (the paper\'s protocol); default: whole sequences')
    ap.add_argument('--stride', type=int, default=None, help='with --max_len: the step between two training windows; default: max_len')
    ap.add_argument('--holdout', type=int, default=1, choices=[1, 2],
                    help='with --device_batches: 2 holds out the penultimate item for validation and the last for test (the '
                         'paper\'s leave-one-out split; both are reported); default 1: the last item is the test target')
    ap.add_argument('--last_item_rate', type=float, default=0.0,
                    help='with --device_batches: the share of training rows whose only masked position is the last one')
    ap.add_argument('--attention', default='bidirectional', choices=['bidirectional', 'causal'],
                    help='causal: left-to-right self-attention inside the kernels; with --device_batches --last_item_rate 1.0 a '
                         'left-to-right next-item model (every training row predicts the item after its prefix)')
    ap.add_argument('--norm', default='post', choices=['post', 'pre'],
                    help='pre: pre-LN encoder blocks, x + drop(sublayer(LayerNorm(x))), and one LayerNorm behind the last layer (q, k and v '
                         'all from the normalised rows; the full last layer always runs); post: the reference\'s blocks')
    ap.add_argument('--mq_causal', action='store_true',
                    help='with --attention causal: evaluate the last encoder layer at the rows the head reads only (ops.mq_causal, off '
                         'by default; with attention dropout in training also B4C_MQ_ATTN_DROPOUT=1); the next-item evaluation names '
                         'its rows and passes row_offsets= either way')
    ap.add_argument('--popularity_buckets', type=int, default=0,
                    help='with --device_batches: K > 0 adds a second feature to the model and to every batch -- the bucket, of K, of '
                         'the item\'s count in the training split (masked with the item); default 0: the one-feature model')
    add_train_loss_arguments(ap)
    add_objective_argument(ap)
    add_contrastive_arguments(ap)
    a = ap.parse_args()
    check_contrastive_arguments(ap, a)
    if a.popularity_buckets and (not a.device_batches or a.paper_model or a.popularity_buckets < 0):
        ap.error('--popularity_buckets K > 0 needs --device_batches and the reference\'s model (no --paper_model)')
    if a.objective == 'next_item' and not a.device_batches:
        ap.error('--objective next_item needs --device_batches')
    check_train_loss_arguments(ap, a)
    protocol = dict(max_len=a.max_len, stride=a.stride, holdout=a.holdout, last_item_rate=a.last_item_rate)
    if not a.device_batches and protocol != dict(max_len=None, stride=None, holdout=1, last_item_rate=0.0):
        ap.error('--max_len, --stride, --holdout and --last_item_rate need --device_batches')
    from bert4clickpath_amd import input_pipeline, ops, optim
    from bert4clickpath_amd.clickstream_transformer.training_utils import WarmupLinearDecay
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    data = input_pipeline.BeautyCloze(a.data)
    if a.mq_causal:
        ops.mq_causal = True
    dtype = torch.float32 if a.dtype == 'f32' else torch.bfloat16
    longest = (int(np.diff(data.offsets).max()) if a.max_len is None else a.max_len) + 3       # [CLS] [SEP] items [SEP]
    model = build_model(data.V, a.dropout, dtype, paper_positions=longest if a.paper_model else None, attention=a.attention,
                        tied_head=a.train_loss != 'full', buckets=a.popularity_buckets, norm=a.norm).cuda()
    lr = WarmupLinearDecay(1e-3, a.warmup, max(a.steps, a.warmup + 1)) if a.warmup > 0 else 1e-3
    opt = optim.Adam(model.parameters(), learning_rate=lr, global_clipnorm=a.clipnorm, weight_decay=a.weight_decay,
                     exclude_from_weight_decay=optim.no_decay_params(model) if a.weight_decay is not None else ())
    T.set_dropout_seed(a.seed)
    t0, losses = time.perf_counter(), []
    dev_data = None
    if a.device_batches:
        from bert4clickpath_amd.cloze_batches import DeviceCloze, Feature
        if a.popularity_buckets:        # counted on the training views of the same protocol, on the host
            counts = DeviceCloze.from_npz(a.data, device=None, **protocol).item_counts('train')
            protocol_kw = dict(protocol, features={POPULARITY: Feature(popularity_buckets(counts, a.popularity_buckets),
                                                                       a.popularity_buckets, per='item', on_mask='mask')})
        else:
            protocol_kw = protocol
        dev_data = DeviceCloze.from_npz(a.data, **protocol_kw)
    next_item = a.objective == 'next_item'
    sampling = train_sampling(dev_data, a)
    per_epoch = max(dev_data.n_windows // a.batch, 1) if dev_data is not None else 1
    for step, b in enumerate(next_item_train_batches(dev_data, a, a.steps, sampling['item_cdf']) if next_item
                             else (dev_data or data).train_batches(a.batch, a.seed, a.steps)):
        opt.zero_grad()
        views = {}
        if a.contrastive_weight > 0 and a.contrastive_ops is not None:      # the views' seed of the epoch, as the builders' own
            views = dict(dev_data=dev_data, batch=b, view_seed=int(ops.rand64_host(a.seed, step // per_epoch)))
        if next_item:                 # unmasked rows, every position's target and its negatives: all built on the device
            loss = next_item_training_loss(model, a, b, sampling['logq'])
            if a.contrastive_weight > 0:
                loss = loss + contrastive_term(model, a, model._next_item_inputs(b), last_targets(labels=b['labels'], row_offsets=b['row_offsets']),
                                               n_real_tokens=b['n_real_tokens'], **views)
        elif dev_data is not None:      # items and padded labels are on the device already; nothing is read back
            loss = training_loss(model, a, dev_data.inputs(b, 'asin'), b['labels_padded'], **sampling,
                                 max_masked_per_row=b['labels_padded'].shape[1], n_real_tokens=b['n_real_tokens'])
            if a.contrastive_weight > 0:
                loss = loss + contrastive_term(model, a, dev_data.inputs(b, 'asin'), last_targets(labels_padded=b['labels_padded']),
                                               n_real_tokens=b['n_real_tokens'], **views)
        else:
            ids = torch.from_numpy(b['ids'])
            items = ids[:, 2:-1].contiguous().cuda()
            loss = training_loss(model, a, {'asin': items}, torch.from_numpy(b['labels']).cuda(),
                                 flat_idx=torch.from_numpy(b['flat_idx']).cuda())
            if a.contrastive_weight > 0:
                loss = loss + contrastive_term(model, a, {'asin': items}, last_targets(labels_padded=torch.from_numpy(b['labels_padded']).cuda()))
        loss.backward()
        opt.step()
        if step % 100 == 0 or step == a.steps - 1:
            losses.append((step, float(loss.detach())))
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    from bert4clickpath_amd import cloze
    from bert4clickpath_amd.clickstream_transformer.constants import NUM_RESERVED_TOKENS
    counts = None
    if a.negatives and a.sampler == 'popularity':       # the training split: every sequence without its held-out items
        if dev_data is not None:
            counts = dev_data.item_counts('train')
        else:
            train = np.concatenate([data.seq(i)[:-1] for i in range(data.n_seq)]) + NUM_RESERVED_TOKENS
            counts = cloze.item_counts(train, data.V)

    def evaluate(split):
        """the metrics of one split ('test': the last item; 'valid', with --holdout 2: the penultimate one)"""
        hits = ndcg = n = fhits = fndcg = shits = sndcg = 0.0
        for b in (dev_data.next_item_eval_batches(1024, a.eval_limit, split=split) if next_item else
                  dev_data.eval_batches(1024, a.eval_limit, split=split) if dev_data is not None else data.eval_batches(1024, a.eval_limit)):
            seen, side = None, {}
            if next_item:                 # one compact row per sequence that has a target, at its last input; the row holds no [MASK]
                items, labels, flat, side = b['items'], b['labels'], b['flat_idx'], b.get('features', {})
                if a.exclude_seen or a.negatives:
                    seen = dev_data.history(b['target_seq_idx'], split=split)
            elif dev_data is not None:      # at most one [MASK] per row; a sequence too short for the target has none
                real = b['n_masked'] == 1
                items, labels, flat = b['items'][real], b['labels_padded'][real].reshape(-1).to(torch.int32), None
                side = {k: v[real] for k, v in b.get('features', {}).items()}
                if a.max_len is not None and (a.exclude_seen or a.negatives):      # a window does not hold the older items
                    seen = dev_data.history(b['seq_idx'], split=split)[real]
            else:
                ids = torch.from_numpy(b['ids'])
                items = ids[:, 2:-1].contiguous().cuda()
                labels, flat = torch.from_numpy(b['labels']).cuda(), torch.from_numpy(b['flat_idx']).cuda()
            if seen is None and (a.exclude_seen or a.negatives):
                seen = cloze.seen_items(items)
            # (row_offsets: the last layer runs at the named rows only where that route is open -- a bidirectional model, a causal one
            # with --mq_causal)
            kw = {'n_real_tokens': b['n_real_tokens'], 'row_offsets': b['row_offsets']} if next_item else {}
            feats = {'asin': items, **side}
            _, h, nd = model.predict_topk(feats, 10, labels, flat_idx=flat, **kw)
            hits += float(h.sum()); ndcg += float(nd.sum()); n += h.numel()
            if a.exclude_seen:          # one [MASK] (the target) per sequence: the rows are the sequences, in order
                _, h, nd = model.predict_topk(feats, 10, labels, flat_idx=flat, exclude=seen, **kw)
                fhits += float(h.sum()); fndcg += float(nd.sum())
            if a.negatives:             # row_base: the draws of a row do not depend on the batch size
                cand = cloze.sample_candidates(labels, a.negatives, exclude=seen, item_counts=counts, seed=a.seed,
                                               row_base=int(n) - labels.numel(), num_items=data.V)
                _, h, nd = model.predict_topk(feats, 10, labels, flat_idx=flat, candidates=cand, **kw)
                shits += float(h.sum()); sndcg += float(nd.sum())
        res = {'hitrate@10': 100.0 * hits / n, 'ndcg@10': 100.0 * ndcg / n, 'n_eval': int(n)}
        if a.exclude_seen:
            res.update({'filtered_hitrate@10': 100.0 * fhits / n, 'filtered_ndcg@10': 100.0 * fndcg / n})
        if a.negatives:
            res.update({'sampled_hitrate@10': 100.0 * shits / n, 'sampled_ndcg@10': 100.0 * sndcg / n})
        return res

    out = {'what': 'Amazon Beauty, HIP path' + (', the BERT4Rec paper\'s model' if a.paper_model else ''), 'dtype': a.dtype, 'steps': a.steps, 'batch': a.batch,
           'dropout': a.dropout}
    out.update(evaluate('test'))
    out.update({'train_seconds': train_s, 'loss_curve': losses, 'device_batches': bool(a.device_batches)})
    if a.negatives:
        out['sampled_protocol'] = ('BERT4Rec paper: 1 held-out + %d %s-sampled unseen items (not the reference\'s full ranking)'
                                   % (a.negatives, a.sampler))
    if a.device_batches:
        out['data_protocol'] = protocol
        out['objective'] = a.objective
        out['popularity_buckets'] = a.popularity_buckets
    if a.contrastive_weight > 0:
        out['contrastive'] = dict(weight=a.contrastive_weight, views=a.contrastive_views, temperature=a.contrastive_temperature, similarity=a.contrastive_sim,
                                  same_target=a.contrastive_same_target)
    if a.holdout == 2:               # the split a model is selected on; the test numbers above are read once, at the end
        out['valid'] = evaluate('valid')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
