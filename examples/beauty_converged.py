#!/usr/bin/env python3
"""Amazon-Beauty BERT4Rec trained TO CONVERGENCE with the reference's loop controls (examples/BERT4Rec/source/main.py):
epochs of `steps_per_epoch` = 1000 steps at 512 sequences (main.py:186-188, 196), validation after every epoch on the
EVAL-mode data (mask the last item of the full sequence, input_pipeline.py:115-120; main.py:20-41), monitored value =
val_loss; ReduceLROnPlateau(val_loss, patience 10, factor 0.317) (main.py:134), EarlyStopping(val_loss, patience 30)
(main.py:156), ModelCheckpoint(save_best_only) (main.py:137-142).  Model: d_model 64, 2 layers, 2 heads, dff 100, head
[1024,512,256,128] -> V, dropout 0.1, Adam(1e-3, .9, .999, 1e-9) (main.py:87, 207-211, 236, 262-263).

Reports HitRate@10 / NDCG@10 (rank over all V items) of the final weights and of the best-val_loss checkpoint, plus the
per-epoch curve, as one JSON line.  --max_seconds bounds the wall time (the run then reports stopped_by = "time").
With --device_batches, --max_len / --stride / --holdout / --last_item_rate select the BERT4Rec paper's data protocol
(cloze_batches.DeviceCloze); with --holdout 2 the callbacks monitor the validation split (the penultimate item) and the test split
(the last item) is read once at the end, full-ranking and filtered by the user's whole history.

    python examples/beauty_converged.py --seed 1 --dtype f32 --max_seconds 1000
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from examples.beauty_hitrate import (add_objective_argument, add_train_loss_arguments, build_model, check_train_loss_arguments,  # noqa: E402
                                     next_item_train_batches, next_item_training_loss, train_sampling, training_loss)


def evaluate(model, data, batch=1024, split='test', filtered=False, next_item=False):
    """-> (val_loss, HitRate@10 %, NDCG@10 %) on every user: mask the split's target, rank over all V items; filtered: the
    ranking leaves out the user's history (DeviceCloze.history: a row's window does not hold the older items).
    data: input_pipeline.BeautyCloze (host batches) or cloze_batches.DeviceCloze (batches built on the device).
    next_item: the rows end at the item in front of the target and hold no [MASK] (DeviceCloze.next_item_eval_batches)."""
    tot = hits = ndcg = n = 0.0
    with torch.no_grad():
        for b in (data.next_item_eval_batches(batch, split=split) if next_item else
                  data.eval_batches(batch, split=split) if hasattr(data, 'history') else data.eval_batches(batch)):
            seen, kw = None, {}
            if next_item:              # one compact row per sequence that has a target, at its last input
                items, lab, flat = b['items'], b['labels'], b['flat_idx']
                kw = {'row_offsets': b['row_offsets']}     # the last layer at the named rows only, where that route is open
                if filtered:
                    seen = data.history(b['target_seq_idx'], split=split)
            elif 'items' in b:           # DeviceCloze: at most one [MASK] per row; a sequence too short for the target has none
                real = b['n_masked'] == 1
                items, lab, flat = b['items'][real], b['labels_padded'][real].reshape(-1).to(torch.int32), None
                if filtered:
                    seen = data.history(b['seq_idx'], split=split)[real]
            else:
                items = torch.from_numpy(b['ids'])[:, 2:-1].contiguous().cuda()
                lab = torch.from_numpy(b['labels']).cuda()
                flat = torch.from_numpy(b['flat_idx']).cuda()
            loss = model.cloze_loss({'asin': items}, lab, training=False, flat_idx=flat)
            _, h, nd = model.predict_topk({'asin': items}, 10, lab, flat_idx=flat, exclude=seen, **kw)
            tot += float(loss) * h.numel()
            hits += float(h.sum()); ndcg += float(nd.sum()); n += h.numel()
    return tot / n, 100.0 * hits / n, 100.0 * ndcg / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--steps_per_epoch', type=int, default=1000)
    ap.add_argument('--max_epochs', type=int, default=10000)
    ap.add_argument('--max_seconds', type=float, default=1000.0)
    ap.add_argument('--dropout', type=float, default=0.1)
    ap.add_argument('--log', default=None, help='progress file (one line per epoch)')
    ap.add_argument('--data', default=os.path.join(ROOT, 'data', 'beauty_sequences.npz'))
    ap.add_argument('--device_batches', action='store_true',
                    help='build the training and validation batches on the device (cloze_batches.DeviceCloze); the masks are that '
                         'kernel\'s own stream')
    ap.add_argument('--max_len', type=int, default=None,
                    help='with --device_batches: rows of at most this many items -- long training sequences are cut into sliding '
                         'windows, evaluation keeps the most recent ones (the BERT4Rec paper\'s protocol); default: whole sequences')
    ap.add_argument('--stride', type=int, default=None, help='with --max_len: the step between two training windows; default: max_len')
    ap.add_argument('--holdout', type=int, default=1, choices=[1, 2],
                    help='with --device_batches: 2 holds out the penultimate item for validation -- the callbacks monitor it -- and '
                         'the last for test, reported once at the end; default 1: the callbacks monitor the last item')
    ap.add_argument('--last_item_rate', type=float, default=0.0,
                    help='with --device_batches: the share of training rows whose only masked position is the last one')
    ap.add_argument('--attention', default='bidirectional', choices=['bidirectional', 'causal'],
                    help='causal: left-to-right self-attention inside the kernels; with --device_batches --last_item_rate 1.0 a '
                         'left-to-right next-item model')
    ap.add_argument('--mq_causal', action='store_true',
                    help='with --attention causal: evaluate the last encoder layer at the rows the head reads only (ops.mq_causal, off '
                         'by default)')
    add_train_loss_arguments(ap)
    add_objective_argument(ap)
    a = ap.parse_args()
    next_item = a.objective == 'next_item'
    if next_item and not a.device_batches:
        ap.error('--objective next_item needs --device_batches')
    check_train_loss_arguments(ap, a)
    protocol = dict(max_len=a.max_len, stride=a.stride, holdout=a.holdout, last_item_rate=a.last_item_rate)
    if not a.device_batches and protocol != dict(max_len=None, stride=None, holdout=1, last_item_rate=0.0):
        ap.error('--max_len, --stride, --holdout and --last_item_rate need --device_batches')
    from bert4clickpath_amd import checkpoint as ck, input_pipeline, ops, optim
    if a.mq_causal:
        ops.mq_causal = True
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    if a.device_batches:
        from bert4clickpath_amd.cloze_batches import DeviceCloze
        data = DeviceCloze.from_npz(a.data, **protocol)
    else:
        data = input_pipeline.BeautyCloze(a.data)
    dtype = torch.float32 if a.dtype == 'f32' else torch.bfloat16
    model = build_model(data.V, a.dropout, dtype, seed=1234 + a.seed, attention=a.attention, tied_head=a.train_loss != 'full').cuda()
    opt = optim.Adam(model.parameters())
    T.set_dropout_seed(a.seed)
    tmp = tempfile.mkdtemp(prefix='b4c_beauty_')
    saver = ck.ModelCheckpoint(tmp, model, opt, save_best_only=True)
    plateau = ck.ReduceLROnPlateau(opt, factor=0.317, patience=10)
    stopper = ck.EarlyStopping(patience=30)
    steps = a.steps_per_epoch * a.max_epochs
    sampling = train_sampling(data, a)
    batches = next_item_train_batches(data, a, steps, sampling['item_cdf']) if next_item else data.train_batches(a.batch, a.seed, steps)
    monitored = 'valid' if a.holdout == 2 else 'test'      # the split the callbacks see
    t0 = time.perf_counter()
    curve, stopped_by, best = [], 'max_epochs', None
    for epoch in range(a.max_epochs):
        tl = 0.0
        for _ in range(a.steps_per_epoch):
            b = next(batches)
            opt.zero_grad()
            if next_item:
                loss = next_item_training_loss(model, a, b, sampling['logq'])
            elif a.device_batches:
                loss = training_loss(model, a, {'asin': b['items']}, b['labels_padded'], **sampling,
                                     max_masked_per_row=b['labels_padded'].shape[1], n_real_tokens=b['n_real_tokens'])
            else:
                items = torch.from_numpy(b['ids'])[:, 2:-1].contiguous().cuda()
                loss = training_loss(model, a, {'asin': items}, torch.from_numpy(b['labels_padded']).cuda(), max_masked_per_row=10)
            loss.backward()
            opt.step()
            tl = loss
        val_loss, hr, nd = evaluate(model, data, split=monitored, next_item=next_item)
        row = {'epoch': epoch + 1, 'train_loss_last': float(tl), 'val_loss': val_loss, 'hitrate@10': hr, 'ndcg@10': nd,
               'lr': opt.lr, 'seconds': time.perf_counter() - t0}
        curve.append(row)
        if saver.on_epoch_end(epoch, val_loss, {'hitrate@10': hr, 'ndcg@10': nd}):
            best = row
        plateau.on_epoch_end(epoch, val_loss)
        if a.log:
            with open(a.log, 'a') as f:
                f.write(json.dumps(row) + '\n')
        print('epoch %d val_loss %.4f HR@10 %.2f lr %.2e (%.0f s)' % (epoch + 1, val_loss, hr, opt.lr, row['seconds']), flush=True)
        if stopper.on_epoch_end(epoch, val_loss):
            stopped_by = 'early_stopping'
            break
        if time.perf_counter() - t0 > a.max_seconds:
            stopped_by = 'time'
            break
    final = curve[-1]
    by_hr = max(curve, key=lambda r: r['hitrate@10'])
    report = {}
    if a.device_batches:
        report['data_protocol'] = dict(protocol, monitored_split=monitored)
    if a.holdout == 2:                 # the held-out last item, read once: the weights are the last epoch's
        loss, hr, nd = evaluate(model, data, split='test', next_item=next_item)
        report['test'] = {'loss': loss, 'hitrate@10': hr, 'ndcg@10': nd}
        _, fhr, fnd = evaluate(model, data, split='test', filtered=True, next_item=next_item)
        report['test'].update({'filtered_hitrate@10': fhr, 'filtered_ndcg@10': fnd})
    print(json.dumps({'what': 'Amazon Beauty, HIP path, reference loop controls (ReduceLROnPlateau 0.317/10, EarlyStopping 30, '
                              'best-val_loss checkpoint)', 'dtype': a.dtype, 'seed': a.seed, 'batch': a.batch,
                      'steps_per_epoch': a.steps_per_epoch, 'epochs_run': len(curve), 'stopped_by': stopped_by,
                      'final': final, 'best_val_loss_epoch': best, 'best_hitrate_epoch': by_hr, 'curve': curve, **report}))


if __name__ == '__main__':
    main()
