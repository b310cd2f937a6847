"""What the causal masked-query last layer (ops.mq_causal) does to ranking with a causal model at rows the caller names
("Causal form of the masked-query last layer").

A causal model of bench.py's C2 shape (V = 50,000, S = 200, d_model = 128, H = 2, B = 4096, bf16, the packed layout, bench.py's
sequence lengths and head), L = 2 and L = 4 encoder layers.  The rows are those of a next-item evaluation batch: one query row per
sequence, at its last input.  The call is predict_topk(feats, 10, labels, flat_idx=, row_offsets=, n_real_tokens=):
  off   ops.mq_causal off: the full last layer, rows gathered -- the parent commit's route, the yardstick
  on    ops.mq_causal on: the last layer at the B query rows (b4c_attn_mq_fwd_ex, B4C_ATTN_CAUSAL)
interleaved round by round in ONE process; a round is `--calls` timed calls between two device events each, its figure their median;
the table reports the median [min - max] of the rounds.  The launch recorder (ops.start_recording) gives the per-family device time
of one call of each route on the last round.

  python scratch/mq_causal_rank.py OUT.json [--rounds 5] [--calls 10] [--warmup 5]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    argv = sys.argv[1:]
    out_path = argv[0]
    opt = {'--rounds': 5, '--calls': 10, '--warmup': 5}
    for k, v in zip(argv[1::2], argv[2::2]):
        opt[k] = type(opt[k])(v)
    import numpy as np
    import torch
    import bench
    from bert4clickpath_amd import input_pipeline, ops
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    sys.argv = ['bench.py']
    a = bench.parse()
    assert torch.cuda.is_available(), 'needs the MI355X'
    device = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    b = input_pipeline.synthetic_cloze_batch(a.batch, a.seq, a.vocab, seed=4321)
    ids = torch.from_numpy(b['ids'])
    lens = b['lens'].astype(np.int64)                              # items per sequence; the row is [CLS] [SEP] items [SEP]
    feats = {'asin': ids[:, 2:a.seq - 1].contiguous().to(device)}
    flat = torch.from_numpy((np.arange(a.batch) * a.seq + lens + 1).astype(np.int32)).to(device)      # the last item of every row
    off = torch.arange(a.batch + 1, dtype=torch.int32, device=device)
    labels = torch.from_numpy(np.random.default_rng(1).integers(0, a.vocab, a.batch).astype(np.int32)).to(device)
    n_real = int((b['ids'] != 0).sum())
    out = {'what': 'predict_topk(flat_idx=, row_offsets=) of a causal model, ms per call (device events), routes interleaved in one process',
           'shape': {'V': a.vocab, 'S': a.seq, 'd_model': a.d_model, 'H': a.heads, 'B': a.batch, 'dtype': 'bf16', 'layout': 'packed',
                     'rows': a.batch, 'real_tokens': n_real},
           'rounds': opt['--rounds'], 'calls_per_round': opt['--calls'], 'layers': {}}
    for L in (2, 4):
        torch.manual_seed(1234)
        model = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(a.vocab)]}, {'items': a.d_model},
                                       SoftMaxHead([1024, 512, 256, 128], a.vocab), value_to_head='[MASK]', num_encoder_layers=L,
                                       num_attention_heads=a.heads, dropout_rate=a.dropout, encoder_ff_dim=a.dff,
                                       compute_dtype=torch.bfloat16, attention='causal').to(device)

        def call():
            return model.predict_topk(feats, 10, labels, flat_idx=flat, row_offsets=off, n_real_tokens=n_real)

        res = {}
        for name in ('off', 'on'):
            ops.mq_causal = name == 'on'
            for _ in range(opt['--warmup']):
                res[name] = call()
        ops.mq_causal = False
        torch.cuda.synchronize()
        same_top1 = float((res['off'][0][:, 0] == res['on'][0][:, 0]).float().mean())
        ms = {'off': [], 'on': []}
        fams = {}
        for r in range(opt['--rounds']):
            for name in ('off', 'on'):
                ops.mq_causal = name == 'on'
                call()                                             # one untimed call after the switch
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(opt['--calls'] + 1)]
                torch.cuda.synchronize()
                ev[0].record()
                for s in range(opt['--calls']):
                    call()
                    ev[s + 1].record()
                torch.cuda.synchronize()
                ms[name].append(statistics.median(ev[s].elapsed_time(ev[s + 1]) for s in range(opt['--calls'])))
                if r == opt['--rounds'] - 1:                       # the launch recorder brackets every launch with events: a run of its own
                    ops.start_recording()
                    call()
                    rec = ops.stop_recording()
                    fams[name] = {f: {'ms': v['ms'], 'launches': v['launches']} for f, v in rec.items()}
        ops.mq_causal = False
        out['layers'][str(L)] = {'ms_per_call_by_round': ms, 'ms_per_call_median': {n: statistics.median(v) for n, v in ms.items()},
                                 'ms_per_call_spread': {n: [min(v), max(v)] for n, v in ms.items()},
                                 'first_ranked_item_equal_share': same_top1, 'launch_families_one_call': fams}
        del model
    with open(out_path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps({L: (v['ms_per_call_median'], v['ms_per_call_spread'], v['first_ranked_item_equal_share'])
                      for L, v in out['layers'].items()}))


if __name__ == '__main__':
    main()
