"""What the masked-query last layer with attention dropout (ops.mq_attn_dropout) wins back on bench.py's training step (DESIGN.md
section 7, profiles/mq_attn_dropout_cost.json).

One bench.Training object (the C2 workload: bf16, packed, dropout 0.1, unless other bench.py arguments are given after `--`),
three variants of its step, interleaved round by round in ONE process so that they share the machine's state:
  off     attention_dropout_rate 0.2, ops.mq_attn_dropout off: the full last layer with its masks, rows gathered (the default)
  on      attention_dropout_rate 0.2, ops.mq_attn_dropout on: the last layer at the [MASK] rows, masks on those rows only
  base    attention_dropout_rate 0: the masked-query last layer without masks (the common baseline)
off - on = what the route wins back; on - base = the masks of the other layers plus those on the R query rows.  Step times are
device events around each step; the per-launch attention figures are the launch recorder's (ops.start_recording) on the last round:
attn_mq_fwd / attn_mq_bwd of `on` carry the masks, those of `base` do not.

  python scratch/mq_attn_dropout_cost.py OUT.json [--rounds 5] [--steps 20] [--rate 0.2] [-- bench.py arguments]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    argv = sys.argv[1:]
    bench_args = []
    if '--' in argv:
        i = argv.index('--')
        argv, bench_args = argv[:i], argv[i + 1:]
    out_path = argv[0]
    opt = {'--rounds': 5, '--steps': 20, '--rate': 0.2, '--warmup': 20}
    for k, v in zip(argv[1::2], argv[2::2]):
        opt[k] = type(opt[k])(v)
    import torch
    import bench
    from bert4clickpath_amd import ops
    sys.argv = ['bench.py'] + bench_args
    a = bench.parse()
    device = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    tr = bench.Training(a, 0, 1, device)
    enc = tr.model.transformer.encoder

    def variant(name):
        rate = 0.0 if name == 'base' else opt['--rate']
        ops.mq_attn_dropout = name == 'on'
        tr.model.attention_dropout_rate = tr.model.transformer.attention_dropout_rate = enc.attention_dropout_rate = rate
        for layer in enc.enc_layers:
            layer.attention_dropout_rate = rate

    names = ['off', 'on', 'base']
    it = 0
    for name in names:
        variant(name)
        for _ in range(opt['--warmup']):
            tr.step(it)
            it += 1
    ms = {n: [] for n in names}
    fams = {}
    for r in range(opt['--rounds']):
        for name in names:
            variant(name)
            tr.step(it)                    # one untimed step after the switch
            it += 1
            last = r == opt['--rounds'] - 1
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(opt['--steps'] + 1)]
            torch.cuda.synchronize()
            ev[0].record()
            for s in range(opt['--steps']):
                tr.step(it)
                it += 1
                ev[s + 1].record()
            torch.cuda.synchronize()
            ms[name].append(statistics.median(ev[s].elapsed_time(ev[s + 1]) for s in range(opt['--steps'])))
            if last:                       # the launch recorder brackets every launch with events: a run of its own
                ops.start_recording()
                for s in range(3):
                    tr.step(it)
                    it += 1
                rec = ops.stop_recording()
                fams[name] = {f: {'ms_per_launch': v['ms'] / v['launches'], 'launches_per_step': v['launches'] / 3}
                              for f, v in rec.items() if f.startswith('attn')}
    out = {'what': 'bench.py training step, median ms per step of each round (device events), variants interleaved in one process',
           'bench_args': bench_args, 'rate': opt['--rate'], 'rounds': opt['--rounds'], 'steps_per_round': opt['--steps'],
           'ms_per_step_by_round': ms, 'ms_per_step_median': {n: statistics.median(v) for n, v in ms.items()},
           'ms_per_step_spread': {n: [min(v), max(v)] for n, v in ms.items()}, 'attention_launches': fams}
    with open(out_path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
