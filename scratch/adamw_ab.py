"""A/B of Adam(weight_decay=...) inside bench.Training's step: windows of warmed steps, in ONE process, with
`opt.weight_decay = None` (the entry points of the commit before the feature: tests/test_gpu_adamw.py counts the calls) and
`= 0.01` with the BERT exclusions (optim.no_decay_params), device-event timed.  Prints every window, the medians and the spread
of the None windows among themselves.

--order alternate: None and decayed windows alternate, so drift over the run cancels.  A row-lazy table that has decayed keeps
  the AdamW row kernel while its rows may owe decayed steps, so each switch back to None is followed by sync_rows() +
  reset_rows() (outside the timed part): the None windows then launch the plain kernels.  Each decayed window starts with every
  row stamped, so its rotation replays at most as many steps as the window is old: with 100-step windows the replay never
  reaches max_staleness = 256.
--order blocks: all None windows first, then all decayed windows in one stretch: the later ones are the steady state (replays
  of max_staleness steps), but drift over the run is not cancelled.

    python scratch/adamw_ab.py --config c2 [--windows 5] [--steps 100] [--warmup 30] [--out FILE]
    python scratch/adamw_ab.py --config c5 --order blocks
    rocprofv3 --kernel-trace --stats -d DIR -- python scratch/adamw_ab.py --config c2 --windows 1 --steps 20      (kernel times)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='c2', choices=['c2', 'c4', 'c5'])
    ap.add_argument('--windows', type=int, default=5, help='alternations: each is one None window and one decayed window')
    ap.add_argument('--steps', type=int, default=100, help='steps per window')
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--weight_decay', type=float, default=0.01)
    ap.add_argument('--order', default='alternate', choices=['alternate', 'blocks'])
    ap.add_argument('--out', default=None)
    o = ap.parse_args()
    sys.argv = ['bench.py', '--config', o.config, '--no_cpu_baseline']
    import bench
    from bert4clickpath_amd import optim
    a = bench.parse()
    device = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    tr = bench.Training(a, 0, 1, device)
    opt = tr.opt
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('config %s: arena %d fp32 elements (%d chunks), dense share %d, lazy tables %s' % (
        o.config, opt.arena.numel, (opt.arena.numel + 1023) // 1024, sum(hi - lo for lo, hi in opt.dense_ranges) if opt.lazy else opt.arena.numel,
        [(lz.rows, lz.width) for lz in opt.lazy]))
    step_no = 0
    for _ in range(o.warmup):
        tr.step(step_no)
        step_no += 1
    # the BERT convention, on an optimizer that bench.py built without the argument.  This writes the optimizer's private
    # exclusion state, which is only sound BEFORE its first decayed step: the device copy of the block flags is built then
    assert opt._decay_blocks_dev is None and opt.weight_decay is None
    opt._no_decay = {id(p) for p in optim.no_decay_params(tr.model)}
    for lz in opt.lazy:
        lz.decay = id(lz.p) not in opt._no_decay
    blocks = opt.decay_blocks_host()
    say('decayed blocks: %d of %d (%d bytes of flags); decayed lazy tables %s' % (
        int(blocks.sum()), blocks.numel(), blocks.numel(), [(lz.rows, lz.width) for lz in opt.lazy if lz.decay]))

    def window(wd):
        nonlocal step_no
        if wd is None and opt._decay_seen:      # back to the plain kernels (see --order alternate above)
            opt.sync_rows()
            opt.reset_rows()
        opt.weight_decay = wd
        for _ in range(5):                  # settle after the switch
            tr.step(step_no)
            step_no += 1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(o.steps):
            tr.step(step_no)
            step_no += 1
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / o.steps        # us per step

    off, on = [], []
    if o.order == 'blocks':
        off = [window(None) for _ in range(o.windows)]
        on = [window(o.weight_decay) for _ in range(o.windows)]
    for w in range(o.windows):
        if o.order == 'alternate':
            off.append(window(None))
            on.append(window(o.weight_decay))
        say('%s %d: None %.1f us/step   weight_decay=%g %.1f us/step   difference %+.1f us' % (
            'alternation' if o.order == 'alternate' else 'window', w, off[w], o.weight_decay, on[w], on[w] - off[w]))
    m_off, m_on = statistics.median(off), statistics.median(on)
    say('median None %.1f us/step, median decayed %.1f us/step, median difference %+.1f us (%.2f %%)' % (
        m_off, m_on, m_on - m_off, 100.0 * (m_on - m_off) / m_off))
    say('spread of the None windows among themselves: min %.1f max %.1f (max - min %.1f us)' % (min(off), max(off), max(off) - min(off)))
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
