"""A/B of Adam(global_clipnorm=...) inside bench.Training's step: windows of warmed steps alternate, in ONE process, between
`opt.global_clipnorm = None` (the launches of the commit before the feature, bit for bit: tests/test_gpu_clipnorm.py) and
`= 5.0`, device-event timed.  Prints every window, the medians, the spread of the None windows among themselves, and the id
counts the row form was handed (config 5).

    python scratch/clip_ab.py --config c2 [--windows 5] [--steps 100] [--warmup 30] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scratch/clip_ab.py --config c2 --windows 1 --steps 20      (kernel times)
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
    ap.add_argument('--windows', type=int, default=5, help='alternations: each is one None window and one clipped window')
    ap.add_argument('--steps', type=int, default=100, help='steps per window')
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--clip', type=float, default=5.0)
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
    # the ids the row form is handed in one step
    named = []
    orig = optim.LazyRows.grad_sumsq

    def counting(self, partial):
        named.append((self.rows, 'all_rows' if self.all_rows else sum(int(i.numel()) for i in self.touched)))
        return orig(self, partial)
    optim.LazyRows.grad_sumsq = counting
    opt.global_clipnorm = o.clip
    tr.step(step_no)
    step_no += 1
    optim.LazyRows.grad_sumsq = orig
    torch.cuda.synchronize()
    say('one clipped step: grad norm %.6g; ids named per lazy table (rows, ids): %s' % (float(opt.last_grad_norm), named))

    def window(clip):
        nonlocal step_no
        opt.global_clipnorm = clip
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
    for w in range(o.windows):
        off.append(window(None))
        on.append(window(o.clip))
        say('alternation %d: None %.1f us/step   clip=%g %.1f us/step   difference %+.1f us' % (w, off[-1], o.clip, on[-1], on[-1] - off[-1]))
    m_off, m_on = statistics.median(off), statistics.median(on)
    say('median None %.1f us/step, median clipped %.1f us/step, median difference %+.1f us (%.2f %%)' % (
        m_off, m_on, m_on - m_off, 100.0 * (m_on - m_off) / m_off))
    say('spread of the None windows among themselves: min %.1f max %.1f (max - min %.1f us)' % (min(off), max(off), max(off) - min(off)))
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
