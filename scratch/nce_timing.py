"""The fused in-batch contrastive loss (ops.nce_fwd + ops.nce_bwd) against the same loss built from the existing kernels, at
N = 8192, K = 128, bf16 (the benchmark's batch: N = 2B): b4c_gemm_nt into fp32 logits [N, N], b4c_softmax_ce_fwd_bwd in place, the
cast of the 268 MB of dlogits to the GEMMs' bf16 operand, and two GEMMs for dz (dlogits z and dlogits^T z).  The materialised route
is timing only: it cannot leave the diagonal or a group out of the log-sum-exp without an [N, N] mask, so its numbers are not the
loss's.  The two routes alternate inside one process, WINDOWS windows of ITERS iterations each, HIP events around every window.
usage: python scratch/nce_timing.py [out.json]"""
import json
import sys

import torch

from bert4clickpath_amd import _lib as L
from bert4clickpath_amd import ops

N, K, WINDOWS, ITERS, TEMP = 8192, 128, 7, 20, 0.5


def main():
    torch.manual_seed(0)
    z = (torch.randn(N, K, device='cuda') * 0.3).bfloat16()
    zt = z.t().contiguous()
    idx = torch.arange(N, dtype=torch.int32, device='cuda')
    pos = torch.cat([idx[N // 2:], idx[:N // 2]]).contiguous()
    gscale = torch.full((1,), 1.0 / N, device='cuda')
    zs = (z.float() / TEMP).bfloat16()                      # the temperature folded into one operand

    def fused_fwd(sim):
        return ops.nce_fwd(z, pos, None, TEMP, sim)

    def fused(sim):
        item, lse, rnorm = ops.nce_fwd(z, pos, None, TEMP, sim)
        return ops.nce_bwd(z, pos, None, TEMP, sim, rnorm, lse, gscale)

    def materialised():
        logits = ops.gemm_nt(zs, z, N, out_dtype=torch.float32)
        ops.softmax_ce_fwd_bwd_(logits, pos, gscale, N, L.CE_PLAIN)
        dl = logits.bfloat16()
        a = ops.gemm_nt(dl, zt, K, out_dtype=torch.float32)
        b, _ = ops.gemm_tn(dl, z, N, K, want_bias=False)
        return a + b

    routes = {'fused fwd (dot)': lambda: fused_fwd('dot'), 'fused fwd+bwd (dot)': lambda: fused('dot'),
              'fused fwd+bwd (cos)': lambda: fused('cos'), 'materialised fwd+bwd': materialised}
    for f in routes.values():                               # warm-up: allocator, workspaces, LDS opt-in
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(WINDOWS):
        for name, f in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(ITERS):
                f()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / ITERS)
    out = {'N': N, 'K': K, 'dtype': 'bf16', 'windows': WINDOWS, 'iters': ITERS, 'device': torch.cuda.get_device_name(0), 'ms': {}}
    for name, t in times.items():
        t = sorted(t)
        out['ms'][name] = {'median': t[len(t) // 2], 'min': t[0], 'max': t[-1]}
        print('%-24s %.3f ms  [%.3f - %.3f]' % (name, t[len(t) // 2], t[0], t[-1]))
    flops = 2.0 * N * N * K
    out['tflops'] = {'fwd': flops / out['ms']['fused fwd (dot)']['median'] * 1e-9,
                     'fwd+bwd': 3 * flops / out['ms']['fused fwd+bwd (dot)']['median'] * 1e-9}
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
