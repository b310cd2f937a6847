"""Cost of b4c_embed_ln_fwd / _bwd against the composition the plain kernels allow (forward: embed_fwd at rate 0 -> add_ln_fwd with
a zero y -> b4c_dropout; backward: add_ln_bwd), and of the paper-model training step against the same model with
embedding_layernorm=False, transform=None.  C2 token count (B = 4096, S = 200, packed rows), d = 128, bf16, dropout 0.1; the
variants are interleaved, medians [min - max] over the rounds.  Needs the MI355X:

    python scratch/paper_cost.py [out.json]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4clickpath_amd import input_pipeline, ops, optim                                   # noqa: E402
from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, ClozeMaskedItemPrediction      # noqa: E402

OUT = {}
B, S, V, D = 4096, 200, 50000, 128


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1000.0        # us per call


def med(xs):
    return '%.1f [%.1f - %.1f]' % (statistics.median(xs), min(xs), max(xs))


def kernels():
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=4321)
    ids = torch.from_numpy(b['ids']).cuda().contiguous()
    n_real = int((b['ids'] != 0).sum())
    counts, cu, tok_src, packed_of, mx = ops.nonpad_positions(ids, n_real)
    pk = ops.Packed(cu, tok_src, packed_of, B, S, n_real, int(mx.item()))
    g = torch.Generator().manual_seed(0)
    table = (torch.randn(V + 11, D, generator=g) * 0.5).cuda()
    pe = (torch.randn(S, D, generator=g) * 0.5).cuda()
    gamma, beta = torch.ones(D, device='cuda'), torch.zeros(D, device='cuda')
    bf = torch.bfloat16
    dout = torch.randn(n_real, D, generator=g).to(bf).cuda()
    zero_y = torch.zeros(n_real, D, dtype=bf, device='cuda')
    out, _, stats = ops.embed_ln_fwd([ids], [table], pe, 1.0, gamma, beta, 0.1, 7, bf, pk)
    x, _ = ops.embed_concat_pe_fwd([ids], [table], pe, 1.0, 0.0, 0, bf, pk)
    z, o2, st2 = ops.add_dropout_layernorm_fwd(x.reshape(-1, D), zero_y, gamma, beta, 0.0, 0)
    # the two forwards agree up to the bf16 rounding of x in the composition
    comp = ops.dropout(o2, 0.1, 7)
    OUT['fwd_max_abs_diff_fused_vs_composition'] = float((out.reshape(-1, D).float() - comp.float()).abs().max())
    dg, db = torch.zeros(D, device='cuda'), torch.zeros(D, device='cuda')

    def f_fused():
        ops.embed_ln_fwd([ids], [table], pe, 1.0, gamma, beta, 0.1, 7, bf, pk, out=out, stats=stats)

    def f_comp():
        xx, _ = ops.embed_concat_pe_fwd([ids], [table], pe, 1.0, 0.0, 0, bf, pk)
        _, oo, _ = ops.add_dropout_layernorm_fwd(xx.reshape(-1, D), zero_y, gamma, beta, 0.0, 0)
        ops.dropout(oo, 0.1, 7)

    def b_fused():
        ops.embed_ln_bwd([ids], [table], pe, 1.0, gamma, stats, dout, 0.1, 7, pk, into=(dg, db))

    def b_comp():
        ops.add_dropout_layernorm_bwd(dout, z, st2, gamma, 0.0, 0, into=(dg, db))
    fns = {'fwd_fused': f_fused, 'fwd_composition': f_comp, 'bwd_fused': b_fused, 'bwd_composition': b_comp}
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(8):
        for k, f in fns.items():
            res[k].append(timed(f, 20))
    es = 2
    OUT['tokens'] = n_real
    OUT['bytes_fwd_MB'] = (n_real * D * (4 + es) + 8 * n_real) / 1e6
    OUT['bytes_bwd_MB'] = (n_real * D * (4 + 2 * es) + 8 * n_real) / 1e6
    for k, v in res.items():
        OUT[k + '_us'] = med(v)
        print(k, med(v), 'us', flush=True)


def model(paper):
    torch.manual_seed(3)
    head = ClozeMaskedItemPrediction([], V, transform='gelu_tanh' if paper else None)
    return ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': D}, head,
                                  value_to_head='[MASK]', num_encoder_layers=4, num_attention_heads=2, encoder_ff_dim=512,
                                  dropout_rate=0.1, compute_dtype=torch.bfloat16, ffn_activation='gelu_tanh',
                                  position_encoding='learned', max_positions=S, embedding_layernorm=paper,
                                  embedding_scale=1.0 if paper else None).cuda()


def steps():
    batches = []
    for j in range(3):
        b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=4321 + 1000 * j)
        ids = torch.from_numpy(b['ids'])
        batches.append(({'asin': ids[:, 2:S - 1].contiguous().cuda()}, torch.from_numpy(b['labels_padded']).cuda(),
                        int((b['ids'] != 0).sum())))
    runs = {}
    for name, paper in (('paper', True), ('plain_ends', False)):
        m = model(paper)
        runs[name] = (m, optim.Adam(m.parameters()))
    i = [0]

    def step(name):
        m, opt = runs[name]
        feats, labels, n_real = batches[i[0] % 3]
        i[0] += 1
        opt.zero_grad()
        loss = m.cloze_loss(feats, labels, training=True, max_masked_per_row=10, n_real_tokens=n_real)
        loss.backward()
        opt.step()
    for name in runs:
        for _ in range(4):
            step(name)
    torch.cuda.synchronize()
    res = {k: [] for k in runs}
    for _ in range(6):
        for name in runs:
            res[name].append(timed(lambda: step(name), 10) / 1000.0)
    for k, v in res.items():
        OUT['step_' + k + '_ms'] = '%.2f [%.2f - %.2f]' % (statistics.median(v), min(v), max(v))
        print('step', k, OUT['step_' + k + '_ms'], 'ms', flush=True)


if __name__ == '__main__':
    assert torch.cuda.is_available()
    kernels()
    steps()
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as f:
            json.dump(OUT, f, indent=1)
    print(json.dumps(OUT))
