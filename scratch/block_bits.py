"""Launches and bits of the autograd blocks (ops.EmbedFn / EmbedLNFn, AttnBlockFn, MQAttnBlockFn, FFNBlockFn, DenseActLNFn, MLPFn), for
comparing two checkouts that share one libb4c_hip.so (B4C_LIB_PATH): a host-side change of the blocks must leave every field equal.
Per configuration: three optimizer steps as tests/test_gpu_deterministic.py::_run takes them (V = 3000, B = 96, S = 64, fixed dropout
seed, ops.deterministic on), in an arena (optim.Adam) and without one (torch.optim.Adam, fresh sinks), on the packed and the dense
layout; recorded are the losses, the (family, bytes) launch list and a SHA-256 of every parameter and of every gradient of the last
backward pass.
usage: python scratch/block_bits.py out.json            (run from the checkout under test)
       python scratch/block_bits.py --compare a.json b.json     (exit status 1 and the differing fields when they differ)"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V, B, S = 3000, 96, 64
UNFUSED = {'fused_attn_out_bwd': False, 'fused_ffn_fwd': False, 'fused_ffn_bwd': False, 'fused_dxdw': 0}
# name -> (model keywords, ops switches, extras: 'two' features, 'tied' head with a transform, 'lazy' tables, 'fp32')
CONFIGS = {
    'default': ({}, {}, ()),
    'fp32': ({}, {}, ('fp32',)),
    'two_concat': ({}, {}, ('two',)),
    'two_sum': ({'feature_combine': 'sum'}, {}, ('two',)),
    'learned': ({'position_encoding': 'learned', 'max_positions': S}, {}, ()),
    'embed_ln_learned': ({'position_encoding': 'learned', 'max_positions': S, 'embedding_layernorm': True}, {}, ()),
    'gelu_tanh_dff136': ({'ffn_activation': 'gelu_tanh', 'encoder_ff_dim': 136}, {}, ()),
    'attn_drop_full_last': ({'attention_dropout_rate': 0.2}, {'mq_attn_dropout': False}, ()),
    'attn_drop_mq_last': ({'attention_dropout_rate': 0.2}, {'mq_attn_dropout': True}, ()),
    'no_mq_last_layer': ({}, {'mq_last_layer': False}, ()),
    'unfused': ({}, UNFUSED, ()),
    'tied_transform': ({}, {}, ('tied',)),
    'lazy_rows': ({}, {}, ('lazy',)),
}


def sha(t):
    if t is None:
        return None
    return hashlib.sha256(t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def run(model_kw, extras, arena, packed):
    from bert4clickpath_amd import input_pipeline, ops, optim
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, ClozeMaskedItemPrediction, SoftMaxHead
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    two = 'two' in extras
    torch.manual_seed(5)
    chains, vocabs, dims = {'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': 128}
    if two:
        chains['actions'], vocabs['actions'] = ['act'], ['a%d' % i for i in range(20)]
        dims = {'items': 128, 'actions': 128} if model_kw.get('feature_combine') == 'sum' else {'items': 96, 'actions': 32}
    head = ClozeMaskedItemPrediction([64, 128], V, transform='gelu_tanh') if 'tied' in extras else SoftMaxHead([64, 128], V)
    m = ClickstreamTransformer(chains, vocabs, dims, head, value_to_head='[MASK]', num_encoder_layers=3, num_attention_heads=2,
                               dropout_rate=0.1, compute_dtype=torch.float32 if 'fp32' in extras else torch.bfloat16,
                               **model_kw).to('cuda')
    if arena:
        lazy = [p for n, p in m.named_parameters() if 'embedding_layers' in n] if 'lazy' in extras else []
        opt = optim.Adam(m.parameters(), lazy_rows=lazy)
    else:
        opt = torch.optim.Adam(m.parameters())
    T.set_dropout_seed(777)
    ops.family_log = []
    losses = []
    for i in range(3):
        b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=100 + i, min_len=10, n_extra_features=1 if two else 0, extra_vocab=20)
        feats = {'asin': torch.from_numpy(b['ids'])[:, 2:S - 1].contiguous().cuda()}
        if two:
            feats['act'] = torch.from_numpy(b['extra'][0])[:, 2:S - 1].contiguous().cuda()
        opt.zero_grad()
        layout = {'n_real_tokens': int((b['ids'] != 0).sum())} if packed else {'packed': False}
        loss = m.cloze_loss(feats, torch.from_numpy(b['labels_padded']).cuda(), training=True, max_masked_per_row=10, **layout)
        loss.backward()
        if i == 2:
            if arena:
                ops.join_side_work(opt.arena.ctx)
            torch.cuda.synchronize()
            grads = {n: sha(p.grad) for n, p in m.named_parameters()}
        opt.step()
        losses.append(float(loss.detach()).hex())
    torch.cuda.synchronize()
    return {'losses': losses, 'launches': [[f, int(n)] for f, n in ops.family_log], 'grads': grads,
            'params': {n: sha(p) for n, p in m.named_parameters()}}


def main(out_path):
    from bert4clickpath_amd import ops
    print('package under test:', os.path.dirname(ops.__file__), flush=True)
    names = ('deterministic', 'family_log', 'mq_attn_dropout', 'mq_last_layer') + tuple(UNFUSED)
    out = {}
    for name, (model_kw, switches, extras) in CONFIGS.items():
        for arena in (True, False):
            if 'lazy' in extras and not arena:
                continue            # optim.LazyRows is the arena optimizer's
            for packed in ((True, False) if 'fp32' not in extras else (False,)):     # (the packed layout is bf16 only)
                prev = {k: getattr(ops, k) for k in names}
                ops.deterministic = True
                for k, v in switches.items():
                    setattr(ops, k, v)
                try:
                    key = '%s/%s/%s' % (name, 'arena' if arena else 'no_arena', 'packed' if packed else 'dense')
                    out[key] = run(model_kw, extras, arena, packed)
                    print(key, out[key]['losses'][-1], len(out[key]['launches']), 'launches', flush=True)
                finally:
                    for k, v in prev.items():
                        setattr(ops, k, v)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = ['%s: in one file only' % k for k in sorted(set(a) ^ set(b))]
    for k in sorted(set(a) & set(b)):
        bad += ['%s: %s differ' % (k, field) for field in sorted(set(a[k]) | set(b[k])) if a[k].get(field) != b[k].get(field)]
    print('\n'.join(bad) if bad else '%d configurations, every field equal' % len(a))
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])
