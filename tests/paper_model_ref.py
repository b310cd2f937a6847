"""float64 restatement of the two ends of the BERT4Rec paper's model -- the input stage drop(LayerNorm(scale * E + P)) and the
masked-item head's transform LayerNorm(act(Dense)) in front of the tied projection -- in torch CPU autograd.  NO REFERENCE
ORACLE: the reference's input stage is drop(E * sqrt(d) + P) without a norm and its head is untied; this file states what the
extensions mean, on top of oracle/torch_ref.py's pieces (layer_norm, dropout, the masked-row gather, the sparse CE) and
tests/paper_encoder_ref.py's activations.  Used by test_paper_model_cpu.py, test_gpu_embed_ln.py and test_gpu_paper_model.py."""
import numpy as np
import torch

import paper_encoder_ref as pr
from oracle import numpy_ref as nr
from oracle import torch_ref as tr

EPS = nr.LN_EPS         # 1e-6: the eps of every LayerNormalization of the package


# ---- the input stage -------------------------------------------------------------------------------------------------------
def embed_pre(ids_list, tables, pe, scale, combine='concat'):
    """pre [B, S, d] = scale * (concat_f | sum_f) table_f[clamp(ids_f)] + pe[s]: the row LayerNorm sees"""
    parts = [t[i.clamp(0, t.shape[0] - 1)] for i, t in zip(ids_list, tables)]
    x = sum(parts[1:], parts[0]) if combine == 'sum' else torch.cat(parts, dim=-1)
    S = ids_list[0].shape[1]
    return x * scale + pe[:S][None]


def ln_stats(pre, eps=EPS):
    """(mean, rstd) of every row: biased variance, eps inside the root"""
    mean = pre.mean(-1, keepdim=True)
    var = ((pre - mean) ** 2).mean(-1, keepdim=True)
    return mean, torch.rsqrt(var + eps)


def embed_ln(ids_list, tables, pe, scale, gamma, beta, keep=None, rate=0.0, combine='concat', eps=EPS):
    """drop(LayerNorm(pre)) [B, S, d]; keep: the host copy of the kernel's mask, shaped like the output (None: no dropout)"""
    pre = embed_pre(ids_list, tables, pe, scale, combine)
    return tr.dropout(tr.layer_norm(pre, gamma, beta, eps), rate, keep)


def ln_backward(dout, pre, gamma, keep=None, rate=0.0, eps=EPS):
    """closed form of the stage's backward up to the pre-norm row -> (dpre, dgamma, dbeta):
        g = keep / (1 - rate) * dout;  dbeta = sum_t g;  dgamma = sum_t g * xhat
        a = g * gamma;  dpre = rstd * (a - mean_j(a) - xhat * mean_j(a * xhat))"""
    d = pre.shape[-1]
    g = dout if (keep is None or rate == 0.0) else dout * keep.to(dout.dtype) / (1.0 - rate)
    mean, rstd = ln_stats(pre, eps)
    xh = (pre - mean) * rstd
    a = g * gamma
    dpre = rstd * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))
    return dpre, (g * xh).reshape(-1, d).sum(0), g.reshape(-1, d).sum(0)


# ---- the head's transform --------------------------------------------------------------------------------------------------
def head_transform(h, kernel, bias, gamma, beta, act='gelu_tanh', eps=EPS, relu=None):
    """LayerNorm(act(h W + b)); relu(z): what stands for a 'relu' activation (a bf16_gates recorder's on / off pattern)"""
    u = h @ kernel + bias
    return tr.layer_norm(relu(u) if (act == 'relu' and relu is not None) else pr.act(act, u), gamma, beta, eps)


def transform_backward(dout, h, kernel, bias, gamma, act='gelu_tanh', eps=EPS):
    """closed form -> (dh, dW, db, dgamma, dbeta): the LayerNorm backward above on a = act(u), then du = da * act'(u)"""
    u = h @ kernel + bias
    da, dgamma, dbeta = ln_backward(dout, pr.act(act, u), gamma, eps=eps)
    du = da * pr.act_grad(act, u)
    return du @ kernel.t(), h.t() @ du, du.sum(0), dgamma, dbeta


def tied_head_logits(x, hP, table, id_offset, V, transform=None, relu=tr._relu):
    """ClozeMaskedItemPrediction: relu(Dense) x n (all the intermediate layers without a transform, all but the last with one),
    the transform, then h . E[off : off + V]^T + output_bias.  hP: the head's state-dict entries without their 'head.' prefix.
    relu('head.<i>', z): the ReLU of Dense layer i, as torch_ref's heads take it (the transform's own, when it is 'relu', included)."""
    n = len([k for k in hP if k.startswith('intermediate_layers.') and k.endswith('.kernel')])
    for i in range(n - (1 if transform else 0)):
        x = relu('head.%d' % i, x @ hP['intermediate_layers.%d.kernel' % i] + hP['intermediate_layers.%d.bias' % i])
    if transform:
        x = head_transform(x, hP['intermediate_layers.%d.kernel' % (n - 1)], hP['intermediate_layers.%d.bias' % (n - 1)],
                           hP['transform_norm.gamma'], hP['transform_norm.beta'], transform,
                           relu=lambda z: relu('head.%d' % (n - 1), z))
    return x @ table[id_offset:id_offset + V].t() + hP['output_bias']


# ---- the model -------------------------------------------------------------------------------------------------------------
def encoder(x, pad, tP, num_layers, num_heads, ffn='relu'):
    """the encoder layers of torch_ref.transformer_forward (float64, no dropout) on the stage's output x [B, S, d]; pad [B, S]
    bool marks the pad keys; ffn: the feed-forward activation"""
    B, S, d = x.shape
    depth = d // num_heads
    neg = pad.to(x.dtype)[:, None, None, :] * -1e9
    for i in range(num_layers):
        p = 'encoder.enc_layers.%d.' % i

        def lin(t, name):
            return t @ tP[p + name + '.kernel'] + tP[p + name + '.bias']

        def split(t):
            return t.reshape(B, S, num_heads, depth).permute(0, 2, 1, 3)
        q, k, v = split(lin(x, 'mha.wq')), split(lin(x, 'mha.wk')), split(lin(x, 'mha.wv'))
        w = torch.softmax(q @ k.transpose(-1, -2) / float(np.sqrt(np.float32(depth))) + neg, dim=-1)
        o = (w @ v).permute(0, 2, 1, 3).reshape(B, S, d)
        out1 = tr.layer_norm(x + lin(o, 'mha.dense'), tP[p + 'layernorm1.gamma'], tP[p + 'layernorm1.beta'])
        f = lin(pr.act(ffn, lin(out1, 'ffn.0')), 'ffn.1')
        x = tr.layer_norm(out1 + f, tP[p + 'layernorm2.gamma'], tP[p + 'layernorm2.beta'])
    return x


def model_logits(ids, P, num_layers, num_heads, V, ffn='relu', transform=None, embedding_scale=None, feature='items',
                 id_offset=10):
    """-> logits [R, V] of the [MASK] rows (row-major) of a ClickstreamTransformer with a ClozeMaskedItemPrediction head.  P: the
    model's state dict as float64 leaves.  The input stage is the paper's when P holds 'transformer.embedding_norm.gamma', else
    the reference's; the positional table is P['transformer.position_embedding.weight'] or the sinusoid; embedding_scale None:
    the float32 sqrt(d_model)."""
    tP = {k[len('transformer.'):]: v for k, v in P.items() if k.startswith('transformer.')}
    hP = {k[len('head.'):]: v for k, v in P.items() if k.startswith('head.')}
    table = tP['embedding_layers.%s.weight' % feature]
    d = table.shape[1]
    S = ids.shape[1]
    pe = tP['position_embedding.weight'] if 'position_embedding.weight' in tP else tr.positional_encoding(S, d, table.dtype)
    scale = float(np.sqrt(np.float32(d))) if embedding_scale is None else float(embedding_scale)
    if 'embedding_norm.gamma' in tP:
        x = embed_ln([ids], [table], pe, scale, tP['embedding_norm.gamma'], tP['embedding_norm.beta'])
    else:
        x = embed_pre([ids], [table], pe, scale)
    enc = encoder(x, ids == nr.INPUT_PAD, tP, num_layers, num_heads, ffn)
    rows, _ = tr.gather_masked_rows(enc, ids)
    return tied_head_logits(rows, hP, table, id_offset, V, transform)


def model_loss(ids, labels_compact, P, num_layers, num_heads, V, **kw):
    """-> (mean TF sparse CE over the [MASK] rows, probabilities [R, V]) of model_logits(...)"""
    probs = torch.softmax(model_logits(ids, P, num_layers, num_heads, V, **kw), dim=-1)
    return tr.sparse_ce_tf(probs, labels_compact).sum() / labels_compact.numel(), probs
