"""float64 restatement of the pre-LN encoder (norm='pre') in torch CPU autograd.  NO REFERENCE ORACLE: the reference's blocks are
post-LN; this file states what the keyword means, on top of oracle/torch_ref.py's pieces (layer_norm, dropout, the rounders, the
head, the loss) and paper_encoder_ref.py's activations:

    n1 = LN(x; gamma1, beta1);  x'  = x  + drop_1(MHA(n1, n1, n1) Wo + bo)
    n2 = LN(x'; gamma2, beta2); x'' = x' + drop_2(act(n2 W1 + b1) W2 + b2)          per layer,
    out = LN(x_L; final_norm)                                                        after the last one.

Also the closed forms of the row kernel b4c_layernorm_bwd_add.  Used by test_pre_ln_cpu.py, test_gpu_pre_ln_kernels.py and
test_gpu_pre_ln_model.py."""
import math

import numpy as np
import torch

import paper_encoder_ref as pr
from oracle import numpy_ref as nr
from oracle import torch_ref as tr


def layer(x, P, pre, num_heads, neg, act='relu', dropout_rate=0.0, keep1=None, keep2=None, emulate_bf16=False, relu=None, tag='ffn.0',
          attn_rate=0.0, keep_attn=None):
    """One pre-LN layer on the stream x (B, S, d) -> the UN-normalised stream (torch's norm_first layer).  P[pre + name]: the
    layer's parameters under the state-dict names (dense kernels [in, out]); neg (B | 1, 1, S | 1, S): the additive attention mask
    (-1e9 on padded keys, -inf above the diagonal of a causal layer).  relu(tag, z): torch_ref's activation hook (None: `act`).
    attn_rate, keep_attn (B, H, S, S) bool: dropout on the attention probabilities (ops.attn_keep_mask's bits)."""
    rb, rg, rw = tr._rounders(emulate_bf16)
    B, S, d = x.shape
    depth = d // num_heads
    hook = relu if relu is not None else (lambda _tag, z: pr.act(act, z))

    def lin(t, name):
        return rb(t @ rw(P[pre + name + '.kernel'])) + P[pre + name + '.bias']

    def split(t):
        return t.reshape(B, S, num_heads, depth).permute(0, 2, 1, 3)
    n1 = rb(tr.layer_norm(rg(x), P[pre + 'layernorm1.gamma'], P[pre + 'layernorm1.beta']))
    q, k, v = split(rb(lin(n1, 'mha.wq'))), split(rb(lin(n1, 'mha.wk'))), split(rb(lin(n1, 'mha.wv')))
    # (the scale is the exact 1 / sqrt(depth): torch's own; torch_ref's float32 square root differs from it by 2e-8 at depth 8 or 32,
    # far below what any comparison with the kernels resolves, and not at all at depth 16 or 64)
    logits = rg(q @ k.transpose(-1, -2) / math.sqrt(depth)) + neg
    w = torch.softmax(logits, dim=-1)
    if attn_rate > 0 and keep_attn is not None:
        w = w * keep_attn.to(w.dtype) / (1.0 - attn_rate)
    o = w @ v
    o = rb(o.permute(0, 2, 1, 3).reshape(B, S, d))
    x = rb(x + tr.dropout(rb(lin(o, 'mha.dense')), dropout_rate, keep1))
    n2 = rb(tr.layer_norm(rg(x), P[pre + 'layernorm2.gamma'], P[pre + 'layernorm2.beta']))
    f = rb(lin(rb(hook(tag, lin(n2, 'ffn.0'))), 'ffn.1'))
    return rb(x + tr.dropout(f, dropout_rate, keep2))


def attention_mask(first_ids, dt, causal=False):
    """the additive mask of the kernels: -1e9 on padded keys; a causal layer excludes the keys behind the query outright (-inf)"""
    neg = (first_ids == nr.INPUT_PAD).to(dt)[:, None, None, :] * -1e9
    if causal:
        S = first_ids.shape[1]
        neg = neg + torch.zeros(S, S, dtype=dt).masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float('-inf'))
    return neg


def encoder(x, P, num_layers, num_heads, neg, act='relu', dropout_rate=0.0, keep_masks=None, emulate_bf16=False, relu=None,
            prefix='encoder.', attn_rate=0.0, keep_attn=None):
    """num_layers pre-LN layers and the final norm P[prefix + 'final_norm.gamma' / '.beta']; keep_masks: torch_ref's
    {'l<i>.1', 'l<i>.2'}; keep_attn: one (B, H, S, S) mask per layer"""
    rb, rg, _ = tr._rounders(emulate_bf16)
    km = keep_masks or {}
    for i in range(num_layers):
        x = layer(x, P, prefix + 'enc_layers.%d.' % i, num_heads, neg, act, dropout_rate, km.get('l%d.1' % i), km.get('l%d.2' % i),
                  emulate_bf16, relu, 'ffn.%d' % i, attn_rate, keep_attn[i] if keep_attn else None)
    return rb(tr.layer_norm(rg(x), P[prefix + 'final_norm.gamma'], P[prefix + 'final_norm.beta']))


def transformer_forward(causal=False, attn_rate=0.0, keep_attn=None):
    """torch_ref.transformer_forward's signature with the pre-LN encoder behind the (unchanged) embedding stage"""
    def forward(ids_by_feature, P, num_layers, num_heads, dropout_rate=0.0, keep_masks=None, emulate_bf16=False, relu=tr._relu,
                combine='concat'):
        rb, _, _ = tr._rounders(emulate_bf16)
        feats = list(ids_by_feature.keys())
        first = ids_by_feature[feats[0]]
        B, S = first.shape
        parts = [P['embedding_layers.%s.weight' % f][ids_by_feature[f]] for f in feats]
        x = sum(parts[1:], parts[0]) if combine == 'sum' else torch.cat(parts, dim=-1)
        d = x.shape[-1]
        x = x * float(np.sqrt(np.float32(d))) + tr.positional_encoding(S, d, x.dtype)[None]
        x = rb(tr.dropout(x, dropout_rate, (keep_masks or {}).get('emb')))
        return encoder(x, P, num_layers, num_heads, attention_mask(first, x.dtype, causal), 'relu', dropout_rate, keep_masks,
                       emulate_bf16, relu, attn_rate=attn_rate, keep_attn=keep_attn)
    return forward


def model_loss(ids, labels_compact, P, num_layers, num_heads, n_hidden, ffn='relu', relu=tr._relu, causal=False, attn_rate=0.0,
               keep_attn=None, **kw):
    """paper_encoder_ref.model_loss (same hooks: ffn, relu, a learned positional table in P, torch_ref.model_loss's keywords) of the
    pre-LN model; causal: left-to-right attention; attn_rate, keep_attn: attention dropout with one regenerated mask per layer"""
    orig = tr.transformer_forward
    tr.transformer_forward = transformer_forward(causal, attn_rate, keep_attn)
    try:
        return pr.model_loss(ids, labels_compact, P, num_layers, num_heads, n_hidden, ffn=ffn, relu=relu, **kw)
    finally:
        tr.transformer_forward = orig


# ---- b4c_layernorm_bwd_add in closed form ----------------------------------------------------------------------------------
def ln_bwd_add(dout, x, mean, rstd, gamma, res):
    """float64 (dx, dgamma, dbeta) of  dx = res + rstd * (a - mean_j(a) - xhat * mean_j(a * xhat)),  a = dout * gamma,
    xhat = (x - mean) * rstd, dgamma = sum_rows dout * xhat, dbeta = sum_rows dout.  mean, rstd [rows]: the SAVED stats (the
    kernel's inputs), everything taken to float64 as given."""
    dout, x, gamma, res = dout.double(), x.double(), gamma.double(), res.double()
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    xhat = (x - mean) * rstd
    a = dout * gamma
    dx = res + rstd * (a - a.mean(1, keepdim=True) - xhat * (a * xhat).mean(1, keepdim=True))
    return dx, (dout * xhat).sum(0), dout.sum(0)


def ln_bwd_add_autograd(dout, x, gamma, res, eps=nr.LN_EPS):
    """the same dx through autograd of tr.layer_norm (stats taken from x in float64): the closed form's own check"""
    x = x.double().clone().requires_grad_(True)
    g = gamma.double().clone().requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    tr.layer_norm(x, g, b, eps).backward(dout.double())
    return res.double() + x.grad, g.grad, b.grad
