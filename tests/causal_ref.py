"""float64 restatement of causal (left-to-right) self-attention (an extension: the reference's encoder never builds a look-ahead
mask, so there is NO REFERENCE ORACLE under oracle/; this file is the checker, as tests/attn_dropout_ref.py is for attention dropout).

Semantics (include/b4c.h, B4C_ATTN_CAUSAL): key k is visible to query q iff k <= q, both counted inside the sequence;
  P[q][k] = softmax_{k <= q}(q . k / sqrt(dh) + pad[k] * -1e9),   lse[q] = the log-sum-exp over the visible keys.
The keys behind q are excluded outright: the additive mask is pad * -1e9 + triu(-inf, 1), handed to attn_dropout_ref.attention,
which takes any additive mask (and the regenerated dropout keep bits).  The backward is autograd's through these lines."""
import numpy as np
import torch

import attn_dropout_ref as ad
from oracle import numpy_ref as nr
from oracle import torch_ref as tr


def causal_neg(S, key_pad=None, dtype=torch.float64):
    """additive mask broadcastable to [B, H, S, S]: -inf above the diagonal, plus pad[k] * -1e9 (key_pad [B, S], 1 = pad)"""
    neg = torch.triu(torch.full((S, S), float('-inf'), dtype=dtype), diagonal=1)[None, None]
    if key_pad is not None:
        neg = neg + key_pad.to(dtype)[:, None, None, :] * -1e9
    return neg


def split_heads(qkv, H, dh):
    """qkv [B, S, 3*H*dh] (q | k | v column blocks) -> q, k, v [B, H, S, dh]"""
    B, S, _ = qkv.shape
    d = H * dh
    return [qkv[..., i * d:(i + 1) * d].reshape(B, S, H, dh).permute(0, 2, 1, 3) for i in range(3)]


def attention_qkv(qkv, H, dh, key_pad=None, keep=None, rate=0.0):
    """qkv [B, S, 3*H*dh] float64, key_pad [B, S] or None, keep [B, H, S, S] or None -> (o [B, S, H*dh], lse [B, H, S])"""
    B, S, _ = qkv.shape
    q, k, v = split_heads(qkv, H, dh)
    o, lse = ad.attention(q, k, v, causal_neg(S, key_pad, qkv.dtype), keep, rate)
    return o.permute(0, 2, 1, 3).reshape(B, S, H * dh), lse


def weights(qkv, H, dh, key_pad=None):
    """the undropped P [B, H, S, S] (exactly 0 above the diagonal: exp(-inf))"""
    B, S, _ = qkv.shape
    q, k, _ = split_heads(qkv, H, dh)
    logits = q @ k.transpose(-1, -2) / float(np.sqrt(np.float32(dh))) + causal_neg(S, key_pad, qkv.dtype)
    return torch.softmax(logits, -1)


def attention_grads(qkv, do, lens, H, dh, pad=None, keep=None, rate=0.0):
    """sequences of the lengths `lens` stored one after the other (the dense layout: all lengths equal): qkv [T, 3*H*dh],
    do [T, H*dh] (any dtype; taken to float64 as they are), pad [T] key bytes or None, keep [B, H, S_arg, S_arg] or None
    -> (o [T, H*dh], [lse [H, L] per sequence], d qkv [T, 3*H*dh]) in float64"""
    off = np.concatenate([[0], np.cumsum(lens)])
    q64 = qkv.double().cpu().requires_grad_(True)
    outs, lses = [], []
    for b, L in enumerate(lens):
        kp = None if pad is None else pad[off[b]:off[b] + L][None].cpu()
        kb = None if keep is None else keep[b:b + 1, :, :L, :L]
        o, lse = attention_qkv(q64[off[b]:off[b] + L][None], H, dh, kp, kb, rate)
        outs.append(o[0])
        lses.append(lse[0].detach())
    o = torch.cat(outs)
    o.backward(do.double().cpu())
    return o.detach(), lses, q64.grad


def encoder_forward(x, key_pad, P, num_layers, num_heads, rate=0.0, attn_rate=0.0, keep_res=None, keep_attn=None, relu=tr._relu,
                    prefix='enc_layers.'):
    """attn_dropout_ref.encoder_forward's post-LN stack on x [B, S, d] float64 with the causal mask; relu(name, z) as
    oracle/torch_ref.transformer_forward takes it ('ffn.<layer>')"""
    B, S, d = x.shape
    depth = d // num_heads
    neg = causal_neg(S, key_pad, x.dtype)
    keep_res = keep_res or {}
    for i in range(num_layers):
        pre = '%s%d.' % (prefix, i)

        def lin(t, name):
            return t @ P[pre + name + '.kernel'] + P[pre + name + '.bias']

        def split(t):
            return t.reshape(B, S, num_heads, depth).permute(0, 2, 1, 3)
        o, _ = ad.attention(split(lin(x, 'mha.wq')), split(lin(x, 'mha.wk')), split(lin(x, 'mha.wv')), neg,
                            keep_attn[i] if keep_attn else None, attn_rate)
        o = o.permute(0, 2, 1, 3).reshape(B, S, d)
        attn = tr.dropout(lin(o, 'mha.dense'), rate, keep_res.get('l%d.1' % i))
        out1 = tr.layer_norm(x + attn, P[pre + 'layernorm1.gamma'], P[pre + 'layernorm1.beta'], nr.LN_EPS)
        f = tr.dropout(lin(relu('ffn.%d' % i, lin(out1, 'ffn.0')), 'ffn.1'), rate, keep_res.get('l%d.2' % i))
        x = tr.layer_norm(out1 + f, P[pre + 'layernorm2.gamma'], P[pre + 'layernorm2.beta'], nr.LN_EPS)
    return x


def model_encode(ids, P, num_layers, num_heads, rate=0.0, attn_rate=0.0, keep=None, keep_attn=None, relu=tr._relu,
                 feature='items'):
    """oracle/torch_ref.transformer_forward's input stage (table rows * sqrt(d) + sinusoid, dropout keep['emb']) and the causal
    stack above.  P: the model's state dict in float64 ('transformer.' names)."""
    keep = keep or {}
    x = P['transformer.embedding_layers.%s.weight' % feature][ids]
    B, S, d = x.shape
    x = x * float(np.sqrt(np.float32(d))) + tr.positional_encoding(S, d, x.dtype)[None]
    x = tr.dropout(x, rate, keep.get('emb'))
    return encoder_forward(x, (ids == nr.INPUT_PAD), P, num_layers, num_heads, rate, attn_rate, keep, keep_attn, relu,
                           prefix='transformer.encoder.enc_layers.')


def model_loss(ids, flat_idx, labels, P, num_layers, num_heads, n_hidden, relu=tr._relu, **kw):
    """cloze_loss of a causal model: the rows flat_idx (long, positions b*S + s) of the causal encoder's output -> the softmax
    head -> the mean TF sparse cross-entropy against `labels` (long, label space)"""
    enc = model_encode(ids, P, num_layers, num_heads, relu=relu, **kw)
    rows = enc.reshape(-1, enc.shape[-1])[flat_idx]
    hP = {k[len('head.'):]: v for k, v in P.items() if k.startswith('head.')}
    probs = torch.softmax(tr.softmax_head_logits(rows, hP, n_hidden, relu=relu), -1)
    return tr.sparse_ce_tf(probs, labels).sum() / labels.numel(), enc
