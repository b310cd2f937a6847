"""float64 restatement of attention-probability dropout (an extension: the reference's attention has no dropout, so there is
no oracle under oracle/; this file is the checker, as tests/test_gpu_gelu.py is for GELU).

Semantics (include/b4c.h): with P the masked softmax,  P~[q][k] = keep(b,h,q,k) ? P[q][k] / (1 - rate) : 0,  O = P~ V; the
log-sum-exp is that of P.  The backward is autograd's through these lines.

The keep rule, restated in Python: element e = ((b*H + h) * S_arg + q) * S4 + k of the keep-mask stream of b4c_keep, S4 = S_arg
rounded up to a multiple of 4; q, k count inside the sequence; S_arg is the pitch of the launch (S, or the packed max_len)."""
import numpy as np
import torch

from oracle import numpy_ref as nr
from oracle.torch_ref import dropout, layer_norm
from paper_encoder_ref import act


def elem_index(b, h, q, k, H, S_arg):
    S4 = (S_arg + 3) // 4 * 4
    return ((b * H + h) * S_arg + q) * S4 + k


def keep_mask(ops, seed, B, H, S_arg, rate):
    """bool [B, H, S_arg, S_arg] from the stream of ops.keep_mask (= b4c_keep) and the index rule above"""
    S4 = (S_arg + 3) // 4 * 4
    m = torch.from_numpy(ops.keep_mask(seed, B * H * S_arg * S4, rate))
    return m.view(B, H, S_arg, S4)[..., :S_arg]


def attention(q, k, v, neg, keep, rate):
    """q, k, v [..., S, dh] float64; neg: additive key mask broadcastable to [..., S, S] (pad * -1e9) or None;
    keep: bool [..., S, S] or None -> (O, lse)"""
    logits = q @ k.transpose(-1, -2) / float(np.sqrt(np.float32(q.shape[-1])))
    if neg is not None:
        logits = logits + neg
    p = torch.softmax(logits, dim=-1)
    if keep is not None and rate > 0:
        p = p * keep.to(p.dtype) / (1.0 - rate)
    return p @ v, torch.logsumexp(logits, -1)


def attention_qkv(qkv, H, dh, key_pad, keep, rate):
    """qkv [B, S, 3*H*dh] float64 (q | k | v column blocks, head h = columns h*dh ..), key_pad [B, S] (1 = pad) or None,
    keep [B, H, S, S] -> (o [B, S, H*dh], lse [B, H, S])"""
    B, S, _ = qkv.shape
    d = H * dh
    q, k, v = [qkv[..., i * d:(i + 1) * d].reshape(B, S, H, dh).permute(0, 2, 1, 3) for i in range(3)]
    neg = None if key_pad is None else key_pad.to(qkv.dtype)[:, None, None, :] * -1e9
    o, lse = attention(q, k, v, neg, keep, rate)
    return o.permute(0, 2, 1, 3).reshape(B, S, d), lse


def encoder_forward(x, key_pad, P, num_layers, num_heads, rate, attn_rate, keep_res, keep_attn, activation='relu'):
    """The post-LN encoder stack on x [B, S, d] float64 (the input dropout already applied): oracle/torch_ref.transformer_forward's
    layer lines with the attention dropout added.  P: 'enc_layers.<i>.mha.wq.kernel' ...; keep_res['l<i>.1' | 'l<i>.2'] [B, S, d],
    keep_attn[i] [B, H, S, S]; activation: that of the feed-forward ('relu' | 'gelu' | 'gelu_tanh', paper_encoder_ref.act)."""
    B, S, d = x.shape
    depth = d // num_heads
    neg = key_pad.to(x.dtype)[:, None, None, :] * -1e9
    for i in range(num_layers):
        pre = 'enc_layers.%d.' % i

        def lin(t, name):
            return t @ P[pre + name + '.kernel'] + P[pre + name + '.bias']

        def split(t):
            return t.reshape(B, S, num_heads, depth).permute(0, 2, 1, 3)
        o, _ = attention(split(lin(x, 'mha.wq')), split(lin(x, 'mha.wk')), split(lin(x, 'mha.wv')), neg, keep_attn[i], attn_rate)
        o = o.permute(0, 2, 1, 3).reshape(B, S, d)
        attn = dropout(lin(o, 'mha.dense'), rate, keep_res['l%d.1' % i])
        out1 = layer_norm(x + attn, P[pre + 'layernorm1.gamma'], P[pre + 'layernorm1.beta'], nr.LN_EPS)
        f = dropout(lin(act(activation, lin(out1, 'ffn.0')), 'ffn.1'), rate, keep_res['l%d.2' % i])
        x = layer_norm(out1 + f, P[pre + 'layernorm2.gamma'], P[pre + 'layernorm2.beta'], nr.LN_EPS)
    return x


def attention_grads(qkv, do, key_pad, B, S, H, dh, keep, rate):
    """dense layout: qkv [B*S, 3*H*dh], do [B*S, H*dh] (any dtype; taken to float64 as they are), key_pad [B, S], keep [B, H, S, S] or
    None -> (o [B*S, H*dh], lse [B, H, S], d qkv) in float64, the gradient by autograd through attention_qkv"""
    q64 = qkv.double().cpu().requires_grad_(True)
    o, lse = attention_qkv(q64.view(B, S, -1), H, dh, key_pad, keep, rate)
    o = o.reshape(B * S, H * dh)
    o.backward(do.double().cpu())
    return o.detach(), lse.detach(), q64.grad


# ---- exact mask recovery (tests/test_gpu_attn_dropout_routes.py; shown on this file alone by tests/test_attn_dropout_cpu.py) -----
# q = k = 0 makes P uniform over the real keys of a sequence, so every kept, unpadded probability is the same nonzero number and
# every dropped or padded one is exactly 0.  A one-hot V (dO) then copies a window of dh keys (queries) of P~ into o (dV).
def recovery_passes(S, dh):
    return -(-S // dh)


def recovery_operands(lens, H, dh, p, dtype):
    """pass p over sequences of the lengths `lens`, stored one after the other -> (qkv [T, 3*H*dh], do [T, H*dh]):
    q = k = 0; V row k of a sequence = one-hot at column k - p*dh for p*dh <= k < (p+1)*dh, zero elsewhere; dO row q likewise."""
    d, off = H * dh, np.concatenate([[0], np.cumsum(lens)])
    qkv = torch.zeros(int(off[-1]), 3 * d, dtype=dtype)
    do = torch.zeros(int(off[-1]), d, dtype=dtype)
    for b, L in enumerate(lens):
        i = torch.arange(p * dh, max(p * dh, min((p + 1) * dh, L)))          # (empty: the sequence ends before this window)
        for h in range(H):
            qkv[off[b] + i, 2 * d + h * dh + i - p * dh] = 1.0
            do[off[b] + i, h * dh + i - p * dh] = 1.0
    return qkv, do


def recovery_collect(fwd, bwd, o, dv, lens, H, dh, p):
    """books pass p: fwd[b][h][q][p*dh + c] = (o[q][h][c] != 0), bwd[b][h][p*dh + c][k] = (dV[k][h][c] != 0); fwd, bwd: lists of
    bool [H, L, L] per sequence ([h][query][key]); o, dv: [T, H*dh] on the host.  Columns past the sequence must be zero."""
    off = np.concatenate([[0], np.cumsum(lens)])
    for b, L in enumerate(lens):
        n = max(0, min(dh, L - p * dh))
        ob = (o[off[b]:off[b] + L].reshape(L, H, dh) != 0).permute(1, 0, 2)          # [h][q][c]
        vb = (dv[off[b]:off[b] + L].reshape(L, H, dh) != 0).permute(1, 2, 0)         # [h][c][k]
        assert not ob[:, :, n:].any() and not vb[:, n:, :].any(), ('a column past the window is nonzero', b, p)
        fwd[b][:, :, p * dh:p * dh + n] = ob[:, :, :n]
        bwd[b][:, p * dh:p * dh + n, :] = vb[:, :n, :]


def recovery_pads(B, S):
    """key bytes [B, S] of the recovery cases: sequence 0 pads its last 4 keys, sequence 1 the keys 5 .. S-2 (whole key tiles in the
    middle), as tests/test_gpu_kernels.py::test_attention_fwd_bwd; key 0 always stays real (a sequence without any real key has
    no masked softmax to recover: the kernels and the reference fall back to uniform weights over the pads)."""
    pad = torch.zeros(B, S, dtype=torch.uint8)
    pad[0, max(S - 4, 1):] = 1
    if B > 1:
        pad[1, 5:max(S - 1, 5)] = 1
    return pad
