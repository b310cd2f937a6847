"""float64 restatement of the two paper-faithful encoder extensions -- the GELU feed-forward activation and the learned
positional table -- in torch CPU autograd.  NO REFERENCE ORACLE: the reference has neither (its feed-forward is ReLU, its
positions the fixed sinusoid); this file states what the extensions mean, on top of oracle/torch_ref.py's dataflow.  Used by
test_gpu_gelu.py and test_gpu_learned_positions.py."""
import math

import torch

from oracle import torch_ref as tr

APPROX = {'gelu': 'none', 'gelu_tanh': 'tanh'}


def act(name, z):
    """'relu' | 'gelu' (x Phi(x), erf) | 'gelu_tanh'"""
    if name == 'relu':
        return torch.relu(z)
    return torch.nn.functional.gelu(z, approximate=APPROX[name])


def act_grad(name, u):
    """d act / d u in closed form (float64)"""
    if name == 'relu':
        return (u > 0).to(u.dtype)
    if name == 'gelu':
        return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    k = math.sqrt(2 / math.pi)
    t = torch.tanh(k * (u + 0.044715 * u ** 3))
    return 0.5 * (1 + t) + 0.5 * u * (1 - t * t) * k * (1 + 3 * 0.044715 * u * u)


def ffn_activation(name, relu=tr._relu):
    """the `relu(name, z)` hook of torch_ref.transformer_forward / model_loss: the encoder's feed-forward blocks ('ffn.<i>') take
    the activation `name`; the head's trunk ('head.<i>') keeps ReLU (through `relu`, e.g. a bf16_gates recorder's)"""
    def hook(layer, z):
        return act(name, z) if layer.startswith('ffn.') and name != 'relu' else relu(layer, z)
    return hook


def model_loss(ids, labels_compact, P, num_layers, num_heads, n_hidden, ffn='relu', relu=tr._relu, **kw):
    """torch_ref.model_loss with the feed-forward activation `ffn` and, when P holds 'transformer.position_embedding.weight' (a leaf
    tensor [max_positions, d]), that table in place of the sinusoid: x = drop(table * sqrt(d) + P[s])."""
    table = P.get('transformer.position_embedding.weight')
    orig = tr.positional_encoding
    if table is not None:
        tr.positional_encoding = lambda S, d, dtype=torch.float32: table[:S].to(dtype)
    try:
        return tr.model_loss(ids, labels_compact, P, num_layers, num_heads, n_hidden, relu=ffn_activation(ffn, relu), **kw)
    finally:
        tr.positional_encoding = orig


def pos_table_grad(dout, cu, S, d, keep=None, rate=0.0):
    """dP [S, d] float64 = sum over sequences b longer than s of keep / (1 - rate) * dout[cu[b] + s]   (b4c_pos_table_bwd)"""
    g = dout.double().reshape(-1, d)
    if keep is not None and rate > 0:
        g = g * keep.reshape(-1, d).double() / (1.0 - rate)
    dP = torch.zeros(S, d, dtype=torch.float64)
    for b in range(len(cu) - 1):
        n = min(int(cu[b + 1] - cu[b]), S)
        dP[:n] += g[int(cu[b]):int(cu[b]) + n]
    return dP
