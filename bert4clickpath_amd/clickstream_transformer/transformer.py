"""Encoder stack, MI355X-native.  Same names and call contracts as the reference's
clickstream_transformer/transformer.py (Transformer, Encoder, EncoderLayer, MultiHeadAttention,
point_wise_feed_forward_network, positional_encoding, create_padding_mask,
scaled_dot_product_attention); the bodies launch the HIP kernels of libb4c_hip.so.

State-dict names mirror the Keras variable tree: ``encoder.enc_layers.<i>.mha.{wq,wk,wv,dense}.{kernel,bias}``,
``...ffn.{0,1}.{kernel,bias}``, ``...layernorm{1,2}.{gamma,beta}``, ``embedding_layers.<feature>.weight``;
dense kernels are stored [in, out] like Keras.

Build constraints of the HIP path: every feature's embedding dim % 8 == 0, head depth in
{16, 32, 64, 128}, sequence tensors are int64 on the HIP device.
"""
import math
import numbers

import numpy as np
import torch
from torch import nn

from .. import ops
from .._lib import B4CError
from .constants import INPUT_PAD, SEP

_MASK64 = (1 << 64) - 1


class _SeedStream:
    """Per-call dropout seeds: splitmix64 over (base, counter)."""

    def __init__(self, base=0x5EEDB4C):
        self.base, self.counter = base, 0

    def reseed(self, base):
        self.base, self.counter = int(base) & _MASK64, 0

    def next(self):
        self.counter += 1
        z = (self.base + self.counter * 0x9E3779B97F4A7C15) & _MASK64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
        return z ^ (z >> 31)


dropout_seeds = _SeedStream()


def set_dropout_seed(seed):
    dropout_seeds.reseed(seed)


def _attention_rate(rate):
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError('attention_dropout_rate must lie in [0, 1), got %r' % (rate,))
    return rate


ATTENTION_KINDS = ('bidirectional', 'causal')


def _attention_kind(attention):
    if attention not in ATTENTION_KINDS:
        raise ValueError("attention must be 'bidirectional' or 'causal', got %r" % (attention,))
    return attention


NORM_KINDS = ('post', 'pre')


def _norm_kind(norm):
    if norm not in NORM_KINDS:
        raise ValueError("norm must be 'post' or 'pre', got %r" % (norm,))
    return norm


def create_segment_markers(seq, sep=SEP):
    """Cumulative count of SEP tokens along axis 1 (reference transformer.py:6-34; unused on the hot path)."""
    return torch.cumsum((seq == sep).to(torch.int32), dim=1)


def create_padding_mask(seq):
    """float32 (B,1,1,S) mask, 1 where the id is the pad id (reference transformer.py:38-41).
    The hot path carries the same information as one byte per token from the embedding kernel."""
    return (seq == INPUT_PAD).to(torch.float32)[:, None, None, :]


def create_look_ahead_mask(size):
    """float32 (size, size) mask, 1 above the diagonal: position q may not look at the positions after q (the reference family's
    helper; the reference's scaled_dot_product_attention documents the mask kind, its encoder never builds one).  The kernels
    never read such a matrix: `causal=True` / attention='causal' is this mask."""
    return torch.triu(torch.ones(size, size, dtype=torch.float32), diagonal=1)


_pe_cache = {}


def positional_encoding(position, d_model):
    """Fixed sinusoidal table (1, position, d_model), float32; angles in float64 exactly as the
    reference builds them (transformer.py:44-61): sin on even columns, cos on odd columns."""
    key = (position, d_model)
    if key not in _pe_cache:
        pos = np.arange(position, dtype=np.float64)[:, None]
        i = np.arange(d_model, dtype=np.int64)[None, :]
        ang = pos / np.power(10000.0, (2 * (i // 2)).astype(np.float64) / np.float64(np.float32(d_model)))
        ang[:, 0::2] = np.sin(ang[:, 0::2])
        ang[:, 1::2] = np.cos(ang[:, 1::2])
        _pe_cache[key] = torch.from_numpy(ang.astype(np.float32))[None]
    return _pe_cache[key]


def _mask_to_bytes(mask, B, S, device):
    """Accepts the reference's (B,1,1,S) float mask or a (B,S) byte/bool mask; None = no padding."""
    if mask is None:
        return ops.zeros(B, S, dtype=torch.uint8, device=device)
    m = mask.reshape(B, S)
    return (m != 0).to(torch.uint8).contiguous()


def _key_mask_bytes(mask, B, Sk, device):
    """Key-side padding masks only: the reference's (B,1,1,Sk) float mask, a (B,Sk) byte / bool / float mask, or None.
    (The reference's function also accepts any mask broadcastable to (..., Sq, Sk); the encoder never builds one.)"""
    if mask is None:
        return ops.zeros(B, Sk, dtype=torch.uint8, device=device)
    if mask.numel() != B * Sk:
        raise B4CError('MI355X build: attention masks are key-side padding masks of %d x %d elements, got shape %s; '
                       'a look-ahead mask is the argument causal=True (with the padding mask as `mask`), other (Sq, Sk) masks '
                       'are not supported' % (B, Sk, tuple(mask.shape)))
    return (mask.reshape(B, Sk) != 0).to(torch.uint8).contiguous()


def _pad_rows(x, S):
    """(B, s, d) -> (B, S, d), zero rows appended."""
    if x.shape[1] == S:
        return x
    return torch.nn.functional.pad(x, (0, 0, 0, S - x.shape[1]))


def _causal_kw(causal, Sq, Sk):
    """keywords of a causal launch ({} for a bidirectional one: the calls it has always made)"""
    if not causal:
        return {}
    if Sq != Sk:
        raise ValueError('causal attention needs queries and keys of one length (Sq = %d, Sk = %d)' % (Sq, Sk))
    return {'causal': True}


def scaled_dot_product_attention(q, k, v, mask=None, return_weights=False, causal=False):
    """q: (B, H, Sq, depth), k / v: (B, H, Sk, depth) on the HIP device -> (output (B,H,Sq,depth), weights).
    The attention-weight matrix (B,H,Sq,Sk) is materialised only with return_weights=True (the reference returns it
    and its only caller discards it, transformer.py:203); otherwise the second result is None.
    mask: the key-side padding mask.  causal=True is the reference's look-ahead mask (create_look_ahead_mask(Sq)) on top of it:
    query q sees keys 0 .. q only (Sq == Sk, otherwise ValueError); the returned weights are zero above the diagonal."""
    ckw = _causal_kw(causal, q.shape[2], k.shape[2])
    ops._cuda(q, k, v)
    B, H, Sq, dh = q.shape
    Sk = k.shape[2]
    S = max(Sq, Sk)
    key_pad = _key_mask_bytes(mask, B, Sk, q.device)
    if Sk < S:
        key_pad = torch.nn.functional.pad(key_pad, (0, S - Sk), value=1)
    pack = torch.cat([_pad_rows(t.permute(0, 2, 1, 3).reshape(B, -1, H * dh), S).reshape(B * S, H * dh) for t in (q, k, v)],
                     dim=1).contiguous()
    o, lse = ops.attn_fwd(pack, key_pad, B, S, H, dh, **ckw)
    w = ops.attn_weights(pack, key_pad, lse, B, S, H, dh, **ckw)[:, :, :Sq, :Sk] if return_weights else None
    return o.view(B, S, H, dh)[:, :Sq].permute(0, 2, 1, 3), w


class Dense(nn.Module):
    """Keras-style Dense parameters: kernel [in, units] (glorot uniform), bias zeros."""

    def __init__(self, in_dim, units):
        super().__init__()
        lim = math.sqrt(6.0 / (in_dim + units))
        self.kernel = nn.Parameter(torch.empty(in_dim, units).uniform_(-lim, lim))
        self.bias = nn.Parameter(torch.zeros(units))
        self.in_dim, self.units = in_dim, units


class LayerNormalization(nn.Module):
    def __init__(self, d, epsilon=1e-6):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(d))
        self.beta = nn.Parameter(torch.zeros(d))
        self.epsilon = epsilon


class MultiHeadAttention(nn.Module):
    def __init__(self, d_model, num_heads, **kwargs):
        super().__init__()
        assert d_model % num_heads == 0
        self.num_heads, self.d_model = num_heads, d_model
        self.depth = d_model // num_heads
        self.wq, self.wk, self.wv = Dense(d_model, d_model), Dense(d_model, d_model), Dense(d_model, d_model)
        self.dense = Dense(d_model, d_model)
        self._pk_qkv = ops.PackedLinear([self.wq.kernel, self.wk.kernel, self.wv.kernel],
                                        [self.wq.bias, self.wk.bias, self.wv.bias])
        self._pk_o = ops.PackedLinear([self.dense.kernel], [self.dense.bias])

    def get_config(self):
        return {'d_model': self.d_model, 'num_heads': self.num_heads}

    def forward(self, v, k, q, mask, return_weights=False, causal=False):
        """call(v, k, q, mask) of the reference (:137-160): q (B, Sq, d), k / v (B, Sk, d), key-side padding mask
        ((B,1,1,Sk) float, 1 = pad, or (B,Sk) bytes) -> (output (B, Sq, d), attention weights (B, H, Sq, Sk) or None).
        Differentiable; the weights are materialised only on request (the encoder discards them, :203).
        Sequences of different length are padded to the longer one (pad keys masked, pad queries dropped).
        causal=True: the look-ahead mask on top of the padding mask (Sq == Sk, otherwise ValueError); the weights are zero above
        the diagonal."""
        ckw = _causal_kw(causal, q.shape[1], k.shape[1])
        ops._cuda(v, k, q)
        B, Sq, d = q.shape
        Sk = k.shape[1]
        if v.shape[1] != Sk:
            raise ValueError('k and v must have the same length (%d vs %d)' % (Sk, v.shape[1]))
        S = max(Sq, Sk)
        same = (v is k and k is q)
        key_pad = _key_mask_bytes(mask, B, Sk, q.device)
        if Sk < S:
            key_pad = torch.nn.functional.pad(key_pad, (0, S - Sk), value=1)
        xq = _pad_rows(q, S).reshape(B * S, d)
        xk = xq if same else _pad_rows(k, S).reshape(B * S, d)
        xv = xq if same else (xk if v is k else _pad_rows(v, S).reshape(B * S, d))
        out, w = ops.MHAFn.apply(xq, xk, xv, key_pad, self.wq.kernel, self.wq.bias, self.wk.kernel, self.wk.bias,
                                 self.wv.kernel, self.wv.bias, self.dense.kernel, self.dense.bias, self._pk_qkv, self._pk_o,
                                 B, S, self.num_heads, same, bool(return_weights), *([True] if ckw else []))
        out = out.view(B, S, d)[:, :Sq]
        return out, (w[:, :, :Sq, :Sk] if return_weights else None)


class _FeedForward(nn.ModuleList):
    """Two Dense layers addressed as ffn[0] / ffn[1] (state-dict keys ``ffn.0.*`` / ``ffn.1.*``) like the
    reference's keras.Sequential (transformer.py:163-167)."""

    def __init__(self, d_model, dff, ffn_activation='relu'):
        super().__init__([Dense(d_model, dff), Dense(dff, d_model)])
        # 'relu' (the reference) | 'gelu' (x Phi(x), erf) | 'gelu_tanh' (the BERT4Rec code's form): no reference counterpart
        self.act = ops.ffn_act_code(ffn_activation)
        self.ffn_activation = ffn_activation
        self._pk1 = ops.PackedLinear([self[0].kernel], [self[0].bias])
        self._pk2 = ops.PackedLinear([self[1].kernel], [self[1].bias])

    def forward(self, x):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        wt1, _, b1 = self._pk1.get(x2.dtype, shp[-1], False)
        wt2, _, b2 = self._pk2.get(x2.dtype, self._pk1.Np, False)
        with torch.no_grad():
            h = ops.gemm_nt(x2, wt1, self._pk1.Np, b1, act=self.act)
            y = ops.gemm_nt(h, wt2, shp[-1], b2)
        return y.view(shp)


def point_wise_feed_forward_network(d_model, dff, ffn_activation='relu'):
    return _FeedForward(d_model, dff, ffn_activation)


class EncoderLayer(nn.Module):
    """Post-LN block: out1 = LN1(x + drop(mha(x))); out2 = LN2(out1 + drop(ffn(out1))) (reference :202-213).
    Runs as two fused autograd blocks of HIP kernels.
    attention_dropout_rate (BERT's attention_probs_dropout_prob; no reference counterpart): dropout on the attention
    probabilities inside the attention kernels, in training only.  Its seed is a THIRD draw from dropout_seeds, taken after the
    two of the residual branches and only when the rate is > 0: at rate 0 the seed stream is what it always was.
    attention ('bidirectional' | 'causal'; no reference counterpart): 'causal' is left-to-right self-attention inside the kernels,
    position q attends to positions 0 .. q only (the position in the dense layout, the row inside the sequence in the packed one).
    norm ('post' | 'pre'; no reference counterpart): 'pre' is the pre-LN block, torch's norm_first layer -- x' = x + drop(mha(LN1(x))),
    x'' = x' + drop(ffn(LN2(x'))): q, k and v are all taken from the normalised rows, the layer returns the UN-normalised stream and
    the norm that ends a stack belongs to Encoder (final_norm).  Same parameters, names and dropout seeds as the post-LN layer; no
    masked-query form (rows=)."""

    def __init__(self, d_model, num_heads, dff, rate=0.1, ffn_activation='relu', attention_dropout_rate=0.0,
                 attention='bidirectional', norm='post', **kwargs):
        super().__init__()
        self.d_model, self.num_heads, self.dff, self.rate = d_model, num_heads, dff, rate
        self.ffn_activation = ffn_activation
        self.attention = _attention_kind(attention)
        self.norm = _norm_kind(norm)
        self.attention_dropout_rate = _attention_rate(attention_dropout_rate)
        self.mha = MultiHeadAttention(d_model, num_heads)
        self.ffn = point_wise_feed_forward_network(d_model, dff, ffn_activation)
        self.layernorm1 = LayerNormalization(d_model, 1e-6)
        self.layernorm2 = LayerNormalization(d_model, 1e-6)

    def get_config(self):
        return {'d_model': self.d_model, 'num_heads': self.num_heads, 'dff': self.dff, 'rate': self.rate,
                **({'ffn_activation': self.ffn_activation} if self.ffn_activation != 'relu' else {}),
                **({'attention_dropout_rate': self.attention_dropout_rate} if self.attention_dropout_rate else {}),
                **({'attention': self.attention} if self.attention != 'bidirectional' else {}),
                **({'norm': self.norm} if self.norm != 'post' else {})}

    def pre_ln_halves(self, x2, n, stats, key_pad, B, S, cu, training, next_norm):
        """The two pre-LN halves on the stream x2 [T, d] with n = LN1(x2) and its stats given -> (x'', LN(x''; next_norm), its
        stats): each tail writes the stream and the NEXT norm's rows in one launch (ops.PreLNAttnBlockFn / PreLNFFNBlockFn)."""
        m, f = self.mha, self.ffn
        s1 = dropout_seeds.next() if training else 0
        s2 = dropout_seeds.next() if training else 0
        a_rate = self.attention_dropout_rate if training else 0.0
        s3 = dropout_seeds.next() if a_rate > 0 else 0
        need_tape = training or torch.is_grad_enabled()
        rate = self.rate if training else 0.0
        x1, n1, st1 = ops.PreLNAttnBlockFn.apply(x2, m.wq.kernel, m.wq.bias, m.wk.kernel, m.wk.bias, m.wv.kernel, m.wv.bias,
                                                 m.dense.kernel, m.dense.bias, self.layernorm1.gamma, self.layernorm1.beta, n, stats,
                                                 key_pad, self.layernorm2.gamma, self.layernorm2.beta, m._pk_qkv, m._pk_o, B, S,
                                                 self.num_heads, rate, s1, need_tape, cu, a_rate, s3,
                                                 *([True] if self.attention == 'causal' else []))
        return ops.PreLNFFNBlockFn.apply(x1, f[0].kernel, f[0].bias, f[1].kernel, f[1].bias, self.layernorm2.gamma,
                                         self.layernorm2.beta, n1, st1, next_norm.gamma, next_norm.beta, f._pk1, f._pk2, rate, s2,
                                         need_tape, f.act)

    def forward(self, x, training=None, mask=None, packed=None, rows=None):
        """x (B, S, d); or, with `packed` (ops.Packed), the (1, T, d) rows of the real tokens only and mask = the (T,) key
        bytes the embedding stage produced for them.
        rows = (midx [R] int32 token rows, moff [B+1] int32 per-sequence offsets into them): the layer is evaluated for
        those query rows only (keys / values from every token) and returns (R, d) -- the last layer of the Cloze path.
        In training with attention_dropout_rate > 0 that takes ops.mq_attn_dropout (off by default: B4CError); the masked-query
        kernels then draw, with the layer's third seed, the masks the full layer draws for those rows.
        On a causal layer it takes ops.mq_causal (off by default: B4CError): each query row then attends to the keys up to its own
        position, as the full causal layer does at that row."""
        B, S, d = x.shape
        training = bool(training)
        cu = None
        if packed is not None:
            key_pad, cu = mask, packed.cu
            x2 = x.reshape(-1, d)
            out_shape = x.shape
            B, S = packed.B, packed.max_len
        else:
            key_pad = mask if (mask is not None and mask.dtype == torch.uint8 and mask.dim() == 2) else \
                _mask_to_bytes(mask, B, S, x.device)
            x2 = x.reshape(B * S, d)
            out_shape = (B, S, d)
        if self.norm == 'pre':
            if rows is not None:
                raise B4CError('a pre-LN layer has no masked-query form (rows=): evaluate the full layer and gather its rows '
                               '(Encoder.rows_supported / rows_route answer False)')
            # a layer on its own: LN1 is launched here, and the last tail's norm output (no next norm to feed) is dropped
            n, stats = ops.layernorm_fwd(x2, self.layernorm1.gamma.detach(), self.layernorm1.beta.detach())
            return self.pre_ln_halves(x2, n, stats, key_pad, B, S, cu, training, self.layernorm1)[0].view(out_shape)
        m, f = self.mha, self.ffn
        s1 = dropout_seeds.next() if training else 0
        s2 = dropout_seeds.next() if training else 0
        a_rate = self.attention_dropout_rate if training else 0.0
        s3 = dropout_seeds.next() if a_rate > 0 else 0
        need_tape = training or torch.is_grad_enabled()
        if rows is not None:
            if self.attention == 'causal' and not ops.mq_causal:
                raise B4CError('the masked-query last layer (rows=) of a causal encoder needs ops.mq_causal (B4C_MQ_CAUSAL=1; off by '
                               'default): evaluate the full layer of a causal encoder and gather its rows '
                               '(Encoder.rows_supported(dtype, training), Encoder.rows_route)')
            if a_rate > 0 and not ops.mq_attn_dropout:
                raise B4CError('the masked-query last layer (rows=) has no attention dropout: evaluate the full layer while '
                               'training with attention_dropout_rate > 0 (Encoder.rows_supported(dtype, training))')
            midx, moff = rows
            if cu is None:          # dense layout: sequence b owns token rows b*S .. (b+1)*S, pad keys are masked by their bytes
                cu = torch.arange(B + 1, dtype=torch.int32, device=x.device) * S
                kp = key_pad.reshape(-1)
            else:
                kp = None           # packed layout: every token is real
            out1 = ops.MQAttnBlockFn.apply(x2, midx, moff, cu, kp, m.wq.kernel, m.wq.bias, m.wk.kernel, m.wk.bias, m.wv.kernel,
                                           m.wv.bias, m.dense.kernel, m.dense.bias, self.layernorm1.gamma, self.layernorm1.beta,
                                           m._pk_qkv, m._pk_o, B, S, self.num_heads, self.rate if training else 0.0, s1, need_tape,
                                           a_rate, s3, *([True] if self.attention == 'causal' else []))
        else:
            out1 = ops.AttnBlockFn.apply(x2, key_pad, m.wq.kernel, m.wq.bias, m.wk.kernel, m.wk.bias, m.wv.kernel, m.wv.bias,
                                         m.dense.kernel, m.dense.bias, self.layernorm1.gamma, self.layernorm1.beta,
                                         m._pk_qkv, m._pk_o, B, S, self.num_heads, self.rate if training else 0.0, s1, need_tape, cu,
                                         a_rate, s3, *([True] if self.attention == 'causal' else []))
        out2 = ops.FFNBlockFn.apply(out1, f[0].kernel, f[0].bias, f[1].kernel, f[1].bias, self.layernorm2.gamma,
                                    self.layernorm2.beta, f._pk1, f._pk2, self.rate if training else 0.0, s2, need_tape, f.act)
        return out2 if rows is not None else out2.view(out_shape)      # rows: (R, d) as the blocks leave it


class Encoder(nn.Module):
    """num_layers EncoderLayers; no final LayerNorm (reference :255-268).  The input dropout of the
    reference's Encoder.call (:263) is fused into the embedding kernel when ``Transformer`` calls the Encoder;
    an Encoder called on its own applies it with the stand-alone dropout kernel (same keep-mask generator).
    norm='pre' (no reference counterpart): pre-LN layers (EncoderLayer) and one LayerNorm after the last of them, ``final_norm``
    (gamma ones, beta zeros, eps 1e-6) -- nn.TransformerEncoder(norm_first layers, norm=LayerNorm).  The full last layer always
    runs: rows= is refused, rows_supported / rows_route answer False."""

    def __init__(self, num_layers, d_model, num_heads, dff, dropout_rate, ffn_activation='relu', attention_dropout_rate=0.0,
                 attention='bidirectional', norm='post', **kwargs):
        super().__init__()
        self.num_layers, self.d_model, self.num_heads, self.dff, self.dropout_rate = \
            num_layers, d_model, num_heads, dff, dropout_rate
        ops.ffn_act_code(ffn_activation)        # (ValueError also for an encoder of no layers)
        self.ffn_activation = ffn_activation
        self.attention_dropout_rate = _attention_rate(attention_dropout_rate)
        self.attention = _attention_kind(attention)
        self.norm = _norm_kind(norm)
        self.enc_layers = nn.ModuleList([EncoderLayer(d_model, num_heads, dff, dropout_rate, ffn_activation,
                                                      self.attention_dropout_rate, self.attention,
                                                      **({'norm': 'pre'} if self.norm == 'pre' else {})) for _ in range(num_layers)])
        if self.norm == 'pre':
            self.final_norm = LayerNormalization(d_model, 1e-6)

    def get_config(self):
        return {'num_layers': self.num_layers, 'd_model': self.d_model, 'num_heads': self.num_heads, 'dff': self.dff,
                'dropout_rate': self.dropout_rate,
                **({'ffn_activation': self.ffn_activation} if self.ffn_activation != 'relu' else {}),
                **({'attention_dropout_rate': self.attention_dropout_rate} if self.attention_dropout_rate else {}),
                **({'attention': self.attention} if self.attention != 'bidirectional' else {}),
                **({'norm': self.norm} if self.norm != 'post' else {})}

    def _forward_pre(self, x, training, mask, packed):
        """The pre-LN stack: one layernorm_fwd (LN1 of the first layer), then every half's tail writes the stream and the next
        norm's rows; the last tail is given final_norm, whose rows are the encoder's output."""
        B, S, d = x.shape
        if packed is not None:
            key_pad, cu = mask, packed.cu
            x2 = x.reshape(-1, d)
            B, S = packed.B, packed.max_len
        else:
            key_pad = mask if (mask is not None and mask.dtype == torch.uint8 and mask.dim() == 2) else \
                _mask_to_bytes(mask, B, S, x.device)
            cu = None
            x2 = x.reshape(B * S, d)
        norms = [layer.layernorm1 for layer in self.enc_layers] + [self.final_norm]
        n, stats = ops.layernorm_fwd(x2, norms[0].gamma.detach(), norms[0].beta.detach())
        for i, layer in enumerate(self.enc_layers):
            x2, n, stats = layer.pre_ln_halves(x2, n, stats, key_pad, B, S, cu, bool(training), norms[i + 1])
        out = ops.PreLNFinalNormFn.apply(x2, self.final_norm.gamma, self.final_norm.beta, n, stats,
                                         bool(training) or torch.is_grad_enabled())
        return out.view(x.shape)

    def forward(self, inputs, training=None, mask=None, _input_dropout_done=False, packed=None, rows=None):
        """rows (see EncoderLayer.forward): the LAST layer is evaluated for those query rows only; returns (R, d)."""
        x = inputs
        if training and self.dropout_rate > 0 and not _input_dropout_done:
            x = ops.DropoutFn.apply(x, float(self.dropout_rate), dropout_seeds.next())
        if self.norm == 'pre':
            if rows is not None:
                raise B4CError('a pre-LN encoder has no masked-query last layer (rows=): rows_supported / rows_route answer False, '
                               'evaluate the full encoder and gather its rows')
            return self._forward_pre(x, training, mask, packed)
        B, S, d = x.shape
        last = len(self.enc_layers) - 1
        for i, layer in enumerate(self.enc_layers):
            x = layer(x, training, mask, packed, rows if i == last else None)
        return x

    def rows_supported(self, x_dtype, training=False):
        """The masked-query form of the last layer: head depth 32 / 64 (b4c_attn_mq_*), at least one layer.  Those kernels have no
        attention dropout: a training pass with attention_dropout_rate > 0 takes the full last layer and gathers its rows.  A causal
        encoder takes the full last layer too: the kernels' causal form (b4c_attn_mq_*_ex) is behind a switch that is off by
        default and that rows_route applies (ops.mq_causal), so this answer stays False for it.  A pre-LN encoder: False (the
        masked-query kernels' tail is the post-LN one)."""
        if self.norm == 'pre':
            return False
        if not self.enc_layers or self.attention == 'causal' or (training and self.attention_dropout_rate > 0):
            return False
        return (self.d_model // self.num_heads) in (32, 64) and self.d_model % 8 == 0

    def rows_route(self, x_dtype, training=False):
        """Does the last layer take its masked-query form in this pass?  rows_supported(...); with ops.mq_attn_dropout on, the same
        shape conditions without the dropout exclusion (b4c_attn_mq_*_drop draws the full layer's masks for the query rows).
        A causal encoder: False, as rows_supported says, unless ops.mq_causal is on; then the shape conditions (b4c_attn_mq_*_ex with
        B4C_ATTN_CAUSAL), and in a training pass with attention_dropout_rate > 0 ops.mq_attn_dropout on top, as above.
        A pre-LN encoder: False whatever the switches say."""
        if self.norm == 'pre':
            return False
        if self.attention == 'causal':
            if not ops.mq_causal or not self.enc_layers or (training and self.attention_dropout_rate > 0 and not ops.mq_attn_dropout):
                return False
            return (self.d_model // self.num_heads) in (32, 64) and self.d_model % 8 == 0
        if ops.mq_attn_dropout:
            return self.rows_supported(x_dtype, False)
        return self.rows_supported(x_dtype, training)


class _Embedding(nn.Module):
    """Keras Embedding parameters: weight (rows, dim) ~ U(-0.05, 0.05)."""

    def __init__(self, rows, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(rows, dim).uniform_(-0.05, 0.05))


class _PositionEmbedding(nn.Module):
    """Learned positional table: weight (max_positions, d_model) ~ N(0, 0.02^2) cut at two sigma."""

    def __init__(self, rows, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.nn.init.trunc_normal_(torch.empty(rows, dim), mean=0.0, std=0.02, a=-0.04, b=0.04))


class _FeatureModules(nn.Module):
    """name -> module container whose keys may be ANY feature name ('items', 'keys', ...), which
    nn.ModuleDict refuses; state-dict keys stay ``embedding_layers.<feature>.weight``."""

    def __init__(self, modules):
        super().__init__()
        for k, m in modules.items():
            self._modules[str(k)] = m

    def __getitem__(self, k):
        return self._modules[k]

    def keys(self):
        return self._modules.keys()


class Transformer(nn.Module):
    """Encoder-only Transformer over one or more categorical sequence features (reference :271-402):
    per-feature embedding -> concat on the last axis (or, feature_combine='sum', added) -> * sqrt(d_model) -> + sinusoidal
    PE -> Encoder.
    Extensions of the BERT4Rec paper, no reference counterpart: ffn_activation ('relu' | 'gelu' | 'gelu_tanh') for the
    feed-forward blocks, position_encoding='learned' with max_positions: the positional table is a parameter
    ``position_embedding.weight`` [max_positions, d_model] (truncated normal, sigma 0.02) instead of the fixed sinusoid, and
    attention_dropout_rate: dropout on the attention probabilities (BERT's attention_probs_dropout_prob), in training only;
    embedding_layernorm=True: the input stage is drop(LayerNorm(scale * rows + PE)) with the parameters
    ``embedding_norm.gamma`` / ``.beta`` (eps 1e-6, as every LayerNormalization here); embedding_scale: a positive number in
    place of sqrt(d_model) (None; the paper does not scale: 1.0); attention='causal': left-to-right self-attention in every layer
    (SASRec, the paper's unidirectional arm) instead of 'bidirectional'; norm='pre': pre-LN encoder layers and the encoder's
    ``encoder.final_norm`` behind the last of them (Encoder) instead of the reference's post-LN layers."""

    def __init__(self, num_layers, num_attention_heads, embedding_sizes, embedding_dims, encoder_ff_dim, dropout_rate,
                 item_embedding_weights=None, compute_dtype=torch.float32, feature_combine='concat', ffn_activation='relu',
                 position_encoding='sinusoidal', max_positions=None, attention_dropout_rate=0.0, embedding_layernorm=False,
                 embedding_scale=None, attention='bidirectional', norm='post', **kwargs):
        super().__init__()
        self.attention = _attention_kind(attention)
        self.norm = _norm_kind(norm)
        if embedding_scale is not None and not (isinstance(embedding_scale, numbers.Real) and not isinstance(embedding_scale, bool)
                                                and 0 < float(embedding_scale) < float('inf')):
            raise ValueError('embedding_scale must be None (sqrt(d_model)) or a positive number, got %r' % (embedding_scale,))
        self.embedding_layernorm = bool(embedding_layernorm)
        self.embedding_scale = None if embedding_scale is None else float(embedding_scale)
        ops.ffn_act_code(ffn_activation)
        self.attention_dropout_rate = _attention_rate(attention_dropout_rate)
        if position_encoding not in ('sinusoidal', 'learned'):
            raise ValueError("position_encoding must be 'sinusoidal' or 'learned', got %r" % (position_encoding,))
        if position_encoding == 'learned' and (max_positions is None or int(max_positions) < 1):
            raise ValueError("position_encoding='learned' needs max_positions (a positive table length), got %r" % (max_positions,))
        self.ffn_activation, self.position_encoding = ffn_activation, position_encoding
        self.max_positions = int(max_positions) if position_encoding == 'learned' else None
        assert set(embedding_sizes.keys()) == set(embedding_dims.keys()), \
            "embedding_sizes and embedding_dims must have the same set of keys."
        self.num_layers, self.num_attention_heads = num_layers, num_attention_heads
        self.embedding_sizes, self.embedding_dims = dict(embedding_sizes), dict(embedding_dims)
        self.encoder_ff_dim, self.dropout_rate = encoder_ff_dim, dropout_rate
        self.item_embedding_weights = item_embedding_weights
        self.maximum_position_encoding = 10000
        # feature_combine='sum' (no reference counterpart; the reference concatenates, :384-388): two or more features of ONE
        # width whose embedding rows are added -- d_model is that width
        if feature_combine not in ('concat', 'sum'):
            raise ValueError("feature_combine must be 'concat' or 'sum', got %r" % (feature_combine,))
        self.feature_combine = feature_combine
        if feature_combine == 'sum':
            widths = set(int(v) for v in embedding_dims.values())
            if len(embedding_dims) < 2 or len(widths) != 1:
                raise ValueError("feature_combine='sum' needs two or more features with one embedding dim, got %r" % (dict(embedding_dims),))
            self.d_model = widths.pop()
        else:
            self.d_model = sum(embedding_dims.values())
        for f, dim in embedding_dims.items():
            if dim % 8 != 0:
                raise B4CError('MI355X build: embedding dim of feature %r is %d; must be a multiple of 8' % (f, dim))
        self.compute_dtype = compute_dtype
        self.encoder = Encoder(num_layers, self.d_model, num_attention_heads, encoder_ff_dim, dropout_rate, ffn_activation,
                               self.attention_dropout_rate, self.attention, **({'norm': 'pre'} if self.norm == 'pre' else {}))
        self.embedding_layers = _FeatureModules({f: _Embedding(int(embedding_sizes[f]), int(embedding_dims[f]))
                                                 for f in embedding_dims.keys()})
        if position_encoding == 'learned':
            # the paper's code: truncated normal, sigma 0.02, cut at 2 sigma; a dense parameter like any other (decayed by AdamW)
            self.maximum_position_encoding = self.max_positions
            self.position_embedding = _PositionEmbedding(self.max_positions, self.d_model)
        else:
            self.register_buffer('pos_encoding', positional_encoding(self.maximum_position_encoding, self.d_model)[0].clone(),
                                 persistent=False)
        self.scale = float(np.sqrt(np.float32(self.d_model)))   # sqrt taken in float32 (reference :390)
        if self.embedding_scale is not None:
            self.scale = self.embedding_scale
        if self.embedding_layernorm:
            if self.d_model > 1024:
                raise B4CError('embedding_layernorm: d_model %d > 1024 (the LayerNorm row kernels)' % self.d_model)
            self.embedding_norm = LayerNormalization(self.d_model, 1e-6)

    def get_config(self):
        return {'num_layers': self.num_layers, 'num_attention_heads': self.num_attention_heads,
                'embedding_sizes': self.embedding_sizes, 'embedding_dims': self.embedding_dims,
                'encoder_ff_dim': self.encoder_ff_dim, 'dropout_rate': self.dropout_rate,
                'item_embedding_weights': self.item_embedding_weights,
                **({'feature_combine': 'sum'} if self.feature_combine == 'sum' else {}),
                **({'ffn_activation': self.ffn_activation} if self.ffn_activation != 'relu' else {}),
                **({'position_encoding': 'learned', 'max_positions': self.max_positions}
                   if self.position_encoding == 'learned' else {}),
                **({'attention_dropout_rate': self.attention_dropout_rate} if self.attention_dropout_rate else {}),
                **({'embedding_layernorm': True} if self.embedding_layernorm else {}),
                **({'embedding_scale': self.embedding_scale} if self.embedding_scale is not None else {}),
                **({'attention': self.attention} if self.attention != 'bidirectional' else {}),
                **({'norm': self.norm} if self.norm != 'post' else {})}

    @property
    def position_table(self):
        """the fp32 positional table the embedding stage adds: the sinusoidal buffer or the learned parameter"""
        return self.position_embedding.weight if self.position_encoding == 'learned' else self.pos_encoding

    def packed_supported(self, S):
        """The padding-free layout runs on the bf16 MFMA attention kernels only (head depth 32 / 64, S <= 512; with ops.long_attn
        on, S <= 2048: the streamed kernels)."""
        dh = self.d_model // self.num_attention_heads
        return self.compute_dtype == torch.bfloat16 and dh in (32, 64) and S <= (ops.ATTN_LONG_MAX_S if ops.long_attn else 512)

    def forward(self, inputs, training=None, mask=None, return_key_pad=False, packed=None, rows=None):
        """inputs: dict feature -> (B,S) int64 ids (first feature defines the padding mask).
        packed (ops.Packed of the first feature's ids): run on the real tokens only -> ((1, T, d) rows, (T,) key bytes).
        rows (midx, moff): only those rows of the last layer's output are computed and returned, as (R, d)."""
        feats = list(inputs.keys())
        if set(feats) != set(self.embedding_dims.keys()):
            raise KeyError('Transformer inputs %s do not match embedded features %s' % (feats, list(self.embedding_dims)))
        training = bool(training)
        ids = [inputs[f].contiguous() for f in feats]
        tables = [self.embedding_layers[f].weight for f in feats]
        B, S = ids[0].shape
        if S > self.maximum_position_encoding:
            raise B4CError('sequence length %d exceeds the positional table (%d)' % (S, self.maximum_position_encoding))
        rate = self.dropout_rate if training else 0.0
        seed = dropout_seeds.next() if training else 0
        if packed is not None and not self.packed_supported(S):
            raise B4CError('packed layout needs bf16, head depth 32 / 64 and S <= %s' % ('%d' % ops.ATTN_LONG_MAX_S if ops.long_attn else '512'))
        # the positional table is a differentiable input when it is the learned parameter (its gradient: b4c_pos_table_bwd); the
        # sinusoidal EmbedFn call is the reference's, EmbedLNFn the paper's input stage
        args = (self.scale, rate, seed, self.compute_dtype, packed, self.feature_combine, len(ids), *ids, *tables)
        if self.embedding_layernorm:
            x, key_pad = ops.EmbedLNFn.apply(self.position_table, self.embedding_norm.gamma, self.embedding_norm.beta, *args)
        else:
            x, key_pad = ops.EmbedFn.apply(self.position_table, *args)
        out = self.encoder(x, training, key_pad, _input_dropout_done=True, packed=packed, rows=rows)
        return (out, key_pad) if return_key_pad else out
