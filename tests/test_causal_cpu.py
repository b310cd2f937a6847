"""Causal (left-to-right) self-attention, the parts that need no GPU (NO REFERENCE ORACLE: an extension -- the float64 restatement
is tests/causal_ref.py): the checker against itself (a causal row is the last row of bidirectional attention over its prefix),
the three entry points and the flag in the C header and its binding, the ABI version, and the `attention=` / `causal=` keywords:
validation, get_config() rules, config and checkpoint round trips, the route of the last layer."""
import os

import numpy as np
import pytest
import torch

import abi_pin
import attn_dropout_ref as ad
import causal_ref as cr


# ---- the checker checks itself --------------------------------------------------------------------------------------------------
def _case(B, S, H, dh, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, 3 * H * dh, generator=g, dtype=torch.float64)
    pad = torch.zeros(B, S, dtype=torch.uint8)
    pad[0, max(S - 4, 1):] = 1                      # the tail of sequence 0
    pad[1, 5:max(S - 1, 5)] = 1                     # keys 5 .. S-2 of sequence 1; key 0 is real
    return qkv, pad


@pytest.mark.parametrize('S', [1, 13, 37])
def test_causal_row_is_the_last_row_of_attention_over_the_prefix(S):
    B, H, dh = 2, 2, 8
    qkv, pad = _case(B, S, H, dh, 100 + S)
    o, lse = cr.attention_qkv(qkv, H, dh, pad)
    for q in range(S):
        op, lp = ad.attention_qkv(qkv[:, :q + 1], H, dh, pad[:, :q + 1], None, 0.0)       # bidirectional over the prefix q + 1
        assert float((o[:, q] - op[:, q]).abs().max()) < 1e-12, q
        assert float((lse[:, :, q] - lp[:, :, q]).abs().max()) < 1e-12, q
    # without the mask the rows differ (the comparison can see a future key)
    if S > 1:
        ob, _ = ad.attention_qkv(qkv, H, dh, pad, None, 0.0)
        assert float((ob[:, 0] - o[:, 0]).abs().max()) > 1e-3
        assert float((ob[:, S - 1] - o[:, S - 1]).abs().max()) < 1e-12                    # the last row sees every key either way


def test_weights_above_the_diagonal_are_exactly_zero_and_rows_sum_to_one():
    B, S, H, dh = 2, 21, 2, 8
    qkv, pad = _case(B, S, H, dh, 7)
    w = cr.weights(qkv, H, dh, pad)
    above = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1)
    assert float(w[..., above].abs().max()) == 0.0
    assert float((w.sum(-1) - 1).abs().max()) < 1e-12
    assert bool((w[..., ~above] > 0).any())
    # ... and so are the gradients of the keys behind the last query that carries a gradient
    do = torch.zeros(B * S, H * dh, dtype=torch.float64)
    p = 9
    do[:p] = torch.randn(p, H * dh, dtype=torch.float64, generator=torch.Generator().manual_seed(1))      # sequence 0, rows < p
    _, _, g = cr.attention_grads(qkv.reshape(B * S, -1), do, [S] * B, H, dh, pad.reshape(-1))
    assert float(g[p:].abs().max()) == 0.0 and float(g[:p].abs().max()) > 0


def test_look_ahead_mask_helper():
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    import clickstream_transformer.transformer as alias
    m = T.create_look_ahead_mask(4)
    assert m.dtype == torch.float32 and tuple(m.shape) == (4, 4)
    assert torch.equal(m, torch.tensor([[0., 1, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1], [0, 0, 0, 0]]))
    assert alias.create_look_ahead_mask is T.create_look_ahead_mask
    # the restatement's additive mask is this mask times -inf
    neg = cr.causal_neg(4)[0, 0]
    assert torch.equal(torch.isinf(neg), m.bool())


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_abi_stays_12():
    """the three entry points and the flag are declared in include/b4c.h (the preprocessed header shows them to a C caller) and
    bound with the lists it gives"""
    import re
    import shutil
    import subprocess
    from bert4clickpath_amd import _lib, ops
    lib = _lib.lib()
    assert lib.b4c_abi_version() == abi_pin.ABI_VERSION and _lib.ABI_VERSION == abi_pin.ABI_VERSION
    new = ('b4c_attn_fwd_ex', 'b4c_attn_bwd_ex', 'b4c_attn_weights_ex')
    sig = _lib.signatures()
    assert set(sig) == set(_lib.declared_symbols()) and len(sig) == abi_pin.ENTRY_POINTS
    assert {n for n in sig if re.fullmatch(r'b4c_attn_(?!mq_)\w+_ex', n)} == set(new)
    for name in new:
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == sig[name][1], name
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    if cc:              # what a C compiler sees of b4c.h
        pre = subprocess.run([cc, '-E', '-dD', _lib.HEADER_PATH], capture_output=True, text=True, check=True).stdout
        for name in new:
            assert re.search(r'\bint %s\(' % name, pre), name
        assert re.search(r'#define B4C_ATTN_CAUSAL 1u', pre)
    assert _lib.header_constants(_lib._header_text(_lib.HEADER_PATH))['B4C_ATTN_CAUSAL'] == 1
    assert _lib.ATTN_CAUSAL == ops.ATTN_CAUSAL == 1
    with open(_lib.HEADER_PATH) as f:
        assert '#define B4C_ATTN_CAUSAL 1u' in f.read()
    c = _lib.ctypes
    tail = [c.c_float, c.c_uint64, c.c_uint32]                      # (dropout_rate, seed, flags)
    # forward: b4c_attn_fwd_varlen_drop's list (cu_seqlens may be NULL) with flags appended; backward likewise; weights + flags
    assert sig['b4c_attn_fwd_ex'][1] == sig['b4c_attn_fwd_varlen_drop'][1] + [c.c_uint32]
    assert sig['b4c_attn_bwd_ex'][1] == sig['b4c_attn_bwd_varlen_drop'][1] + [c.c_uint32]
    assert sig['b4c_attn_fwd_ex'][1][-3:] == tail and sig['b4c_attn_bwd_ex'][1][-3:] == tail
    assert sig['b4c_attn_weights_ex'][1] == sig['b4c_attn_weights'][1] + [c.c_uint32]
    # no existing signature changed
    assert len(sig['b4c_attn_fwd'][1]) == 12 and len(sig['b4c_attn_weights'][1]) == 11


def test_unknown_flag_bits_are_einval():
    """the flags are checked before any pointer is looked at: no GPU needed"""
    from bert4clickpath_amd import _lib
    lib = _lib.lib()
    for flags in (2, 0x80000000, 3):
        assert lib.b4c_attn_fwd_ex(None, 0, None, None, None, 0, None, 1, 1, 1, 32, _lib.F32, None, 0.0, 0, flags) != 0
        assert b'flag' in lib.b4c_last_error()
        assert lib.b4c_attn_bwd_ex(None, 0, None, None, None, 0, None, 0, None, None, None, 0, 1, 1, 1, 32, None, 0, _lib.F32, None,
                                   0.0, 0, flags) != 0
        assert b'flag' in lib.b4c_last_error()
        assert lib.b4c_attn_weights_ex(None, 0, None, None, None, 1, 1, 1, 32, _lib.F32, None, flags) != 0
        assert b'flag' in lib.b4c_last_error()
    # a rate outside [0, 1) likewise
    assert lib.b4c_attn_fwd_ex(None, 0, None, None, None, 0, None, 1, 1, 1, 32, _lib.F32, None, 1.0, 0, 1) != 0
    assert b'dropout rate' in lib.b4c_last_error()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
def _model(**kw):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    V = 50
    return ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': 64}, SoftMaxHead([16, 16], V),
                                  value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, **kw)


def test_attention_keyword_is_validated():
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    for bad in ('sideways', None, 'Causal', True):
        with pytest.raises(ValueError):
            T.EncoderLayer(32, 2, 64, 0.1, attention=bad)
        with pytest.raises(ValueError):
            T.Encoder(1, 32, 2, 64, 0.1, attention=bad)
        with pytest.raises(ValueError):
            T.Transformer(1, 2, {'items': 60}, {'items': 32}, 64, 0.1, attention=bad)
        with pytest.raises(ValueError):
            _model(attention=bad)
    assert T.EncoderLayer(32, 2, 64, 0.1, attention='causal').attention == 'causal'
    assert T.EncoderLayer(32, 2, 64, 0.1).attention == 'bidirectional'


def test_causal_needs_queries_and_keys_of_one_length():
    """raised before anything is launched (and before the device check): no GPU needed"""
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    q, k = torch.zeros(2, 2, 5, 16), torch.zeros(2, 2, 7, 16)
    with pytest.raises(ValueError, match='causal'):
        T.scaled_dot_product_attention(q, k, k, None, causal=True)
    mha = T.MultiHeadAttention(32, 2)
    x5, x7 = torch.zeros(2, 5, 32), torch.zeros(2, 7, 32)
    with pytest.raises(ValueError, match='causal'):
        mha(x7, x7, x5, None, causal=True)


def test_a_mask_of_another_shape_names_causal():
    from bert4clickpath_amd._lib import B4CError
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    with pytest.raises(B4CError, match='causal=True'):
        T._key_mask_bytes(T.create_look_ahead_mask(5), 2, 5, 'cpu')


def test_configs_carry_the_keyword_only_when_set_and_round_trip(tmp_path):
    from bert4clickpath_amd import checkpoint
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    default = _model()
    explicit = _model(attention='bidirectional')
    for m in (default, explicit):
        for cfg in (m.get_config(), m.transformer.get_config(), m.transformer.encoder.get_config(),
                    m.transformer.encoder.enc_layers[0].get_config()):
            assert 'attention' not in cfg
    assert set(explicit.get_config()) == set(default.get_config())
    m = _model(attention='causal')
    cfg, tcfg, ecfg = m.get_config(), m.transformer.get_config(), m.transformer.encoder.get_config()
    assert cfg['attention'] == tcfg['attention'] == ecfg['attention'] == 'causal'
    assert all(l.get_config()['attention'] == 'causal' for l in m.transformer.encoder.enc_layers)
    again = ClickstreamTransformer(**cfg)
    assert again.get_config() == cfg and again.transformer.get_config() == tcfg
    assert all(l.attention == 'causal' for l in again.transformer.encoder.enc_layers)
    assert T.Encoder(**ecfg).get_config() == ecfg
    assert T.EncoderLayer(**m.transformer.encoder.enc_layers[0].get_config()).attention == 'causal'
    # a checkpoint of the causal model restores into the model its config builds: the keyword adds no parameter
    path = checkpoint.save_checkpoint(os.path.join(str(tmp_path), 'ckpt-causal'), m)
    checkpoint.load_checkpoint(path, again)
    assert set(again.state_dict()) == set(default.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(v, again.state_dict()[k]), k
    assert again.attention == 'causal'


def test_a_causal_encoder_takes_the_full_last_layer():
    from bert4clickpath_amd import ops
    from bert4clickpath_amd._lib import B4CError
    enc, base = _model(attention='causal').transformer.encoder, _model().transformer.encoder
    for training in (False, True):
        assert not enc.rows_supported(None, training) and not enc.rows_route(None, training)
        assert base.rows_supported(None, training)
    was = ops.mq_attn_dropout
    ops.mq_attn_dropout = True
    try:
        assert not enc.rows_route(None, True) and base.rows_route(None, True)
    finally:
        ops.mq_attn_dropout = was
    with pytest.raises(B4CError, match='causal'):
        enc.enc_layers[0](torch.zeros(1, 4, 64), False, torch.zeros(1, 4, dtype=torch.uint8), None, rows=(None, None))


def test_blocks_pass_the_flag_and_only_when_set(monkeypatch):
    """EncoderLayer -> AttnBlockFn: a bidirectional layer makes the call it has always made (no extra argument), a causal one
    appends True; the blocks themselves are stubbed (no GPU)"""
    from bert4clickpath_amd import ops
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    seen = {}

    class Attn:
        @staticmethod
        def apply(x2, *a):
            seen['attn'] = a
            return x2

    class FFN:
        @staticmethod
        def apply(x2, *a):
            return x2
    monkeypatch.setattr(ops, 'AttnBlockFn', Attn)
    monkeypatch.setattr(ops, 'FFNBlockFn', FFN)
    x, pad = torch.zeros(2, 5, 32), torch.zeros(2, 5, dtype=torch.uint8)
    T.EncoderLayer(32, 2, 64, 0.1)(x, training=False, mask=pad)
    n = len(seen['attn'])
    assert seen['attn'][-2:] == (0.0, 0)
    T.EncoderLayer(32, 2, 64, 0.1, attention='causal')(x, training=False, mask=pad)
    assert len(seen['attn']) == n + 1 and seen['attn'][-1] is True and seen['attn'][-3:-1] == (0.0, 0)


def test_work_hint_of_a_causal_launch_is_the_triangle():
    from bert4clickpath_amd import ops
    lens = [1, 5, 32, 33]
    T_tok, S = sum(lens), max(lens)
    tri = sum(n * (n + 1) // 2 for n in lens)
    cu = object()                                   # (only its presence is looked at)
    ops.rec_hints['sum_len_sq'] = sum(n * n for n in lens)
    try:
        assert ops._attn_pairs(T_tok, S, cu, True) == tri
        assert ops._attn_pairs(T_tok, S, cu, False) == sum(n * n for n in lens)
    finally:
        ops.rec_hints.pop('sum_len_sq', None)
    assert ops._attn_pairs(4 * 10, 10, None, True) == 4 * 55 and ops._attn_pairs(4 * 10, 10, None, False) == 400
