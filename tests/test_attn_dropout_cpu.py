"""Attention-probability dropout, the parts that need no GPU: the keep rule of include/b4c.h (b4c_attn_keep) against b4c_keep
and the element index restated in Python, the ABI version, the configs, and the seed stream of EncoderLayer."""
import numpy as np
import pytest
import torch

import abi_pin
import attn_dropout_ref as ref
from attn_dropout_ref import elem_index

H, B = 2, 2


@pytest.fixture(scope='module')
def lib():
    from bert4clickpath_amd import _lib
    return _lib.lib()


def _mask(lib, seed, S_arg, rate):
    return np.asarray([[[[lib.b4c_attn_keep(seed, b, h, q, k, H, S_arg, rate) for k in range(S_arg)] for q in range(S_arg)]
                        for h in range(H)] for b in range(B)], dtype=bool)


@pytest.mark.parametrize('S_arg', [22, 40])        # 22: S4 = 24, the row pitch of the rule is not the sequence pitch
def test_keep_rule_is_b4c_keep_at_the_documented_index(lib, S_arg):
    from bert4clickpath_amd import ops
    seed, rate = 0x1234567 + S_arg, 0.25
    got = _mask(lib, seed, S_arg, rate)
    want = np.asarray([[[[lib.b4c_keep(seed, elem_index(b, h, q, k, H, S_arg), rate) for k in range(S_arg)] for q in range(S_arg)]
                         for h in range(H)] for b in range(B)], dtype=bool)
    assert np.array_equal(got, want)
    # the vectorised host regeneration the GPU tests use
    assert np.array_equal(ops.attn_keep_mask(seed, B, H, S_arg, rate).numpy(), got)
    if S_arg == 22:
        assert elem_index(0, 0, 1, 0, H, S_arg) == 24


def test_kept_fraction_and_rate_zero(lib):
    m = _mask(lib, 99, 40, 0.25)
    assert m.size == 6400
    assert 0.70 <= float(m.mean()) <= 0.80          # 0.75 +- 9 sigma of the binomial (sigma = 0.0054)
    assert _mask(lib, 99, 40, 0.0).all()


@pytest.mark.parametrize('S,dh', [(10, 4), (22, 8), (37, 16)])      # S > dh: 3 passes each; 22, 37: S4 != S; 10: a pass of two keys
def test_recovery_construction_on_the_restatement(S, dh):
    """The harness of tests/test_gpu_attn_dropout_routes.py, shown on the float64 restatement alone: with q = k = 0 and the one-hot
    V / dO of pass p, the nonzero pattern of o and of dV over ceil(S / dh) passes IS the regenerated mask AND NOT pad."""
    from bert4clickpath_amd import ops
    Bn, rate, seed = 2, 0.25, 0xC0FFEE + S
    lens = [S] * Bn
    pad = ref.recovery_pads(Bn, S)
    assert pad[0, S - 4:].all() and pad[1, 5:S - 1].all() and int(pad.sum()) == 4 + S - 6
    keep = ops.attn_keep_mask(seed, Bn, H, S, rate)
    fwd = [torch.zeros(H, S, S, dtype=torch.bool) for _ in lens]
    bwd = [torch.zeros(H, S, S, dtype=torch.bool) for _ in lens]
    assert ref.recovery_passes(S, dh) == 3
    for p in range(ref.recovery_passes(S, dh)):
        qkv, do = ref.recovery_operands(lens, H, dh, p, torch.float64)
        o, lse, g = ref.attention_grads(qkv, do, pad, Bn, S, H, dh, keep, rate)
        d = H * dh
        assert not g[:, :2 * d].any()                                   # dQ, dK: exactly zero
        real = (pad == 0).sum(1).double()
        assert float((lse - real.log()[:, None, None]).abs().max()) < 1e-12
        ref.recovery_collect(fwd, bwd, o, g[:, 2 * d:], lens, H, dh, p)
    for b in range(Bn):
        want = keep[b] & (pad[b] == 0)[None, None, :]
        assert torch.equal(fwd[b], want) and torch.equal(bwd[b], want), b
        assert want.any() and not want.all() and not want[:, :, pad[b] != 0].any()


def test_abi_version_stays_12(lib):
    from bert4clickpath_amd import _lib
    assert lib.b4c_abi_version() == abi_pin.ABI_VERSION and _lib.ABI_VERSION == abi_pin.ABI_VERSION
    for name in ('b4c_attn_keep', 'b4c_attn_fwd_drop', 'b4c_attn_bwd_drop_ws', 'b4c_attn_fwd_varlen_drop', 'b4c_attn_bwd_varlen_drop'):
        assert name in _lib.declared_symbols() and hasattr(lib, name)
    # (dropout_rate, seed) are appended to the lists of the entry points they mirror
    sig = _lib.signatures()
    for new, old in (('b4c_attn_fwd_drop', 'b4c_attn_fwd'), ('b4c_attn_bwd_drop_ws', 'b4c_attn_bwd_ws'),
                     ('b4c_attn_fwd_varlen_drop', 'b4c_attn_fwd_varlen'), ('b4c_attn_bwd_varlen_drop', 'b4c_attn_bwd_varlen')):
        assert sig[new][1][:-2] == sig[old][1] and sig[new][1][-2:] == [_lib.ctypes.c_float, _lib.ctypes.c_uint64]


def _model(**kw):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    V = 50
    return ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': 64}, SoftMaxHead([16, 16], V),
                                  value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, **kw)


def test_configs_carry_the_rate_only_when_set():
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    m = _model(attention_dropout_rate=0.2)
    cfg = m.get_config()
    assert cfg['attention_dropout_rate'] == 0.2
    assert m.transformer.get_config()['attention_dropout_rate'] == 0.2
    assert m.transformer.encoder.get_config()['attention_dropout_rate'] == 0.2
    assert all(l.get_config()['attention_dropout_rate'] == 0.2 for l in m.transformer.encoder.enc_layers)
    again = ClickstreamTransformer(**cfg)
    assert again.get_config() == cfg
    assert all(l.attention_dropout_rate == 0.2 for l in again.transformer.encoder.enc_layers)
    default = _model()
    assert 'attention_dropout_rate' not in default.get_config()
    assert 'attention_dropout_rate' not in default.transformer.get_config()
    assert 'attention_dropout_rate' not in default.transformer.encoder.get_config()
    assert 'attention_dropout_rate' not in default.transformer.encoder.enc_layers[0].get_config()
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            T.EncoderLayer(32, 2, 64, 0.1, attention_dropout_rate=bad)
    # the masked-query last layer has no attention dropout: a training pass with the rate set takes the full layer
    enc = m.transformer.encoder
    assert enc.rows_supported(None) and enc.rows_supported(None, False) and not enc.rows_supported(None, True)
    assert default.transformer.encoder.rows_supported(None, True)


class _Stub:
    def __init__(self):
        self.draws = 0

    def next(self):
        self.draws += 1
        return 1000 + self.draws


@pytest.mark.parametrize('attn_rate,training,want', [(0.0, True, 2), (0.2, True, 3), (0.0, False, 0), (0.2, False, 0)])
def test_encoder_layer_seed_draws(monkeypatch, attn_rate, training, want):
    """two draws per training call at rate 0 (the stream every existing model sees), a third -- drawn last -- with attention
    dropout, none in evaluation; the blocks themselves are stubbed (no GPU)"""
    from bert4clickpath_amd import ops
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    stub = _Stub()
    monkeypatch.setattr(T, 'dropout_seeds', stub)
    seen = {}

    class Attn:
        @staticmethod
        def apply(x2, *a):
            seen['attn'] = a
            return x2

    class FFN:
        @staticmethod
        def apply(x2, *a):
            seen['ffn'] = a
            return x2
    monkeypatch.setattr(ops, 'AttnBlockFn', Attn)
    monkeypatch.setattr(ops, 'FFNBlockFn', FFN)
    layer = T.EncoderLayer(32, 2, 64, 0.1, attention_dropout_rate=attn_rate)
    x = torch.zeros(2, 5, 32)
    layer(x, training=training, mask=torch.zeros(2, 5, dtype=torch.uint8))
    assert stub.draws == want
    a = seen['attn']
    a_rate, a_seed = a[-2], a[-1]
    if training:
        assert a[17] == 1001 and seen['ffn'][-3] == 1002           # s1, s2: the first two draws, as ever
    assert (a_rate, a_seed) == ((attn_rate, 1003) if want == 3 else (0.0, 0))
