"""The causal form of the masked-query last layer, the parts that need no GPU: the two entry points include/b4c.h declares, the
switch ops.mq_causal and the route it opens (Encoder.rows_route beside the unchanged Encoder.rows_supported), the trailing
argument EncoderLayer.forward(rows=) hands to the masked-query block, and the rows a caller names with flat_idx + row_offsets."""
import os
import subprocess
import sys

import pytest
import torch

import abi_pin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the header ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_drop_signatures_plus_flags():
    from bert4clickpath_amd import _lib
    sig, c = _lib.signatures(), _lib.ctypes
    assert {'b4c_attn_mq_bwd_ex', 'b4c_attn_mq_fwd_ex'} <= set(sig)
    for new, old in (('b4c_attn_mq_fwd_ex', 'b4c_attn_mq_fwd_drop'), ('b4c_attn_mq_bwd_ex', 'b4c_attn_mq_bwd_drop')):
        assert sig[new][0] == sig[old][0]
        assert sig[new][1] == sig[old][1] + [c.c_uint32]           # a trailing uint32_t flags
    assert _lib.ATTN_CAUSAL == 1                                    # the flag bit is that of the b4c_attn_*_ex entry points


def test_pinned_counts_and_abi_version_stay():
    from bert4clickpath_amd import _lib
    assert _lib.ABI_VERSION == abi_pin.ABI_VERSION
    assert len(_lib.signatures()) == abi_pin.ENTRY_POINTS == len(_lib.declared_symbols())          # the README's entry-point count


def test_library_exports_the_entry_points():
    from bert4clickpath_amd import _lib
    lib, sig = _lib.lib(), _lib.signatures()
    assert lib.b4c_abi_version() == abi_pin.ABI_VERSION
    for name in ('b4c_attn_mq_fwd_ex', 'b4c_attn_mq_bwd_ex'):
        assert hasattr(lib, name) and list(getattr(lib, name).argtypes) == sig[name][1]


# ---- the switch ----------------------------------------------------------------------------------------------------------------------
def test_the_switch_is_off_by_default_and_follows_the_environment():
    from bert4clickpath_amd import ops
    if 'B4C_MQ_CAUSAL' not in os.environ:
        assert ops.mq_causal is False
    # the variable is read once, at import: one fresh interpreter with it set
    out = subprocess.run([sys.executable, '-c', 'from bert4clickpath_amd import ops; print(ops.mq_causal)'], cwd=ROOT,
                         env=dict(os.environ, B4C_MQ_CAUSAL='1'), capture_output=True, text=True, check=True)
    assert out.stdout.strip() == 'True', out.stdout


def _encoder(attention, attn_rate, heads=2):
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    return T.Encoder(num_layers=2, d_model=64, num_heads=heads, dff=32, dropout_rate=0.1, attention_dropout_rate=attn_rate,
                     attention=attention)


def test_rows_route_over_every_cell_and_rows_supported_unchanged(monkeypatch):
    from bert4clickpath_amd import ops
    for attention in ('bidirectional', 'causal'):
        for attn_rate in (0.0, 0.2):
            enc = _encoder(attention, attn_rate)
            for training in (False, True):
                # rows_supported: the parent's answer in every cell, whatever the switches say
                want_supported = attention != 'causal' and not (training and attn_rate > 0)
                for mq_causal in (False, True):
                    for mq_drop in (False, True):
                        monkeypatch.setattr(ops, 'mq_causal', mq_causal)
                        monkeypatch.setattr(ops, 'mq_attn_dropout', mq_drop)
                        assert enc.rows_supported(None, training) is want_supported
                        needs_drop = training and attn_rate > 0
                        if attention == 'causal':
                            want = mq_causal and (mq_drop or not needs_drop)
                        else:
                            want = mq_drop or not needs_drop          # (the causal switch does not touch a bidirectional encoder)
                        assert enc.rows_route(None, training) is want, (attention, attn_rate, training, mq_causal, mq_drop)
    # the shape conditions stay: head depth 16
    monkeypatch.setattr(ops, 'mq_causal', True)
    monkeypatch.setattr(ops, 'mq_attn_dropout', True)
    assert _encoder('causal', 0.0, heads=4).rows_route(None, False) is False


# ---- EncoderLayer.forward(rows=) -----------------------------------------------------------------------------------------------------
def _layer_with_rows(monkeypatch, attention, switch):
    """the blocks stubbed as tests/test_causal_cpu.py::test_blocks_pass_the_flag_and_only_when_set stubs them (no GPU)"""
    from bert4clickpath_amd import ops
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    monkeypatch.setattr(ops, 'mq_causal', switch)
    seen = {}

    class MQ:
        @staticmethod
        def apply(x2, midx, *a):
            seen['mq'] = (midx,) + a
            return x2[:midx.shape[0]]

    class FFN:
        @staticmethod
        def apply(x2, *a):
            return x2
    monkeypatch.setattr(ops, 'MQAttnBlockFn', MQ)
    monkeypatch.setattr(ops, 'FFNBlockFn', FFN)
    layer = T.EncoderLayer(32, 2, 64, 0.1, attention=attention)
    rows = (torch.tensor([1, 3, 7], dtype=torch.int32), torch.tensor([0, 2, 3], dtype=torch.int32))
    return layer, seen, rows


@pytest.mark.parametrize('switch', [False, True])
def test_bidirectional_rows_call_passes_no_extra_argument(monkeypatch, switch):
    layer, seen, rows = _layer_with_rows(monkeypatch, 'bidirectional', switch)
    out = layer(torch.zeros(2, 5, 32), training=False, mask=torch.zeros(2, 5, dtype=torch.uint8), rows=rows)
    assert out.shape == (3, 32)
    assert seen['mq'][-2:] == (0.0, 0) and seen['mq'][0] is rows[0]          # ..., attn_rate, attn_seed: the call of today
    seen['n'] = len(seen['mq'])
    layer2, seen2, _ = _layer_with_rows(monkeypatch, 'causal', True)
    layer2(torch.zeros(2, 5, 32), training=False, mask=torch.zeros(2, 5, dtype=torch.uint8), rows=rows)
    assert len(seen2['mq']) == seen['n'] + 1 and seen2['mq'][-1] is True and seen2['mq'][-3:-1] == (0.0, 0)
    assert seen2['mq'][0] is rows[0] and seen2['mq'][1] is rows[1]           # midx goes down as it came: the kernels' q_rows


def test_causal_rows_call_with_the_switch_off_raises_as_today(monkeypatch):
    from bert4clickpath_amd._lib import B4CError
    layer, seen, rows = _layer_with_rows(monkeypatch, 'causal', False)
    with pytest.raises(B4CError, match='causal'):
        layer(torch.zeros(2, 5, 32), training=False, mask=torch.zeros(2, 5, dtype=torch.uint8), rows=rows)
    assert 'mq' not in seen


def test_ops_wrappers_refuse_causal_without_q_rows():
    from bert4clickpath_amd import ops
    q = torch.zeros(1, 64)
    with pytest.raises(ValueError, match='q_rows'):
        ops.attn_mq_fwd(q, q, None, None, 1, 1, 1, 64, None, None, 0.0, 0, causal=True)
    with pytest.raises(ValueError, match='q_rows'):
        ops.attn_mq_bwd(q, q, None, None, q, q, q, 1, 1, 1, 64, None, None, 0.0, 0, causal=True)


def test_work_hint_of_a_causal_launch_counts_the_visible_pairs():
    from bert4clickpath_amd import ops
    ops.rec_hints['sum_q_len'] = 700
    try:
        assert ops._attn_mq_pairs(5, 200, False) == 700 and ops._attn_mq_pairs(5, 200, True) == 700       # no causal hint: the bound
        ops.rec_hints['sum_q_visible'] = 123
        assert ops._attn_mq_pairs(5, 200, True) == 123 and ops._attn_mq_pairs(5, 200, False) == 700
    finally:
        ops.rec_hints.pop('sum_q_len', None)
        ops.rec_hints.pop('sum_q_visible', None)
    assert ops._attn_mq_pairs(5, 200, True) == 1000 and ops._attn_mq_pairs(5, 200, False) == 1000


# ---- the rows a caller names -----------------------------------------------------------------------------------------------------------
def _cpu_model(attention):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(0)
    return ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(20)]}, {'items': 64}, SoftMaxHead([16], 20),
                                  value_to_head='[MASK]', num_encoder_layers=1, num_attention_heads=2, dropout_rate=0.0,
                                  attention=attention)


class _Encode:
    """stands in for ClickstreamTransformer._encode: notes what rows_of hands over"""

    def __init__(self, model, B, S, d):
        self.model, self.B, self.S, self.d, self.calls = model, B, S, d, []

    def __call__(self, inputs, training, pack=False, n_real_tokens=None, rows_of=None):
        ids = torch.zeros(self.B, self.S, dtype=torch.int64)
        self.model._packed = None
        got = rows_of(ids, ids) if rows_of is not None else None
        self.calls.append(got)
        if got is not None:
            return torch.ones(got[0].shape[0], self.d), ids, ids, None, None
        return torch.ones(self.B, self.S, self.d), ids, ids, None, None


@pytest.mark.parametrize('attention,switch,route', [('bidirectional', False, True), ('causal', True, True), ('causal', False, False)])
def test_masked_rows_with_flat_idx_and_row_offsets_hands_exactly_those_to_encode(monkeypatch, attention, switch, route):
    from bert4clickpath_amd import ops
    monkeypatch.setattr(ops, 'mq_causal', switch)
    monkeypatch.setattr(ops, 'mq_last_layer', True)
    model = _cpu_model(attention)
    enc = _Encode(model, 3, 8, 64)
    monkeypatch.setattr(model, '_encode', enc)
    gathered = {}

    class Gather:
        @staticmethod
        def apply(src, idx, n):
            gathered['idx'] = idx
            return src[idx.long().clamp(min=0)]
    monkeypatch.setattr(ops, 'GatherRowsFn', Gather)
    flat = torch.tensor([5, 20, -1], dtype=torch.int32)
    off = torch.tensor([0, 1, 1, 2], dtype=torch.int32)              # the second sequence has no row
    rows, lab = model._masked_rows({}, False, flat, row_offsets=off)
    assert lab is None and tuple(rows.shape) == (3, 64)
    if route:
        (got,) = enc.calls
        assert torch.equal(got[0], flat) and torch.equal(got[1], off) and got[2] is None
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32
        assert torch.equal(model._row_offsets, off) and 'idx' not in gathered
    else:
        assert enc.calls == [None] and torch.equal(gathered['idx'], flat)          # the gather route, as today
    # flat_idx alone: the gather route whatever the switches say
    enc.calls.clear()
    gathered.clear()
    rows, _ = model._masked_rows({}, False, flat)
    assert enc.calls == [None] and torch.equal(gathered['idx'], flat) and model._row_offsets is None
    # ... and with the masked-query last layer switched off, row_offsets changes nothing either
    monkeypatch.setattr(ops, 'mq_last_layer', False)
    enc.calls.clear()
    gathered.clear()
    model._masked_rows({}, False, flat, row_offsets=off)
    assert enc.calls == [None] and torch.equal(gathered['idx'], flat)
