"""Host side of the paper-faithful model ends (no GPU; NO REFERENCE ORACLE: extensions -- the float64 restatement is
tests/paper_model_ref.py): the restatement's closed-form gradients against autograd and its encoder against oracle/torch_ref.py,
constructor validation and get_config() rules of `embedding_layernorm` / `embedding_scale` / the head's `transform`, state-dict
names, the weight-decay exclusion list, and the new entry points in the C header and its binding."""
import numpy as np
import pytest
import torch

import abi_pin
import paper_model_ref as pm
from test_paper_encoder_cpu import DEFAULT_KEYS

V = 20


def _model(head=None, **kw):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    return ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': 16},
                                  head if head is not None else SoftMaxHead([8], V), value_to_head='[MASK]', num_encoder_layers=1,
                                  num_attention_heads=2, dropout_rate=0.0, **kw)


def _leaf(*shape, g, scale=1.0):
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).requires_grad_(True)


@pytest.mark.parametrize('combine,rate', [('concat', 0.0), ('concat', 0.25), ('sum', 0.25)])
def test_closed_form_input_stage_gradients_match_autograd(combine, rate):
    g = torch.Generator().manual_seed(1)
    B, S = 3, 7
    dims = (16, 16) if combine == 'sum' else (16, 8)
    d = 16 if combine == 'sum' else 24
    tables = [_leaf(11, w, g=g, scale=0.5) for w in dims]
    ids = [torch.randint(-1, 13, (B, S), generator=g) for _ in dims]        # ids below 0 and past the table: clamped
    pe, gamma, beta = _leaf(S + 2, d, g=g), _leaf(d, g=g), _leaf(d, g=g)
    keep = (torch.rand(B, S, d, generator=g) >= rate) if rate else None
    dout = torch.randn(B, S, d, generator=g, dtype=torch.float64)
    pre = pm.embed_pre(ids, tables, pe, 1.7, combine)
    pre.retain_grad()
    out = pm.tr.dropout(pm.tr.layer_norm(pre, gamma, beta, pm.EPS), rate, keep)
    assert torch.equal(out, pm.embed_ln(ids, tables, pe, 1.7, gamma, beta, keep, rate, combine))
    (out * dout).sum().backward()
    dpre, dgamma, dbeta = pm.ln_backward(dout, pre.detach(), gamma.detach(), keep, rate)
    for got, want in ((dpre, pre.grad), (dgamma, gamma.grad), (dbeta, beta.grad)):
        assert float((got - want).abs().max()) < 1e-10
    # the tables and the positional table receive dpre as the plain stage's backward hands it on: scale * rows, sum over sequences
    assert float((pe.grad[:S] - dpre.sum(0)).abs().max()) < 1e-10 and float(pe.grad[S:].abs().max()) == 0
    col = 0
    for i, t in zip(ids, tables):
        want = torch.zeros_like(t)
        w = t.shape[1]
        want.index_add_(0, i.clamp(0, t.shape[0] - 1).reshape(-1), 1.7 * dpre[..., col:col + w].reshape(-1, w))
        assert float((t.grad - want).abs().max()) < 1e-10
        col += 0 if combine == 'sum' else w


@pytest.mark.parametrize('act', ['relu', 'gelu', 'gelu_tanh'])
def test_closed_form_transform_gradients_match_autograd(act):
    g = torch.Generator().manual_seed(2)
    R, K, N = 9, 24, 16
    h, W, b, gamma, beta = _leaf(R, K, g=g), _leaf(K, N, g=g, scale=0.3), _leaf(N, g=g), _leaf(N, g=g), _leaf(N, g=g)
    dout = torch.randn(R, N, generator=g, dtype=torch.float64)
    (pm.head_transform(h, W, b, gamma, beta, act) * dout).sum().backward()
    got = pm.transform_backward(dout, h.detach(), W.detach(), b.detach(), gamma.detach(), act)
    for x, want in zip(got, (h.grad, W.grad, b.grad, gamma.grad, beta.grad)):
        assert float((x - want).abs().max()) < 1e-10


def test_restated_encoder_is_torch_refs():
    """paper_model_ref.encoder + embed_pre at the default scale == oracle/torch_ref.transformer_forward, to the last bit or two"""
    g = torch.Generator().manual_seed(3)
    m = _model()
    P = {k[len('transformer.'):]: v.detach().double() for k, v in m.state_dict().items() if k.startswith('transformer.')}
    ids = torch.randint(1, 30, (4, 9), generator=g)
    ids[1, 5:] = 0
    want = pm.tr.transformer_forward({'items': ids}, P, 1, 2)
    table = P['embedding_layers.items.weight']
    x = pm.embed_pre([ids], [table], pm.tr.positional_encoding(9, 16, torch.float64), float(np.sqrt(np.float32(16))))
    got = pm.encoder(x, ids == 0, P, 1, 2)
    assert float((got - want).abs().max()) < 1e-12


def test_argument_validation():
    from bert4clickpath_amd.clickstream_transformer import ClozeMaskedItemPrediction
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    for bad in (0, -1.0, float('inf'), float('nan'), 'one', True):
        with pytest.raises(ValueError):
            _model(embedding_scale=bad)
        with pytest.raises(ValueError):
            T.Transformer(1, 2, {'items': 30}, {'items': 16}, 8, 0.0, embedding_scale=bad)
    for bad in ('swish', 'GELU', '', 1, ['gelu']):
        with pytest.raises(ValueError):
            ClozeMaskedItemPrediction([], V, transform=bad)
    for ok in (None, 'relu', 'gelu', 'gelu_tanh'):
        assert ClozeMaskedItemPrediction([], V, transform=ok).transform == ok
    assert _model(embedding_scale=1).transformer.scale == 1.0
    assert _model(embedding_scale=np.float32(1.0)).transformer.scale == 1.0          # any real number, numpy's scalars too
    assert _model().transformer.scale == float(np.sqrt(np.float32(16)))


def test_get_config_key_rules_and_round_trip():
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer
    base = _model()
    for cfg in (base.get_config(), base.transformer.get_config()):
        assert not {'embedding_layernorm', 'embedding_scale'} & set(cfg)
    assert set(_model(embedding_layernorm=False, embedding_scale=None).get_config()) == set(base.get_config())
    m = _model(embedding_layernorm=True, embedding_scale=1.0)
    cfg, tcfg = m.get_config(), m.transformer.get_config()
    for c in (cfg, tcfg):
        assert c['embedding_layernorm'] is True and c['embedding_scale'] == 1.0
    again = ClickstreamTransformer(**cfg)
    assert again.get_config() == cfg and again.transformer.get_config() == tcfg and again.transformer.scale == 1.0
    only_scale = _model(embedding_scale=2.5).get_config()
    assert only_scale['embedding_scale'] == 2.5 and 'embedding_layernorm' not in only_scale


def test_state_dict_names_and_parameters():
    from bert4clickpath_amd import optim
    from bert4clickpath_amd.clickstream_transformer import ClozeMaskedItemPrediction
    assert list(_model().state_dict().keys()) == DEFAULT_KEYS
    assert list(_model(embedding_scale=1.0).state_dict().keys()) == DEFAULT_KEYS
    m = _model(embedding_layernorm=True)
    new = ['transformer.embedding_norm.gamma', 'transformer.embedding_norm.beta']
    assert sorted(m.state_dict().keys()) == sorted(DEFAULT_KEYS + new)
    n = m.transformer.embedding_norm
    assert torch.equal(n.gamma.detach(), torch.ones(16)) and torch.equal(n.beta.detach(), torch.zeros(16)) and n.epsilon == 1e-6
    # the tied head: unchanged without a transform; with one ALWAYS a last Dense to the table's width, and the norm
    tied = [k for k in _model(ClozeMaskedItemPrediction([], V)).state_dict() if k.startswith('head.')]
    assert tied == ['head.output_bias']
    wide = [k for k in _model(ClozeMaskedItemPrediction([8], V)).state_dict() if k.startswith('head.')]
    assert wide == ['head.output_bias'] + ['head.intermediate_layers.%d.%s' % (i, w) for i in (0, 1) for w in ('kernel', 'bias')]
    for dims, n_dense in (([], 1), ([16], 2), ([8], 2)):
        t = _model(ClozeMaskedItemPrediction(dims, V, transform='gelu_tanh'))
        keys = [k for k in t.state_dict() if k.startswith('head.')]
        want = ['head.output_bias'] + ['head.intermediate_layers.%d.%s' % (i, w) for i in range(n_dense) for w in ('kernel', 'bias')] + \
            ['head.transform_norm.gamma', 'head.transform_norm.beta']
        assert sorted(keys) == sorted(want), dims
        assert tuple(t.head.intermediate_layers[-1].kernel.shape) == (dims[-1] if dims else 16, 16)
        hn = t.head.transform_norm
        params = t.head._params()
        assert any(p is hn.gamma for p in params) and any(p is hn.beta for p in params)
        assert params[-2] is t.transformer.embedding_layers['items'].weight and params[-1] is t.head.output_bias
        no_decay = optim.no_decay_params(t)
        assert any(p is hn.gamma for p in no_decay) and any(p is hn.beta for p in no_decay)
    no_decay = optim.no_decay_params(m)
    assert any(p is n.gamma for p in no_decay) and any(p is n.beta for p in no_decay)


def test_header_declares_the_entry_points_and_the_binding_parses_them():
    import ctypes
    from bert4clickpath_amd import _lib as L
    assert L.ABI_VERSION == abi_pin.ABI_VERSION
    sig = L.signatures()
    new = ('b4c_embed_ln_fwd', 'b4c_embed_ln_bwd', 'b4c_embed_ln_bwd_workspace_bytes', 'b4c_layernorm_fwd', 'b4c_layernorm_bwd',
           'b4c_layernorm_bwd_workspace_bytes')
    for name in new:
        assert name in sig and name in L.declared_symbols()
    # the forward takes the packed plain stage's arguments plus gamma, beta, eps and stats
    assert len(sig['b4c_embed_ln_fwd'][1]) == len(sig['b4c_embed_concat_pe_fwd_packed'][1]) + 4
    assert sig['b4c_embed_ln_bwd_workspace_bytes'] == (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int])
    assert sig['b4c_layernorm_bwd_workspace_bytes'] == sig['b4c_add_dropout_layernorm_bwd_workspace_bytes']
    assert sig['b4c_layernorm_fwd'][0] is ctypes.c_int and ctypes.c_float in sig['b4c_layernorm_fwd'][1]
    assert sig['b4c_embed_ln_bwd'][1].count(ctypes.c_float) == 2 and sig['b4c_embed_ln_bwd'][1].count(ctypes.c_uint64) == 1
