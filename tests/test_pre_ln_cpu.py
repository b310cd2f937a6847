"""Pre-LN encoder blocks (norm='pre'), the parts that need no GPU: the float64 restatement tests/pre_ln_ref.py against an
independent implementation (torch.nn.TransformerEncoderLayer(norm_first=True)), the entry points' declarations in include/b4c.h and their
binding, the argument refusals of b4c_layernorm_bwd_add, the keyword on the four classes, get_config, state-dict names, the
masked-query route's answer and background_dw_expected(norm=)."""
import ctypes
import os

import pytest
import torch

import abi_pin
import pre_ln_ref as plr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against torch's norm_first layer ---------------------------------------------------------------------------
def _torch_layer(P, pre, d, H, dff, act):
    layer = torch.nn.TransformerEncoderLayer(d, H, dim_feedforward=dff, dropout=0.0, activation=act, layer_norm_eps=1e-6,
                                             batch_first=True, norm_first=True, dtype=torch.float64)
    with torch.no_grad():
        layer.self_attn.in_proj_weight.copy_(torch.cat([P[pre + 'mha.w%s.kernel' % n].T for n in 'qkv']))
        layer.self_attn.in_proj_bias.copy_(torch.cat([P[pre + 'mha.w%s.bias' % n] for n in 'qkv']))
        layer.self_attn.out_proj.weight.copy_(P[pre + 'mha.dense.kernel'].T)
        layer.self_attn.out_proj.bias.copy_(P[pre + 'mha.dense.bias'])
        layer.linear1.weight.copy_(P[pre + 'ffn.0.kernel'].T)
        layer.linear1.bias.copy_(P[pre + 'ffn.0.bias'])
        layer.linear2.weight.copy_(P[pre + 'ffn.1.kernel'].T)
        layer.linear2.bias.copy_(P[pre + 'ffn.1.bias'])
        layer.norm1.weight.copy_(P[pre + 'layernorm1.gamma'])
        layer.norm1.bias.copy_(P[pre + 'layernorm1.beta'])
        layer.norm2.weight.copy_(P[pre + 'layernorm2.gamma'])
        layer.norm2.bias.copy_(P[pre + 'layernorm2.beta'])
    return layer.train()        # (dropout 0: training mode only keeps torch on its plain, differentiable path)


def _layer_params(d, dff, g, pre):
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    P = {}
    for n in ('wq', 'wk', 'wv', 'dense'):
        P[pre + 'mha.%s.kernel' % n], P[pre + 'mha.%s.bias' % n] = r(d, d) / d ** 0.5, r(d) * 0.1
    P[pre + 'ffn.0.kernel'], P[pre + 'ffn.0.bias'] = r(d, dff) / d ** 0.5, r(dff) * 0.1
    P[pre + 'ffn.1.kernel'], P[pre + 'ffn.1.bias'] = r(dff, d) / dff ** 0.5, r(d) * 0.1
    for n in ('layernorm1', 'layernorm2'):
        P[pre + n + '.gamma'], P[pre + n + '.beta'] = 1 + 0.1 * r(d), 0.1 * r(d)
    return P


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('act', ['relu', 'gelu'])
def test_restatement_matches_torch_norm_first_layer(act, causal):
    d, H, S, B, dff = 16, 2, 7, 3, 24
    g = torch.Generator().manual_seed(5 + causal)
    pre = 'encoder.enc_layers.0.'
    P = _layer_params(d, dff, g, pre)
    lens = [7, 4, 1]
    ids = torch.zeros(B, S, dtype=torch.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = 5
    real = (ids != 0)
    x0 = torch.randn(B, S, d, generator=g, dtype=torch.float64)
    w = torch.randn(B, S, d, generator=g, dtype=torch.float64) * real[..., None]       # the loss reads the real positions only
    xa = x0.clone().requires_grad_(True)
    ya = plr.layer(xa, P, pre, H, plr.attention_mask(ids, torch.float64, causal), act)
    (ya * w).sum().backward()
    xb = x0.clone().requires_grad_(True)
    layer = _torch_layer(P, pre, d, H, dff, act)
    cm = torch.triu(torch.ones(S, S, dtype=torch.bool), 1) if causal else None
    yb = layer(xb, src_mask=cm, src_key_padding_mask=~real)
    (yb * w).sum().backward()
    err_y = float(((ya - yb).detach().abs() * real[..., None]).max())
    # a padded position's input reaches the loss through no real query (its key is masked): its gradient is exactly 0 on both sides
    err_g = float((xa.grad - xb.grad).abs().max())
    print('output %.2e gradient %.2e' % (err_y, err_g))
    assert err_y <= 1e-12 and err_g <= 1e-12
    assert float(xa.grad.abs().max()) > 1e-2


def test_encoder_restatement_ends_with_the_final_norm():
    d, H, S, B, dff = 16, 2, 5, 2, 8
    g = torch.Generator().manual_seed(1)
    P = {}
    for i in range(2):
        P.update(_layer_params(d, dff, g, 'encoder.enc_layers.%d.' % i))
    P['encoder.final_norm.gamma'] = 1 + 0.1 * torch.randn(d, generator=g, dtype=torch.float64)
    P['encoder.final_norm.beta'] = 0.1 * torch.randn(d, generator=g, dtype=torch.float64)
    x = torch.randn(B, S, d, generator=g, dtype=torch.float64)
    ids = torch.ones(B, S, dtype=torch.int64)
    neg = plr.attention_mask(ids, torch.float64)
    out = plr.encoder(x, P, 2, H, neg)
    s = plr.layer(plr.layer(x, P, 'encoder.enc_layers.0.', H, neg), P, 'encoder.enc_layers.1.', H, neg)
    want = torch.nn.functional.layer_norm(s, (d,), P['encoder.final_norm.gamma'], P['encoder.final_norm.beta'], 1e-6)
    assert float((out - want).abs().max()) < 1e-12


def test_closed_form_of_the_row_kernel_is_the_autograd_of_layer_norm():
    g = torch.Generator().manual_seed(2)
    rows, d = 9, 24
    x = torch.randn(rows, d, generator=g, dtype=torch.float64) * 1.5 + 0.3
    dout, res = torch.randn(rows, d, generator=g, dtype=torch.float64), torch.randn(rows, d, generator=g, dtype=torch.float64)
    gamma = 1 + 0.1 * torch.randn(d, generator=g, dtype=torch.float64)
    mean = x.mean(1)
    rstd = torch.rsqrt(((x - mean[:, None]) ** 2).mean(1) + 1e-6)
    a = plr.ln_bwd_add(dout, x, mean, rstd, gamma, res)
    b = plr.ln_bwd_add_autograd(dout, x, gamma, res)
    for u, v in zip(a, b):
        assert float((u - v).abs().max()) < 1e-12


# ---- the header and the binding ----------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_counts_hold():
    from bert4clickpath_amd import _lib
    sig = _lib.signatures()
    names = ['b4c_gemm_nt_ln_bwd_add', 'b4c_gemm_nt_ln_bwd_add_workspace_bytes', 'b4c_layernorm_bwd_add',
             'b4c_layernorm_bwd_add_workspace_bytes']
    assert set(names) <= set(sig)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert sig['b4c_layernorm_bwd_add'] == (i32, [vp, vp, vp, vp, vp, i32, vp, vp, vp, i64, i32, vp, i64, i32, vp])
    assert sig['b4c_layernorm_bwd_add_workspace_bytes'] == sig['b4c_layernorm_bwd_workspace_bytes']
    assert sig['b4c_gemm_nt_ln_bwd_add'] == (i32, [vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, vp, i64, i32, vp])
    assert sig['b4c_gemm_nt_ln_bwd_add_workspace_bytes'] == (i64, [i32, i32])
    # the whole ABI, and its version
    assert len(sig) == abi_pin.ENTRY_POINTS == len(_lib.declared_symbols()) and _lib.ABI_VERSION == abi_pin.ABI_VERSION
    with open(os.path.join(ROOT, 'bert4clickpath_amd', 'csrc', 'Makefile')) as f:
        assert 'pre_ln.hip' in f.read()
    lib = _lib.lib()
    for name in names:
        assert list(getattr(lib, name).argtypes) == sig[name][1] and getattr(lib, name).restype is sig[name][0], name


def test_library_exports_and_binds_the_entry_points():
    from bert4clickpath_amd import _lib
    lib = _lib.lib()
    assert lib.b4c_abi_version() == abi_pin.ABI_VERSION
    assert lib.b4c_layernorm_bwd_add.argtypes == _lib.signatures()['b4c_layernorm_bwd_add'][1]
    assert lib.b4c_layernorm_bwd_add_workspace_bytes(100, 128) == lib.b4c_layernorm_bwd_workspace_bytes(100, 128) > 0
    assert lib.b4c_layernorm_bwd_add_workspace_bytes(0, 128) == 0


def test_row_kernel_refuses_bad_arguments_without_a_launch():
    """every pointer below is a host address that is 16-byte aligned and never dereferenced: each call must come back with
    B4C_EINVAL from the argument checks"""
    from bert4clickpath_amd import _lib
    lib = _lib.lib()
    einval = _lib._C['B4C_EINVAL']
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    ws_bytes = lib.b4c_layernorm_bwd_add_workspace_bytes(4, 64)

    def call(**kw):
        a = dict(dout=p, x=p, stats=p, gamma=p, res=p, ld_res=64, dx=p, dgamma=p, dbeta=p, rows=4, d=64, ws=p, ws_bytes=ws_bytes,
                 dtype=_lib.F32)
        a.update(kw)
        return lib.b4c_layernorm_bwd_add(a['dout'], a['x'], a['stats'], a['gamma'], a['res'], a['ld_res'], a['dx'], a['dgamma'],
                                         a['dbeta'], a['rows'], a['d'], a['ws'], a['ws_bytes'], a['dtype'], None)
    for name in ('dout', 'x', 'stats', 'gamma', 'res', 'dx', 'dgamma', 'dbeta', 'ws'):
        assert call(**{name: None}) == einval, name
    for kw in ({'rows': 0}, {'rows': -1}, {'d': 0}, {'d': 12}, {'d': 1032, 'ld_res': 1032}, {'ld_res': 56}, {'ld_res': 68},
               {'res': p + 4}, {'ws_bytes': ws_bytes - 1}, {'ws_bytes': 0}, {'dtype': 7}):
        assert call(**kw) == einval, kw
        assert b'layernorm_bwd_add' in lib.b4c_last_error()


def test_matrix_core_kernel_refuses_bad_arguments_without_a_launch():
    from bert4clickpath_amd import _lib
    lib = _lib.lib()
    einval = _lib._C['B4C_EINVAL']
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    ws_bytes = lib.b4c_gemm_nt_ln_bwd_add_workspace_bytes(4, 128)
    assert ws_bytes > 0 and lib.b4c_gemm_nt_ln_bwd_add_workspace_bytes(0, 128) == 0

    def call(**kw):
        a = dict(A=p, lda=384, Bt=p, ldb=384, x=p, stats=p, gamma=p, res=p, ld_res=128, dx=p, dgamma=p, dbeta=p, M=4, N=128, K=384,
                 ws=p, ws_bytes=ws_bytes, dtype=_lib.BF16)
        a.update(kw)
        return lib.b4c_gemm_nt_ln_bwd_add(a['A'], a['lda'], a['Bt'], a['ldb'], a['x'], a['stats'], a['gamma'], a['res'], a['ld_res'],
                                          a['dx'], a['dgamma'], a['dbeta'], a['M'], a['N'], a['K'], a['ws'], a['ws_bytes'], a['dtype'],
                                          None)
    for name in ('A', 'Bt', 'x', 'stats', 'gamma', 'res', 'dx', 'dgamma', 'dbeta', 'ws'):
        assert call(**{name: None}) == einval, name
    for kw in ({'M': 0}, {'N': 0}, {'N': 264, 'ld_res': 264}, {'N': 132, 'ld_res': 136}, {'K': 0}, {'K': 388, 'lda': 392, 'ldb': 392},
               {'lda': 376}, {'ldb': 376}, {'lda': 388}, {'ldb': 388}, {'ld_res': 120}, {'ld_res': 132},
               {'lda': 1 << 22}, {'ldb': 1 << 22},                       # a 128-row tile of 2^30 bytes: b4c_gemm_nt's rule
               {'A': p + 8}, {'Bt': p + 8}, {'x': p + 8}, {'res': p + 8}, {'dx': p + 8}, {'gamma': p + 8},
               {'ws_bytes': ws_bytes - 1}, {'dtype': _lib.F32}, {'dtype': 9}):
        assert call(**kw) == einval, kw
        assert b'gemm_nt_ln_bwd_add' in lib.b4c_last_error()


# ---- the keyword -----------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(0)
    return ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(20)]}, {'items': 64}, SoftMaxHead([16], 20),
                                  value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, dropout_rate=0.1, **kw)


def test_keyword_is_validated_on_the_four_classes():
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    for bad in ('Pre', 'pre_ln', None, 1, ''):
        with pytest.raises(ValueError, match='norm'):
            T.EncoderLayer(32, 2, 64, 0.1, norm=bad)
        with pytest.raises(ValueError, match='norm'):
            T.Encoder(1, 32, 2, 64, 0.1, norm=bad)
        with pytest.raises(ValueError, match='norm'):
            T.Transformer(1, 2, {'items': 30}, {'items': 32}, 64, 0.1, norm=bad)
        with pytest.raises(ValueError, match='norm'):
            _model(norm=bad)
    for good in ('post', 'pre'):
        assert T.EncoderLayer(32, 2, 64, 0.1, norm=good).norm == good
        assert T.Encoder(1, 32, 2, 64, 0.1, norm=good).norm == good
        assert T.Transformer(1, 2, {'items': 30}, {'items': 32}, 64, 0.1, norm=good).norm == good
        assert _model(norm=good).norm == good
    assert _model().norm == 'post' and _model().transformer.encoder.norm == 'post'
    assert all(l.norm == 'pre' for l in _model(norm='pre').transformer.encoder.enc_layers)


def test_get_config_carries_the_key_only_when_pre():
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    for make in (lambda **kw: T.EncoderLayer(32, 2, 64, 0.1, **kw), lambda **kw: T.Encoder(1, 32, 2, 64, 0.1, **kw),
                 lambda **kw: T.Transformer(1, 2, {'items': 30}, {'items': 32}, 64, 0.1, **kw), _model):
        assert 'norm' not in make().get_config() and 'norm' not in make(norm='post').get_config()
        cfg = make(norm='pre').get_config()
        assert cfg['norm'] == 'pre'
        assert {k: v for k, v in cfg.items() if k != 'norm'}.keys() == make().get_config().keys()
    cfg = _model(norm='pre').get_config()
    cfg.pop('head_unit')
    again = _model(**{k: v for k, v in cfg.items() if k in ('norm',)})
    assert again.norm == 'pre'


def test_state_dict_names():
    post, pre = _model(), _model(norm='pre')
    names = list(post.state_dict().keys())
    assert not any('final_norm' in n for n in names)
    assert sum('layernorm' in n for n in names) == 2 * 2 * 2
    extra = ['transformer.encoder.final_norm.gamma', 'transformer.encoder.final_norm.beta']
    assert sorted(pre.state_dict().keys()) == sorted(names + extra)
    sd = pre.state_dict()
    for n in names:
        assert sd[n].shape == post.state_dict()[n].shape
    fn = pre.transformer.encoder.final_norm
    assert torch.equal(fn.gamma, torch.ones(64)) and torch.equal(fn.beta, torch.zeros(64)) and fn.gamma.dtype == torch.float32
    assert fn.epsilon == 1e-6
    # decayed by nothing: optim.no_decay_params already covers the two vectors
    from bert4clickpath_amd import optim
    nd = set(id(p) for p in optim.no_decay_params(pre))
    assert id(fn.gamma) in nd and id(fn.beta) in nd
    # a post-LN state dict does not load into a pre-LN model silently
    with pytest.raises(RuntimeError, match='final_norm'):
        pre.load_state_dict(post.state_dict())


def test_masked_query_route_answers_false_for_a_pre_ln_encoder(monkeypatch):
    from bert4clickpath_amd import ops
    from bert4clickpath_amd._lib import B4CError
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    for attention in ('bidirectional', 'causal'):
        enc = T.Encoder(2, 64, 2, 32, 0.1, attention=attention, norm='pre')
        post = T.Encoder(2, 64, 2, 32, 0.1, attention=attention)
        for training in (False, True):
            for a, b in ((False, False), (True, True)):
                monkeypatch.setattr(ops, 'mq_causal', a)
                monkeypatch.setattr(ops, 'mq_attn_dropout', b)
                assert enc.rows_supported(None, training) is False and enc.rows_route(None, training) is False
        monkeypatch.setattr(ops, 'mq_causal', True)
        assert post.rows_route(None, False) is True            # the post-LN answer is what it was
    rows = (torch.tensor([1], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32))
    with pytest.raises(B4CError, match='pre-LN'):
        T.Encoder(1, 64, 2, 32, 0.0, norm='pre')(torch.zeros(1, 4, 64), training=False, rows=rows)
    with pytest.raises(B4CError, match='pre-LN'):
        T.EncoderLayer(64, 2, 32, 0.0, norm='pre')(torch.zeros(1, 4, 64), training=False, rows=rows)


def test_background_dw_expected_of_a_pre_ln_model(monkeypatch):
    from bert4clickpath_amd import ops
    bf16, f32 = torch.bfloat16, torch.float32
    monkeypatch.setattr(ops, 'overlap_vocab_dw', None)
    monkeypatch.setattr(ops, 'fused_ffn_bwd', True)
    assert ops.background_dw_expected(128, 100, bf16) is False                      # the fused post-LN shape
    assert ops.background_dw_expected(128, 100, bf16, norm='post') is False
    assert ops.background_dw_expected(128, 100, bf16, norm='pre') is True           # ... answers as an unfused model does
    assert ops.background_dw_expected(128, 100, bf16, 'gelu', norm='pre') is True
    assert ops.background_dw_expected(256, 100, f32, norm='pre') is True
    for forced in (True, False):
        monkeypatch.setattr(ops, 'overlap_vocab_dw', forced)
        assert ops.background_dw_expected(128, 100, bf16, norm='pre') is forced
    with pytest.raises(ValueError, match='norm'):
        ops.background_dw_expected(128, 100, bf16, norm='both')


def test_a_pre_ln_step_sets_no_fused_blocks_flag_and_draws_the_post_ln_seeds(monkeypatch):
    """the halves stubbed (no GPU): the layer draws s1, s2 and s3 only with attention dropout, hands each tail the NEXT norm's
    parameters and the last one the encoder's final norm"""
    from bert4clickpath_amd import ops
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    seen = []

    class Attn:
        @staticmethod
        def apply(x2, *a):
            seen.append(('attn', a))
            return x2, a[10], a[11]

    class FFN:
        @staticmethod
        def apply(x2, *a):
            seen.append(('ffn', a))
            return x2, a[6], a[7]

    class Final:
        @staticmethod
        def apply(x2, gamma, beta, n, stats, training):
            seen.append(('final', (gamma, beta)))
            return n
    monkeypatch.setattr(ops, 'PreLNAttnBlockFn', Attn)
    monkeypatch.setattr(ops, 'PreLNFFNBlockFn', FFN)
    monkeypatch.setattr(ops, 'PreLNFinalNormFn', Final)
    monkeypatch.setattr(ops, 'layernorm_fwd', lambda x, g, b: (x, torch.zeros(x.shape[0], 2)))
    for a_rate, draws in ((0.0, 4), (0.2, 6)):
        del seen[:]
        enc = T.Encoder(2, 32, 2, 16, 0.1, attention_dropout_rate=a_rate, norm='pre')
        T.set_dropout_seed(3)
        out = enc(torch.zeros(2, 5, 32), training=True, mask=torch.zeros(2, 5, dtype=torch.uint8), _input_dropout_done=True)
        assert out.shape == (2, 5, 32) and T.dropout_seeds.counter == draws
        kinds = [k for k, _ in seen]
        assert kinds == ['attn', 'ffn', 'attn', 'ffn', 'final']
        l0, l1 = enc.enc_layers
        assert seen[0][1][8] is l0.layernorm1.gamma and seen[0][1][13] is l0.layernorm2.gamma        # own norm, next norm
        assert seen[1][1][4] is l0.layernorm2.gamma and seen[1][1][8] is l1.layernorm1.gamma
        assert seen[2][1][13] is l1.layernorm2.gamma
        assert seen[3][1][8] is enc.final_norm.gamma and seen[3][1][9] is enc.final_norm.beta
        assert seen[4][1][0] is enc.final_norm.gamma
        # the seeds are the post-LN layer's: the same stream gives a post-LN encoder the same draws in the same places
        T.set_dropout_seed(3)
        want = [T.dropout_seeds.next() for _ in range(draws)]
        per = draws // 2
        assert seen[0][1][21] == want[0] and seen[1][1][13] == want[1] and seen[2][1][21] == want[per]
        if a_rate:
            assert seen[0][1][25] == want[2] and seen[0][1][24] == a_rate
