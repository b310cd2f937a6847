"""GELU in the position-wise feed-forward block (ffn_activation='gelu' | 'gelu_tanh'; NO REFERENCE ORACLE: an extension -- the
float64 restatement is tests/paper_encoder_ref.py): the GEMM epilogue's two activations, its `pre` output and its derivative
gate (b4c_gemm_nt_act) against float64, and the model behind the public keyword against float64 autograd, with the route a GELU
model takes (never the fused ReLU kernels)."""
import pytest
import torch

import paper_encoder_ref as pr

pytestmark = pytest.mark.gpu

# (partial row tile, N = the padded dff of the reference), (several tiles), (one chunk), (N % 8 != 0: the scalar epilogue)
SHAPES = [(37, 104, 128), (300, 512, 128), (1, 8, 8), (129, 50, 64)]
DT = [torch.float32, torch.bfloat16]
ACTS = ['gelu', 'gelu_tanh']
# tests/test_gpu_kernels.py holds the act = NONE launch to TOL x max|want|; a GELU (sup |gelu'| = 1.129) may stretch that error by
# 1.13, and the output is rounded once more to its type (half an ulp: 2^-24 fp32, 2^-9 bf16)
TOL = {torch.float32: 2e-5, torch.bfloat16: 1.2e-2}
EPS_OUT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -9}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops as o
    return o


def _operands(M, N, K, dtype):
    """A [M, K], Bt [N, K], bias [N], gate [M, N] on the device; A Bt^T + bias and the gate have a standard deviation of ~1.6:
    values span about [-4, 4] -- both tails of the GELU and its minimum near -0.75"""
    g = torch.Generator().manual_seed(M * 131 + N * 7 + K)
    a = torch.randn(M, K, generator=g)
    bt = torch.randn(N, K, generator=g) * (1.55 / K ** 0.5)
    bias = torch.randn(N, generator=g) * 0.4
    gate = torch.randn(M, N, generator=g) * 1.6
    return a.to(dtype).cuda(), bt.to(dtype).cuda(), bias.cuda(), gate.to(dtype).cuda()


def _bound(dtype, linear, want):
    return 1.13 * TOL[dtype] * float(linear.abs().max()) + EPS_OUT[dtype] * float(want.abs().max())


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('M,N,K', SHAPES)
def test_epilogue_activation_and_pre_output(ops, M, N, K, dtype, act):
    code = ops.ffn_act_code(act)
    a, bt, bias, _ = _operands(M, N, K, dtype)
    u64 = a.double().cpu() @ bt.double().cpu().T + bias.double().cpu()
    want = pr.act(act, u64)
    h = ops.gemm_nt(a, bt, N, bias, act=code)
    err = float((h.double().cpu() - want).abs().max())
    print('act %s %s %s: err %.3e bound %.3e' % (act, dtype, (M, N, K), err, _bound(dtype, u64, want)))
    assert err <= _bound(dtype, u64, want)
    if M > 1:
        assert float(u64.min()) < -2.5 and float(u64.max()) > 2.5          # the tails are in the test
    # the pre-activation output: what the plain launch writes, bit for bit; C is the same with it
    pre = torch.full((M, N), float('nan'), dtype=dtype, device='cuda')
    h2 = ops.gemm_nt(a, bt, N, bias, act=code, pre=pre)
    plain = ops.gemm_nt(a, bt, N, bias)
    assert torch.equal(pre, plain)
    assert torch.equal(h2, h)


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('M,N,K', SHAPES)
def test_derivative_gate(ops, M, N, K, dtype, act):
    code = ops.ffn_act_code(act)
    dy, w2c, _, u = _operands(M, N, K, dtype)
    lin = dy.double().cpu() @ w2c.double().cpu().T
    want = lin * pr.act_grad(act, u.double().cpu())
    got = ops.gemm_nt(dy, w2c, N, gate=u, gate_act=code)
    err = float((got.double().cpu() - want).abs().max())
    print('gate %s %s %s: err %.3e bound %.3e' % (act, dtype, (M, N, K), err, _bound(dtype, lin, want)))
    assert err <= _bound(dtype, lin, want)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('M,N,K', SHAPES)
def test_relu_gate_of_the_new_entry_point_is_the_old_one(ops, M, N, K, dtype):
    from bert4clickpath_amd import _lib as L
    dy, w2c, _, u = _operands(M, N, K, dtype)
    old = ops.gemm_nt(dy, w2c, N, gate=u)
    new = torch.empty(M, N, dtype=dtype, device='cuda')
    L.check(L.lib().b4c_gemm_nt_act(dy.data_ptr(), dy.stride(0), w2c.data_ptr(), w2c.stride(0), new.data_ptr(), new.stride(0), M, N, K,
                                    None, L.ACT_NONE, u.data_ptr(), u.stride(0), L.ACT_RELU, None, 0, None, 0,
                                    ops.dt_code(dtype), ops.dt_code(dtype), ops._st()), 'gemm_nt_act')
    assert torch.equal(old, new)


# ---- the model ------------------------------------------------------------------------------------------------------------
def _build(V, d, L, H, head_dims, dtype, seed, dropout=0.0, **kw):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(seed)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': d}, SoftMaxHead(list(head_dims), V),
                               value_to_head='[MASK]', num_encoder_layers=L, num_attention_heads=H, dropout_rate=dropout,
                               compute_dtype=dtype, **kw)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias') or n.endswith('beta'):
                p.normal_(0, 0.05)
            if n.endswith('gamma'):
                p.add_(torch.randn_like(p) * 0.05)
    return m.cuda()


def _batch(B, S, V, seed, min_len=4):
    from bert4clickpath_amd import input_pipeline
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=seed, min_len=min_len)
    ids = torch.from_numpy(b['ids'])
    return b, ids, ids[:, 2:S - 1].contiguous().cuda(), torch.from_numpy(b['labels_padded']).cuda()


@pytest.mark.parametrize('act', ACTS)
def test_model_fp32_matches_float64(ops, act):
    """Loss and every parameter gradient of cloze_loss against float64 autograd, with the tolerances tests/test_gpu_model.py holds
    the ReLU model of this kind to (loss 2e-5, gradients 2e-4 of the tensor's largest entry).  On a tree without the feature the
    keyword is swallowed and the model computes ReLU: the comparison fails."""
    V, d, L, H, B, S = 50, 32, 2, 2, 3, 12
    model = _build(V, d, L, H, [24, 16], torch.float32, 7, ffn_activation=act)
    b, ids, items, labels = _batch(B, S, V, 7)
    assert len(set((b['ids'] != 0).sum(1).tolist())) > 1          # ragged
    loss = model.cloze_loss({'asin': items}, labels, training=True)
    loss.backward()
    Pt = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    ref, _ = pr.model_loss(ids, torch.from_numpy(b['labels']).long(), Pt, L, H, 2, ffn=act)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 2e-5
    for name, p in model.named_parameters():
        gr = Pt[name].grad
        if float(gr.abs().max()) < 1e-9:       # the key bias (softmax shift invariance): rounding noise on both sides
            assert float(p.grad.abs().max()) < 1e-6, name
            continue
        err = float((p.grad.cpu().double() - gr).abs().max() / gr.abs().max())
        assert err < 2e-4, (name, err)
    relu = _build(V, d, L, H, [24, 16], torch.float32, 7)
    relu.load_state_dict(model.state_dict())
    relu_loss = float(relu.cloze_loss({'asin': items}, labels, training=False))
    assert abs(relu_loss - float(loss)) > 1e-3, (relu_loss, float(loss))        # the keyword changed the network


def _count_calls(ops, names):
    calls = {n: 0 for n in names}
    orig = {n: getattr(ops, n) for n in names}

    def wrap(n):
        def counted(*a, **k):
            calls[n] += 1
            return orig[n](*a, **k)
        return counted
    for n in names:
        setattr(ops, n, wrap(n))
    return calls, orig


def test_model_bf16_route_and_float64(ops):
    """d_model 128, dff 100, 24 x 200 = 4,800 token rows (the fused kernels' threshold is 4,096), gradients in the optimizer's arena:
    the ReLU model takes b4c_ffn_fwd / b4c_ffn_bwd, the GELU model never does and keeps the fused attention tail (b4c_attn_out_bwd).
    Loss (2e-3) and gradients (bf16_gates.BF16_GRAD_BOUND, L2 per tensor, the head trunk's ReLU patterns shared with the device pass)
    against float64, exact and with the path's bf16 rounding points emulated -- the gates of the ReLU model tests of this shape; a GELU
    has no on / off pattern of its own to share.  The GELU needed no wider gate."""
    from bert4clickpath_amd import optim
    from bf16_gates import BF16_GRAD_BOUND, GateRecorder, grad_errors
    V, d, L, H, B, S = 1000, 128, 2, 2, 24, 200
    b, ids, items, labels = _batch(B, S, V, 13, min_len=150)
    names = ('ffn_fwd', 'ffn_bwd', 'attn_out_bwd')
    counts = {}
    for act in ('relu', 'gelu'):
        model = _build(V, d, L, H, [64, 128], torch.bfloat16, 11, ffn_activation=act)
        opt = optim.Adam(model.parameters())
        opt.zero_grad()
        with GateRecorder(ops) as rec:
            calls, orig = _count_calls(ops, names)
            try:
                loss = model.cloze_loss({'asin': items}, labels, training=True, packed=False)
                loss.backward()
                ops.flush_pending_dw(opt.arena.ctx)
                ops.join_side_work(opt.arena.ctx)
                torch.cuda.synchronize()
            finally:
                for n in names:
                    setattr(ops, n, orig[n])
        counts[act] = dict(calls)
        assert opt.arena.ctx.fused_blocks == (act == 'relu')
        if act == 'relu':
            continue
        rec.patterns = [None] * L + [p for p in rec.patterns]           # (no ReLU in the encoder: the head trunk's patterns only)
        relu = rec.relu_for(L, 2, torch.from_numpy(b['flat_idx']).long(), B, S)
        for what, kw in (('fp64 + device gates', {}), ('bf16-emulating + device gates', {'emulate_bf16': True})):
            Pt = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
            ref, _ = pr.model_loss(ids, torch.from_numpy(b['labels']).long(), Pt, L, H, 2, ffn=act, relu=relu, **kw)
            ref.backward()
            assert abs(float(loss) - float(ref)) < 2e-3 * float(ref), what
            errs = grad_errors(model.named_parameters(), {n: Pt[n].grad for n, _ in model.named_parameters()})
            name, err = max(errs.items(), key=lambda kv: kv[1])
            print('%s: worst gradient tensor %s %.2f %%' % (what, name, 100 * err))
            assert err < BF16_GRAD_BOUND, (what, name, err)
    print('calls', counts)
    assert counts['gelu']['ffn_fwd'] == 0 and counts['gelu']['ffn_bwd'] == 0
    assert counts['relu']['ffn_fwd'] >= 1 and counts['relu']['ffn_bwd'] >= 1
    assert counts['gelu']['attn_out_bwd'] == counts['relu']['attn_out_bwd'] >= 1


def test_dropout_step_is_bit_repeatable(ops):
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    V, d, L, H, B, S = 300, 128, 2, 2, 8, 40
    model = _build(V, d, L, H, [64], torch.bfloat16, 5, dropout=0.1, ffn_activation='gelu_tanh')
    b, ids, items, labels = _batch(B, S, V, 3)
    out = []
    for _ in range(2):
        model.zero_grad()
        T.set_dropout_seed(99)
        loss = model.cloze_loss({'asin': items}, labels, training=True)
        loss.backward()
        out.append((loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}))
    assert torch.equal(out[0][0], out[1][0]) and float(out[0][0]) > 0
    for n in out[0][1]:
        assert torch.equal(out[0][1][n], out[1][1][n]), n


def test_packed_and_dense_layouts_agree(ops):
    """as tests/test_gpu_packed.py holds the ReLU model: loss within 2e-3, gradients within 6 % (two bf16 evaluations of one math)"""
    V, d, L, H, B, S = 300, 64, 2, 2, 12, 48
    model = _build(V, d, L, H, [32, 64], torch.bfloat16, 3, ffn_activation='gelu')
    b, ids, items, labels = _batch(B, S, V, 21, min_len=3)
    n_real = int((b['ids'] != 0).sum())

    def run(**kw):
        model.zero_grad()
        loss = model.cloze_loss({'asin': items}, labels, training=True, max_masked_per_row=10, **kw)
        loss.backward()
        return float(loss), {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    l_dense, g_dense = run(packed=False)
    l_pack, g_pack = run(n_real_tokens=n_real)
    assert model._packed is not None and model._packed.T == n_real
    assert abs(l_pack - l_dense) < 2e-3 * abs(l_dense)
    for n in g_dense:
        if float(g_dense[n].float().norm()) < 1e-9 or n.endswith('mha.wk.bias'):
            continue
        err = float((g_pack[n].double() - g_dense[n].double()).abs().max() / g_dense[n].double().abs().max())
        assert err < 0.06, (n, err)
