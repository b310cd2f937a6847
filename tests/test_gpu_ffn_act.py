"""b4c_ffn_act_fwd / b4c_ffn_act_bwd: the feed-forward block with a GELU activation in one pass each way, against the kernels they
replace on the same inputs (forward: b4c_gemm_nt_act with `pre` + b4c_gemm_nt_add_ln; backward: the five kernels, the hidden gradient
gated by act'(u)) and against float64 (tests/paper_encoder_ref.py's act / act_grad), with the inputs and the bounds of
tests/test_gpu_ffn_fwd.py / test_gpu_ffn_bwd.py: the skeleton is the ReLU kernels' and the rounding points are the unfused route's
(u = bf16(x W1) + b1 and h = act(u), each to bf16; y = bf16(bf16(h W2) + b2); dz, dy in bf16, dh = bf16(bf16(dy W2^T) * act'(u))).  Then the model behind
ops.fused_ffn_gelu: the route it takes with the switch on and off, on against off, on against float64, bit-repeatable steps."""
import pytest
import torch

import fused_rows_ref as fr
import paper_encoder_ref as pr

pytestmark = pytest.mark.gpu

ACT_CODE = {'gelu': 2, 'gelu_tanh': 3}
# (M, F, rate): one-row last tile | some workgroups get a second tile | the four-stage ring wraps (7 tiles per workgroup forward, 13
# backward) | full width | Fp = 8: nearly every image column lies past the width | half width
SHAPES = [(4097, 100, 0.0), (19201, 100, 0.1), (100001, 100, 0.1), (8200, 128, 0.1), (5000, 8, 0.1), (8192, 64, 0.2)]
CASES = [(M, F, rate, act) for M, F, rate in SHAPES for act in (('gelu', 'gelu_tanh') if M in (19201, 5000) else ('gelu',))]


def _keep(M, seed, rate):
    from bert4clickpath_amd import ops
    return torch.from_numpy(ops.keep_mask(seed, M * 128, rate)).reshape(M, 128) if rate > 0 else torch.ones(M, 128, dtype=torch.bool)


# ---- forward ----------------------------------------------------------------------------------------------------------------
def _fwd_fused(a, act, rate, seed, save=True):
    from bert4clickpath_amd import ops
    return ops.ffn_act_fwd(a['x'], a['wt1'], a['b1'], a['wt2'], a['b2'], a['gamma'], a['beta'], a['F'], a['Fp'], ACT_CODE[act], rate, seed,
                           save=save)


def _fwd_two_kernels(a, act, rate, seed):
    from bert4clickpath_amd import ops
    u = torch.empty(a['x'].shape[0], a['Fp'], dtype=torch.bfloat16, device='cuda')
    h = ops.gemm_nt(a['x'], a['wt1'], a['Fp'], a['b1'], act=ACT_CODE[act], pre=u)
    z, out, stats = ops.gemm_nt_add_ln(h, a['wt2'], a['b2'], a['x'], a['gamma'], a['beta'], rate, seed, save=True)
    return h, u, z, out, stats


def _fwd_float64(a, act, rate, seed):
    return fr.ffn_fwd_float64(a, rate, seed, act=act)


@pytest.mark.parametrize('M,F,rate,act', CASES)
def test_fused_gelu_forward_against_the_two_kernels_and_float64(M, F, rate, act):
    from bert4clickpath_amd import ops
    from test_gpu_ffn_fwd import _inputs
    seed = 777 + M
    a = _inputs(M, F, seed)
    assert ops.ffn_fwd_supported(a['x'], a['Fp'])
    got = _fwd_fused(a, act, rate, seed)
    ref = _fwd_two_kernels(a, act, rate, seed)
    torch.cuda.synchronize()
    exact = _fwd_float64(a, act, rate, seed)
    u64 = exact[1][:, :F]
    assert float(u64.min()) < -2.5 and float(u64.max()) > 2.5          # both tails and the minimum of the GELU are in the test
    for n, g_, r_, e_ in zip(('h', 'u', 'z', 'out', 'stats'), got, ref, exact):
        g64, r64 = g_.double().cpu(), r_.double().cpu()
        scale = float(e_.abs().max()) + 1e-30
        err_g, err_r = float((g64 - e_).abs().max()) / scale, float((r64 - e_).abs().max()) / scale
        print('%s: fused %.3e two kernels %.3e apart %.3e (of the largest entry)' % (n, err_g, err_r, float((g64 - r64).abs().max()) / scale))
        if n == 'stats':
            assert err_g <= max(2.0 * err_r, 2e-3), (n, err_g, err_r)     # (mean, rstd of rows of bf16-rounded operands)
        else:
            assert err_g <= max(1.25 * err_r, 2 ** -7), (n, err_g, err_r)
            assert float((g64 - r64).abs().max()) <= 2 ** -6 * scale, n
    again = _fwd_fused(a, act, rate, seed)
    for g_, h_ in zip(got, again):
        assert torch.equal(g_, h_)
    # inference form: no z, no u, no stats, the same out
    h2, u2, z2, out2, st2 = _fwd_fused(a, act, rate, seed, save=False)
    assert z2 is None and u2 is None and st2 is None and torch.equal(out2, got[3]) and torch.equal(h2, got[0])


# ---- backward ---------------------------------------------------------------------------------------------------------------
def _bwd_inputs(M, F, seed, rate, act):
    """tests/test_gpu_ffn_bwd.py's draws, with h = act(u) and the saved u of a forward pass"""
    g = torch.Generator().manual_seed(seed)
    Fp = (F + 7) // 8 * 8
    x = torch.randn(M, 128, generator=g)
    w1 = torch.randn(128, F, generator=g) * 0.09
    b1 = torch.randn(F, generator=g) * 0.1
    w2 = torch.randn(F, 128, generator=g) * 0.1
    gamma = 1.0 + 0.1 * torch.randn(128, generator=g)
    dout = torch.randn(M, 128, generator=g) * 0.05
    xb, w1b, w2b = x.bfloat16(), w1.bfloat16(), w2.bfloat16()
    u, h = torch.zeros(M, Fp), torch.zeros(M, Fp)
    u[:, :F] = xb.float() @ w1b.float() + b1
    h[:, :F] = pr.act(act, u[:, :F].double()).float()
    ub, hb = u.bfloat16(), h.bfloat16()
    y = hb[:, :F].float() @ w2b.float()
    keep = _keep(M, seed, rate)
    z = (xb.float() + torch.where(keep, y / (1.0 - rate), torch.zeros(()))).bfloat16()
    zf = z.float()
    stats = torch.stack([zf.mean(1), 1.0 / torch.sqrt(zf.var(1, unbiased=False) + 1e-6)], 1).contiguous()
    wc1 = torch.zeros(128, Fp)
    wc1[:, :F] = w1b.float()                  # row = input feature, k = hidden column
    wc2 = torch.zeros(Fp, 128)
    wc2[:F] = w2b.float()                     # row = hidden column, k = output column
    dev = lambda t, dt=torch.bfloat16: t.to(dt).cuda().contiguous()
    return dict(dout=dev(dout), z=dev(z), stats=stats.cuda(), gamma=gamma.cuda(), h=dev(hb), u=dev(ub), x=dev(xb), wc2=dev(wc2),
                wc1=dev(wc1), F=F, Fp=Fp, keep=keep)


def _zeros(F, fill=(0.0,) * 6):
    return [torch.full(s, v, device='cuda') for s, v in zip(((128, F), (F,), (F, 128), (128,), (128,), (128,)), fill)]


def _bwd_fused(a, act, rate, seed, sinks=None, u=None):
    from bert4clickpath_amd import ops
    dW1, db1, dW2, db2, dgamma, dbeta = sinks if sinks is not None else _zeros(a['F'])
    assert ops.ffn_bwd_supported(a['x'], a['h'], a['z'])
    dx = ops.ffn_act_bwd(a['dout'], a['z'], a['stats'], a['gamma'], rate, seed, ACT_CODE[act], a['h'], a['u'] if u is None else u, a['x'],
                         a['wc2'], a['wc1'], a['F'], dW1, db1, dW2, db2, dgamma, dbeta)
    return dx, dW1, db1, dW2, db2, dgamma, dbeta


def _bwd_five_kernels(a, act, rate, seed):
    from bert4clickpath_amd import ops
    F, Fp = a['F'], a['Fp']
    dz, dy, dgamma, dbeta = ops.add_dropout_layernorm_bwd(a['dout'], a['z'], a['stats'], a['gamma'], rate, seed)
    dW2, db2 = ops.gemm_tn(a['h'], dy, F, 128)
    dh = ops.gemm_nt(dy, a['wc2'], Fp, gate=a['u'], gate_act=ACT_CODE[act])
    dW1, db1 = ops.gemm_tn(a['x'], dh, 128, F)
    dx = ops.gemm_nt(dh, a['wc1'], 128, residual=dz)
    return dx, dW1, db1, dW2, db2, dgamma, dbeta


def _bwd_float64(a, act, rate):
    return fr.ffn_bwd_float64(a, rate, act=act)


NAMES = ('dx', 'dW1', 'db1', 'dW2', 'db2', 'dgamma', 'dbeta')


@pytest.mark.parametrize('M,F,rate,act', CASES)
def test_fused_gelu_backward_against_the_five_kernels_and_float64(M, F, rate, act):
    """The bounds are tests/test_gpu_ffn_bwd.py's, which rest on both routes rounding at the same points.  b4c_gemm_nt's bf16
    epilogue stages its accumulators as bf16 before bias, activation and gate: the five-kernel route holds
    dh = bf16(bf16(dy W2^T) * act'(u)), two roundings, and the fused kernel rounds there too.  (A first form of the kernel rounded
    the fp32 product once.  Measured on the first case: dW1 3.1e-3 of its largest entry away from the five kernels, over the
    2e-3 held here, both routes 2.5e-3 / 3.0e-3 from float64.)"""
    seed = 1234 + M
    a = _bwd_inputs(M, F, seed, rate, act)
    u64 = a['u'].double().cpu()[:, :F]
    assert float(u64.min()) < -2.5 and float(u64.max()) > 2.5
    got = _bwd_fused(a, act, rate, seed)
    ref = _bwd_five_kernels(a, act, rate, seed)
    torch.cuda.synchronize()
    exact = _bwd_float64(a, act, rate)
    for n, g_, r_, e_ in zip(NAMES, got, ref, exact):
        g64, r64 = g_.double().cpu(), r_.double().cpu()
        scale = float(e_.abs().max()) + 1e-30
        err_g, err_r = float((g64 - e_).abs().max()) / scale, float((r64 - e_).abs().max()) / scale
        print('%s: fused %.3e five kernels %.3e apart %.3e (of the largest entry) mean apart %.3e (of the mean entry)' % (
            n, err_g, err_r, float((g64 - r64).abs().max()) / scale, float((g64 - r64).abs().mean()) / float(e_.abs().mean())))
        if n == 'dx':
            # bf16 output of sums of bf16-rounded intermediates: both routes sit a few bf16 steps from float64, and next to each other
            assert err_g <= max(1.25 * err_r, 2 ** -7), (n, err_g, err_r)
            assert float((g64 - r64).abs().max()) <= 2 ** -7 * scale, n
            assert float((g64 - r64).abs().mean()) <= 2 ** -9 * float(e_.abs().mean()), n     # (half a bf16 step on average)
        else:
            # fp32 sums over M rows of bf16-rounded intermediates: the fused route is no further from float64 than the five kernels
            assert err_g <= max(1.5 * err_r, 1e-4), (n, err_g, err_r)
            assert float((g64 - r64).abs().max()) <= 2e-3 * scale, n
    again = _bwd_fused(a, act, rate, seed)
    for n, g_, h_ in zip(NAMES, got, again):
        assert torch.equal(g_, h_), n         # no float atomics: two runs, the same bits
    if M == 5000:
        # the width hazard: u with a row pitch above Fp and NaN in the gap -- the image's columns past Fp hold the gap, and the gate
        # must not form 0 * act'(NaN).  The same bits as with the contiguous u.
        wide = torch.full((M, a['Fp'] + 8), float('nan'), dtype=torch.bfloat16, device='cuda')
        wide[:, :a['Fp']] = a['u']
        pitched = _bwd_fused(a, act, rate, seed, u=wide[:, :a['Fp']])
        for n, g_, h_ in zip(NAMES, got, pitched):
            assert torch.equal(g_, h_), n


def test_accumulates_into_existing_gradients():
    M, F, rate, seed, act = 6000, 100, 0.1, 9, 'gelu'
    a = _bwd_inputs(M, F, seed, rate, act)
    base = _bwd_fused(a, act, rate, seed)
    fill = (2.0, 3.0, -1.0, 0.5, 7.0, -7.0)
    into = _bwd_fused(a, act, rate, seed, sinks=_zeros(F, fill))
    for got, start, ref in zip(into[1:], fill, base[1:]):
        assert torch.allclose(got, ref + start, rtol=1e-6, atol=1e-6)


# ---- the model ----------------------------------------------------------------------------------------------------------------
V, D, LAYERS, HEADS, B, S = 1000, 128, 2, 2, 24, 200
FAMILIES = ('ffn_fwd', 'ffn_bwd', 'ffn_act_fwd', 'ffn_act_bwd', 'attn_out_bwd')


def _step(ops, model, opt, items, labels):
    opt.zero_grad()
    loss = model.cloze_loss({'asin': items}, labels, training=True, packed=False)
    loss.backward()
    ops.flush_pending_dw(opt.arena.ctx)
    ops.join_side_work(opt.arena.ctx)
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


@pytest.fixture(scope='module')
def model_runs():
    """one training step of the same GELU model (d 128, dff 100, 2 layers, 24 x 200 token rows, bf16, gradients in the optimizer's
    arena) with the switch off and on: {flag: (loss, gradients, call counts, fused_blocks, recorder, model)}"""
    from bert4clickpath_amd import ops, optim
    from bf16_gates import GateRecorder
    from test_gpu_gelu import _batch, _build, _count_calls
    b, ids, items, labels = _batch(B, S, V, 13, min_len=150)
    prev, runs = ops.fused_ffn_gelu, {}
    try:
        for flag in (False, True):
            ops.fused_ffn_gelu = flag
            model = _build(V, D, LAYERS, HEADS, [64, 128], torch.bfloat16, 11, ffn_activation='gelu')
            opt = optim.Adam(model.parameters())
            with GateRecorder(ops) as rec:
                calls, orig = _count_calls(ops, FAMILIES)
                try:
                    loss, grads = _step(ops, model, opt, items, labels)
                finally:
                    for n in FAMILIES:
                        setattr(ops, n, orig[n])
            runs[flag] = (loss, grads, dict(calls), opt.arena.ctx.fused_blocks, rec, model)
    finally:
        ops.fused_ffn_gelu = prev
    return dict(runs=runs, batch=(b, ids, items, labels))


def test_model_route_with_the_switch_on_and_off(model_runs):
    from bert4clickpath_amd import ops
    on, off = model_runs['runs'][True], model_runs['runs'][False]
    print('calls on', on[2], 'off', off[2])
    assert on[2]['ffn_act_fwd'] >= 1 and on[2]['ffn_act_bwd'] >= 1
    assert on[2]['ffn_fwd'] == 0 and on[2]['ffn_bwd'] == 0
    assert on[3] is True
    # off: what tests/test_gpu_gelu.py asserts of a GELU model
    assert off[2]['ffn_fwd'] == 0 and off[2]['ffn_bwd'] == 0 and off[2]['ffn_act_fwd'] == 0 and off[2]['ffn_act_bwd'] == 0
    assert off[3] is False
    assert on[2]['attn_out_bwd'] == off[2]['attn_out_bwd'] >= 1
    prev = ops.fused_ffn_gelu
    try:
        for flag in (False, True):
            ops.fused_ffn_gelu = flag
            if ops.overlap_vocab_dw is None:
                assert ops.background_dw_expected(D, 100, torch.bfloat16, 'gelu') is (not model_runs['runs'][flag][3])
    finally:
        ops.fused_ffn_gelu = prev


def test_model_step_on_against_off(model_runs):
    """Loss within 2e-3 and every gradient tensor within 3e-2 (L2) of the unfused step's, the bounds tests/test_gpu_ffn_fwd.py
    holds the ReLU model to.  (Measured: 0.13 % at most, the key biases aside, with the unfused route's rounding points in both
    kernels; 1.7 - 4.1 % with y kept in fp32 in the forward's row phase -- on 24 sequences the bf16 steps of z that this moves are
    worth that much, through the ReLU gates of the head's trunk among others.)"""
    (loss_on, g_on), (loss_off, g_off) = model_runs['runs'][True][:2], model_runs['runs'][False][:2]
    assert abs(float(loss_on) - float(loss_off)) <= 2e-3 * abs(float(loss_off))
    floor = 1e-6 * max(float(g.float().abs().max()) for g in g_off.values())     # (tests/test_gpu_ffn_fwd.py's floor)
    for n, gd in g_off.items():
        print('%-60s on - off %.2f %% (L2)' % (n, 100 * float((g_on[n].float() - gd.float()).norm()) / max(float(gd.float().norm()), 1e-30)))
    for n, gd in g_off.items():
        gd, gf = gd.float(), g_on[n].float()
        assert float((gf - gd).norm()) <= 3e-2 * float(gd.norm()) + floor * gd.numel() ** 0.5, n


def test_model_step_on_against_float64(model_runs):
    from bf16_gates import BF16_GRAD_BOUND, grad_errors
    loss, _, _, _, rec, model = model_runs['runs'][True]
    b, ids, items, labels = model_runs['batch']
    rec.patterns = [None] * LAYERS + [p for p in rec.patterns]         # (no ReLU in the encoder: the head trunk's patterns only)
    relu = rec.relu_for(LAYERS, 2, torch.from_numpy(b['flat_idx']).long(), B, S)
    Pt = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    ref, _ = pr.model_loss(ids, torch.from_numpy(b['labels']).long(), Pt, LAYERS, HEADS, 2, ffn='gelu', relu=relu)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 2e-3 * float(ref)
    errs = grad_errors(model.named_parameters(), {n: Pt[n].grad for n, _ in model.named_parameters()})
    for n, e in errs.items():
        print('%-60s on - float64 %.2f %% (L2)' % (n, 100 * e))
    name, err = max(errs.items(), key=lambda kv: kv[1])
    print('worst gradient tensor %s %.2f %%' % (name, 100 * err))
    assert err < BF16_GRAD_BOUND, (name, err)


def test_dropout_steps_with_the_switch_on_are_bit_identical():
    from bert4clickpath_amd import ops, optim
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    from test_gpu_gelu import _batch, _build, _count_calls
    b, ids, items, labels = _batch(B, S, V, 3, min_len=150)
    prev, out = ops.fused_ffn_gelu, []
    calls, orig = _count_calls(ops, ('ffn_act_fwd', 'ffn_act_bwd'))
    try:
        ops.fused_ffn_gelu = True
        model = _build(V, D, LAYERS, HEADS, [64], torch.bfloat16, 5, dropout=0.1, ffn_activation='gelu_tanh')
        opt = optim.Adam(model.parameters())
        for _ in range(2):
            T.set_dropout_seed(99)
            out.append(_step(ops, model, opt, items, labels))
    finally:
        ops.fused_ffn_gelu = prev
        for n, f in orig.items():
            setattr(ops, n, f)
    assert calls['ffn_act_fwd'] >= 2 and calls['ffn_act_bwd'] >= 2
    assert torch.equal(out[0][0], out[1][0]) and float(out[0][0]) > 0
    for n in out[0][1]:
        assert torch.equal(out[0][1][n], out[1][1][n]), n
