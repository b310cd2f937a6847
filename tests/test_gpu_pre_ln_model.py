"""The pre-LN model behind the public keyword norm='pre' (NO REFERENCE ORACLE: an extension -- the float64 restatement is
tests/pre_ln_ref.py, itself checked against torch's norm_first layer in tests/test_pre_ln_cpu.py), with the shapes and tolerances
of tests/test_gpu_gelu.py's model tests: fp32 loss 2e-5 and gradients 2e-4 of the tensor's largest entry; bf16 loss 2e-3 relative
and gradients at bf16_gates.BF16_GRAD_BOUND with the device pass's ReLU patterns shared.  Pre-LN adds no rounding step that
post-LN lacks."""
import os

import numpy as np
import pytest
import torch

import pre_ln_ref as plr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops as o
    return o


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


def _compare_fp32(model, loss, ref, Pt):
    assert abs(float(loss.detach()) - float(ref.detach())) < 2e-5, (float(loss), float(ref))
    worst = 0.0
    for name, p in model.named_parameters():
        gr = Pt[name].grad
        assert p.grad is not None, name
        if float(gr.abs().max()) < 1e-9:       # the key bias (softmax shift invariance): rounding noise on both sides
            assert float(p.grad.abs().max()) < 1e-6, name
            continue
        err = float((p.grad.cpu().double() - gr).abs().max() / gr.abs().max())
        worst = max(worst, err)
        assert err < 2e-4, (name, err)
    return worst


# ---- fp32 against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', ['relu', 'gelu_tanh'])
@pytest.mark.parametrize('attention', ['bidirectional', 'causal'])
def test_model_fp32_matches_float64(ops, attention, act):
    """two layers, head depth 16, cloze_loss; the post-LN model of the same weights computes something else"""
    V, d, L, H, B, S = 50, 32, 2, 2, 3, 12
    kw = {'attention': attention} if attention == 'causal' else {}
    model = _build(V, d, L, H, [24, 16], torch.float32, 7, ffn_activation=act, norm='pre', **kw)
    b, ids, items, labels = _batch(B, S, V, 7)
    assert len(set((b['ids'] != 0).sum(1).tolist())) > 1          # ragged
    loss = model.cloze_loss({'asin': items}, labels, training=True)
    loss.backward()
    Pt = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    ref, _ = plr.model_loss(ids, torch.from_numpy(b['labels']).long(), Pt, L, H, 2, ffn=act, causal=attention == 'causal')
    ref.backward()
    worst = _compare_fp32(model, loss, ref, Pt)
    print('pre-LN fp32 %s %s: loss %.6f float64 %.6f, worst gradient %.2e' % (attention, act, float(loss), float(ref), worst))
    assert float(Pt['transformer.encoder.final_norm.gamma'].grad.abs().max()) > 1e-6
    post = _build(V, d, L, H, [24, 16], torch.float32, 7, ffn_activation=act, **kw)
    post.load_state_dict(model.state_dict(), strict=False)
    post_loss = float(post.cloze_loss({'asin': items}, labels, training=False))
    assert abs(post_loss - float(loss)) > 1e-3, (post_loss, float(loss))        # the keyword changed the network


def test_model_fp32_with_every_dropout_mask_regenerated(ops):
    """head depth 32, dropout 0.1 on the residual branches and 0.2 on the attention probabilities, the masks regenerated on the host in
    the order the post-LN layer draws its seeds (embedding; per layer s1, s2, s3), and the reference's own composition
    loss(y, model(x)) beside cloze_loss"""
    from bert4clickpath_amd.cloze import ClozeMaskedLoss
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    from bert4clickpath_amd.clickstream_transformer.losses import sparse_categorical_crossentropy
    V, d, L, H, B, S, rate, a_rate = 60, 64, 2, 2, 4, 16, 0.1, 0.2
    model = _build(V, d, L, H, [24, 16], torch.float32, 7, dropout=rate, attention_dropout_rate=a_rate, norm='pre')
    b, ids, items, labels = _batch(B, S, V, 7)

    def masks():
        stream = T._SeedStream(2025)
        n = B * S * d
        keep = {'emb': torch.from_numpy(ops.keep_mask(stream.next(), n, rate)).view(B, S, d)}
        keep_attn = []
        for i in range(L):
            keep['l%d.1' % i] = torch.from_numpy(ops.keep_mask(stream.next(), n, rate)).view(B, S, d)
            keep['l%d.2' % i] = torch.from_numpy(ops.keep_mask(stream.next(), n, rate)).view(B, S, d)
            keep_attn.append(ops.attn_keep_mask(stream.next(), B, H, S, a_rate))
        return keep, keep_attn, stream.counter
    keep, keep_attn, draws = masks()
    for form in ('cloze_loss', 'loss(y, model(x))'):
        model.zero_grad()
        T.set_dropout_seed(2025)
        if form == 'cloze_loss':
            loss = model.cloze_loss({'asin': items}, labels, training=True)
        else:
            loss = ClozeMaskedLoss(sparse_categorical_crossentropy)(labels, model({'asin': items}, training=True))
        assert T.dropout_seeds.counter == draws == 1 + 3 * L
        loss.backward()
        Pt = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
        ref, _ = plr.model_loss(ids, torch.from_numpy(b['labels']).long(), Pt, L, H, 2, dropout_rate=rate, keep_masks=keep,
                                attn_rate=a_rate, keep_attn=keep_attn)
        ref.backward()
        worst = _compare_fp32(model, loss, ref, Pt)
        print('pre-LN fp32 dropout, %s: loss %.6f float64 %.6f, worst gradient %.2e' % (form, float(loss), float(ref), worst))


# ---- bf16 against float64, both forms of the input-gradient step ----------------------------------------------------------------------
def test_model_bf16_matches_float64_on_every_input_gradient_form(ops, monkeypatch):
    """d_model 128, dff 100, 24 x 200 = 4,800 token rows, gradients in the optimizer's arena (tests/test_gpu_gelu.py's bf16 model):
    the size at which all three forms of the input-gradient step exist (ops.pre_ln_input_bwd), forced in turn.  No persistent post-LN kernel runs and
    the arena's fused_blocks flag stays off."""
    from bert4clickpath_amd import optim
    from bf16_gates import BF16_GRAD_BOUND, GateRecorder, grad_errors
    V, d, L, H, B, S = 1000, 128, 2, 2, 24, 200
    b, ids, items, labels = _batch(B, S, V, 13, min_len=150)
    names = ('ffn_fwd', 'ffn_bwd', 'attn_out_bwd', 'ffn_act_fwd', 'ffn_act_bwd', 'gemm_dxdw', 'layernorm_bwd_add', 'gemm_nt_ln_bwd_add')
    for form in ops.PRE_LN_INPUT_BWD_FORMS:
        monkeypatch.setattr(ops, 'pre_ln_input_bwd', form)
        model = _build(V, d, L, H, [64, 128], torch.bfloat16, 11, norm='pre')
        opt = optim.Adam(model.parameters())
        opt.zero_grad()
        calls = {n: 0 for n in names}
        for n in names:
            def counted(*a, _n=n, _f=getattr(ops, n), **k):
                calls[_n] += 1
                return _f(*a, **k)
            monkeypatch.setattr(ops, n, counted)
        with GateRecorder(ops) as rec:
            loss = model.cloze_loss({'asin': items}, labels, training=True, packed=False)
            loss.backward()
            ops.flush_pending_dw(opt.arena.ctx)
            ops.join_side_work(opt.arena.ctx)
            torch.cuda.synchronize()
        monkeypatch.undo()
        print('form %s calls %s' % (form, calls))
        assert not opt.arena.ctx.fused_blocks and not rec.rows_only_last
        assert calls['ffn_fwd'] == calls['ffn_bwd'] == calls['attn_out_bwd'] == calls['ffn_act_fwd'] == calls['ffn_act_bwd'] == 0
        assert calls['layernorm_bwd_add'] == (0 if form == 'fused' else 2 * L) and calls['gemm_nt_ln_bwd_add'] == (2 * L if form == 'fused' else 0)
        assert calls['gemm_dxdw'] == (2 * L if form == 'dxdw' else L)            # the output projection takes it in either form
        relu = rec.relu_for(L, 2, torch.from_numpy(b['flat_idx']).long(), B, S)
        Pt = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
        ref, _ = plr.model_loss(ids, torch.from_numpy(b['labels']).long(), Pt, L, H, 2, relu=relu)
        ref.backward()
        rec.check_flips()
        assert abs(float(loss) - float(ref)) < 2e-3 * float(ref), form
        errs = grad_errors(model.named_parameters(), {n: Pt[n].grad for n, _ in model.named_parameters()})
        name, err = max(errs.items(), key=lambda kv: kv[1])
        print('pre-LN bf16, form %s: loss %.6f float64 %.6f, worst gradient tensor %s %.2f %%' % (form, float(loss), float(ref), name, 100 * err))
        assert err < BF16_GRAD_BOUND, (form, name, err)


def test_packed_and_dense_layouts_agree(ops):
    """as tests/test_gpu_gelu.py holds its model: loss within 2e-3, gradients within 6 % (two bf16 evaluations of one math)"""
    V, d, L, H, B, S = 300, 64, 2, 2, 12, 48
    model = _build(V, d, L, H, [32, 64], torch.bfloat16, 3, ffn_activation='gelu', norm='pre')
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


def test_dropout_step_is_bit_repeatable(ops):
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    V, d, L, H, B, S = 300, 128, 2, 2, 8, 40
    model = _build(V, d, L, H, [64], torch.bfloat16, 5, dropout=0.1, attention_dropout_rate=0.1, ffn_activation='gelu_tanh', norm='pre')
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


def test_arena_and_plain_gradient_sinks_give_identical_bits(ops):
    """below 4,096 rows the arena opens no other route (no grouped dW queue, no b4c_gemm_dxdw): the same launches add into .grad
    views of the arena or into fresh zeros that autograd receives"""
    from bert4clickpath_amd import optim
    V, d, L, H, B, S = 200, 64, 2, 2, 6, 24
    b, ids, items, labels = _batch(B, S, V, 5)
    grads = []
    for arena in (False, True):
        model = _build(V, d, L, H, [32], torch.bfloat16, 4, norm='pre')
        if arena:
            opt = optim.Adam(model.parameters())
            opt.zero_grad()
        loss = model.cloze_loss({'asin': items}, labels, training=True, packed=False)
        loss.backward()
        if arena:
            ops.flush_pending_dw(opt.arena.ctx)
            ops.join_side_work(opt.arena.ctx)
        torch.cuda.synchronize()
        grads.append((loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}))
    assert torch.equal(grads[0][0], grads[1][0])
    for n in grads[0][1]:
        assert torch.equal(grads[0][1][n], grads[1][1][n]), n
    assert float(grads[0][1]['transformer.encoder.final_norm.gamma'].abs().max()) > 0


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_zeroed_sublayer_outputs_leave_the_final_norm_of_the_input(ops, dtype):
    """Wo, bo, W2, b2 = 0: every half adds an exact zero to the stream, so the encoder's output is layernorm_fwd(x_0; final_norm), bit
    for bit -- the stream is carried unrounded through the tails and the last tail is given the final norm's parameters"""
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    d, L, H, B, S = 64, 2, 2, 3, 10
    torch.manual_seed(0)
    enc = T.Encoder(L, d, H, 32, 0.0, norm='pre').cuda()
    with torch.no_grad():
        for layer in enc.enc_layers:
            for p in (layer.mha.dense.kernel, layer.mha.dense.bias, layer.ffn[1].kernel, layer.ffn[1].bias):
                p.zero_()
        enc.final_norm.gamma.add_(torch.randn(d, device='cuda') * 0.1)
        enc.final_norm.beta.add_(torch.randn(d, device='cuda') * 0.1)
    ops.bump_weights_epoch()
    x0 = torch.randn(B, S, d).to(dtype).cuda()
    mask = torch.zeros(B, S, dtype=torch.uint8, device='cuda')
    mask[1, 7:] = 1
    with torch.no_grad():
        out = enc(x0, training=False, mask=mask)
    want, _ = ops.layernorm_fwd(x0.reshape(B * S, d), enc.final_norm.gamma.detach(), enc.final_norm.beta.detach())
    assert out.shape == (B, S, d) and torch.equal(out.reshape(B * S, d), want)
    # a layer on its own returns the un-normalised stream: here the input itself
    with torch.no_grad():
        assert torch.equal(enc.enc_layers[0](x0, training=False, mask=mask), x0)


def test_predict_topk_of_a_causal_model_at_named_rows_ranks_the_gathered_full_layer_rows(ops):
    """the masked-query route is closed to a pre-LN encoder: predict_topk(flat_idx=, row_offsets=) runs the full last layer and ranks
    its gathered rows"""
    V, d, L, H, B, S, K = 40, 64, 2, 2, 6, 12, 5
    model = _build(V, d, L, H, [32], torch.float32, 9, attention='causal', norm='pre')
    with torch.no_grad():
        model.head.output_layer.kernel.mul_(4.0)
    b, ids, items, labels = _batch(B, S, V, 7)
    feats = {'asin': items}
    enc = model.transformer.encoder
    assert not enc.rows_supported(torch.float32) and not enc.rows_route(torch.float32, False)
    calls = []
    orig = ops.MQAttnBlockFn

    class Noting(orig):
        @staticmethod
        def apply(*a, **k):
            calls.append(1)
            return orig.apply(*a, **k)
    ops.MQAttnBlockFn = Noting
    try:
        real = (ids >= 10)
        last = torch.tensor([int(torch.nonzero(real[r])[-1]) for r in range(B)])           # the last item position of every sequence
        flat = (torch.arange(B) * S + last).to(torch.int32).cuda()
        off = torch.arange(B + 1, dtype=torch.int32).cuda()
        idx, _, _ = model.predict_topk(feats, K, flat_idx=flat, row_offsets=off)
        idx2, _, _ = model.predict_topk(feats, K, flat_idx=flat)
    finally:
        ops.MQAttnBlockFn = orig
    assert not calls
    with torch.no_grad():
        full = model.transformer({'items': ids.cuda()}, training=False)
        rows = full.reshape(B * S, d)[flat.long()]
        logits = model.head.logits(rows, out_fp32=True)[:, :V].float().cpu().numpy()
    order = np.argsort(-logits, axis=1, kind='stable')[:, :K + 1]
    top = np.take_along_axis(logits, order, 1)
    clear = (top[:, :-1] - top[:, 1:] > 1e-3).all(1)
    assert clear.mean() > 0.5
    assert np.array_equal(idx.cpu().numpy()[clear], order[:, :K][clear])
    assert torch.equal(idx, idx2)


def test_checkpoint_round_trip(ops, tmp_path):
    from bert4clickpath_amd import checkpoint, optim
    V, d, L, H, B, S = 60, 32, 2, 2, 4, 12
    model = _build(V, d, L, H, [16], torch.float32, 3, norm='pre')
    opt = optim.Adam(model.parameters())
    b, ids, items, labels = _batch(B, S, V, 3)
    opt.zero_grad()
    model.cloze_loss({'asin': items}, labels, training=True).backward()
    opt.step()
    torch.cuda.synchronize()
    want = float(model.cloze_loss({'asin': items}, labels, training=False))
    path = checkpoint.save_checkpoint(os.path.join(str(tmp_path), 'ckpt-pre-ln'), model, opt, epoch=1)
    other = _build(V, d, L, H, [16], torch.float32, 99, norm='pre')
    opt2 = optim.Adam(other.parameters())
    checkpoint.load_checkpoint(path, other, opt2)
    ops.bump_weights_epoch()
    for (n, p), (_, q) in zip(model.state_dict().items(), other.state_dict().items()):
        assert torch.equal(p, q), n
    assert 'transformer.encoder.final_norm.gamma' in other.state_dict()
    assert float(other.cloze_loss({'asin': items}, labels, training=False)) == want


def test_a_post_ln_model_launches_what_it_launched(ops, monkeypatch):
    """one training step of the default model: no pre-LN family in its launch log, and the log is the one the same model gives when
    the keyword is spelled out as 'post'; the pre-LN model of the same shape does list the new family"""
    from bert4clickpath_amd import optim
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    V, d, L, H, B, S = 300, 128, 2, 2, 24, 200
    b, ids, items, labels = _batch(B, S, V, 13, min_len=150)
    logs = {}
    for tag, kw in (('default', {}), ('post', {'norm': 'post'}), ('pre', {'norm': 'pre'})):
        model = _build(V, d, L, H, [64], torch.bfloat16, 11, dropout=0.1, **kw)
        opt = optim.Adam(model.parameters())
        opt.zero_grad()
        log = []
        monkeypatch.setattr(ops, 'family_log', log)
        T.set_dropout_seed(5)
        loss = model.cloze_loss({'asin': items}, labels, training=True, packed=False)
        loss.backward()
        ops.flush_pending_dw(opt.arena.ctx)
        ops.join_side_work(opt.arena.ctx)
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, 'family_log', None)
        logs[tag] = (log, T.dropout_seeds.counter, float(loss))
    pre_families = {'layernorm_bwd_add', 'gemm_nt_ln_bwd_add'}
    fam = lambda log: [f for f, _ in log]      # noqa: E731
    assert not pre_families & set(fam(logs['default'][0])) and len(logs['default'][0]) > 10
    assert logs['default'] == logs['post']                                   # launches, bytes, seeds drawn and the loss itself
    assert 'layernorm_bwd_add' in fam(logs['pre'][0]) and logs['pre'][1] == logs['default'][1]
    assert 'layernorm_fwd' not in fam(logs['default'][0]) and fam(logs['pre'][0]).count('layernorm_fwd') == 1
