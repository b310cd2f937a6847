"""Models at an encoder length of 600 on the streamed attention kernels (ops.long_attn, B4C_ATTN_LONG=1): two-layer bf16 models with
two heads at d_model 64 and 128 (head depth 32 and 64), B = 3, dropout 0, cloze_loss forward + backward, packed and dense.

With the switch on, the loss and every parameter gradient are held to the float64 oracle (oracle/torch_ref.py) evaluated with the
device pass's own ReLU patterns, at the bars every bf16 model test of this family uses (tests/bf16_gates.py, as
tests/test_gpu_dff.py::test_ff_dim_bf16_under_the_gate_bound holds the padded and the packed layout at S <= 512): loss 2e-3 relative,
every gradient tensor BF16_GRAD_BOUND = 0.03 relative L2, check_flips().  Sharing the patterns matters at this batch: 3 x 10 [MASK]
rows reach the loss, and one ReLU gate that falls on the other side of zero moves every gradient behind it -- without the shared
patterns two bf16 routes of this model (these kernels and the fp32-math row kernels) differ by 5 - 12 % in every tensor, and either
differs from plain float64 by up to 21 % (measured on the MI355X; tests/bf16_gates.py describes the effect).  The same check on the
parent's route for this length -- dense, switch off: the row kernels -- is printed beside them as the control.
With the switch off the packed call raises the B4CError it raised, and a fresh process still prints the row-kernel notice on a
dense launch.  A causal norm='pre' model through next_item_loss on a device-built batch of the same length (1,700 target rows): the
streamed packed route against the dense row-kernel route, the two-evaluations bars of
tests/test_gpu_causal_model.py::test_packed_equals_dense (loss 2e-3 relative, gradients 0.06 relative L2).

Measured on the MI355X (loss error against float64; worst gradient tensor):
  d_model  64, packed and dense (the same bits)   9.4e-5   0.91 % (enc_layers.1.mha.wq.kernel)    control, row kernels: 6.2e-5, 1.00 %
  d_model 128, packed and dense (the same bits)   2.5e-5   1.27 % (enc_layers.1.mha.wq.kernel)    control, row kernels: 5.4e-5, 1.33 %
  gates that differ from the oracle's own: 0.2 % / 0.4 % of a layer's units, the farthest at 0.02 rms
  causal pre-LN, next_item_loss: loss 5.381222 against 5.381191 on the row kernels, worst gradient tensor 4.1 % (the item table)
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu

S_ENC, B = 600, 3
OLD_PACKED_ERROR = r'^packed=True needs bf16 compute, head depth 32 / 64 and an encoder length <= 512$'


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops as o
    return o


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _model(V, d, head_dims, seed=3, **kw):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(seed)
    m = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': d}, SoftMaxHead(list(head_dims), V),
                               value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, dropout_rate=0.0,
                               compute_dtype=torch.bfloat16, **kw)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias') or n.endswith('beta'):
                p.normal_(0, 0.05)
    return m.cuda()


def _grads(model, loss):
    model.zero_grad(set_to_none=True)
    loss.backward()
    return float(loss.detach()), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _two_evaluations(tag, l_a, g_a, l_b, g_b, loss_bar=2e-3, grad_bar=0.06):
    """every figure is printed before the first assertion"""
    errs = {n: rel_err(g_a[n], g_b[n]) for n in g_b if float(g_b[n].float().norm()) >= 1e-9 and not n.endswith('mha.wk.bias')}
    print('%s: loss %.6f / %.6f; gradient tensors %s' % (tag, l_a, l_b, ' '.join('%s=%.3f' % kv for kv in sorted(errs.items()))))
    assert abs(l_a - l_b) < loss_bar * abs(l_b), (tag, l_a, l_b)
    for n, e in errs.items():
        assert e < grad_bar, (tag, n, e)
    return max(errs.values())


@pytest.mark.parametrize('d', [64, 128])
def test_cloze_model_at_length_600(ops, d, monkeypatch):
    from bert4clickpath_amd import input_pipeline
    from bert4clickpath_amd._lib import B4CError
    from bf16_gates import BF16_GRAD_BOUND, GateRecorder, grad_errors
    V = 300
    model = _model(V, d, (32, 64))
    b = input_pipeline.synthetic_cloze_batch(B, S_ENC, V, seed=21, min_len=530)
    ids = torch.from_numpy(b['ids'])
    feats = {'asin': ids[:, 2:S_ENC - 1].contiguous().cuda()}
    labels = torch.from_numpy(b['labels_padded']).cuda()
    n_real = int((b['ids'] != 0).sum())
    assert 512 * B < n_real < B * S_ENC and len(set(b['lens'].tolist())) > 1                 # ragged, every sequence past 512

    def run(**kw):
        model.zero_grad(set_to_none=True)
        with GateRecorder(ops) as rec:
            loss = model.cloze_loss(feats, labels, training=True, max_masked_per_row=10, **kw)
        loss.backward()
        return float(loss.detach()), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, rec

    # the switch off: what the parent did
    monkeypatch.setattr(ops, 'long_attn', False)
    assert not model.transformer.packed_supported(S_ENC)
    with pytest.raises(B4CError, match=OLD_PACKED_ERROR):
        model.cloze_loss(feats, labels, training=True, max_masked_per_row=10, packed=True)
    calls = []
    for name in ('attn_long_fwd', 'attn_long_bwd'):
        monkeypatch.setattr(ops, name, lambda *a, _f=getattr(ops, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    rows_route = run(n_real_tokens=n_real)                                                  # auto: falls back to dense, the row kernels
    assert model._packed is None and not calls
    # the switch on
    monkeypatch.setattr(ops, 'long_attn', True)
    assert model.transformer.packed_supported(S_ENC)
    packed = run(n_real_tokens=n_real)
    assert model._packed is not None and model._packed.T == n_real
    assert calls.count('attn_long_fwd') >= 1 and calls.count('attn_long_bwd') == calls.count('attn_long_fwd')
    del calls[:]
    dense = run(packed=False)
    assert model._packed is None and calls.count('attn_long_fwd') >= 1
    # float64 with each pass's own ReLU patterns; every figure is printed before the first assertion
    token_rows = torch.from_numpy(np.flatnonzero(b['ids'].reshape(-1) != 0)).long()
    figures = {}
    for tag, (l, g, rec) in (('row kernels (control)', rows_route), ('packed', packed), ('dense', dense)):
        relu = rec.relu_for(2, 2, torch.from_numpy(b['flat_idx']).long(), B, S_ENC, token_rows=token_rows)
        Pt = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
        ref, _ = tr.model_loss(ids, torch.from_numpy(b['labels']).long(), Pt, 2, 2, 2, relu=relu)
        ref.backward()
        for n, p in model.named_parameters():
            p.grad = g[n]
        errs = grad_errors(model.named_parameters(), {n: Pt[n].grad for n, _ in model.named_parameters()})
        worst = max(errs, key=errs.get)
        flips = max(f for f, _ in rec.flips.values()), max(far for _, far in rec.flips.values())
        print('attn long model d=%d %s: loss %.6f float64 %.6f (%.2e relative), worst gradient tensor %s %.4f; gates that differ %.4f, '
              'farthest %.3f rms' % (d, tag, l, float(ref), abs(l - float(ref)) / float(ref), worst, errs[worst], flips[0], flips[1]))
        figures[tag] = (l, float(ref), worst, errs[worst], rec)
    for tag in ('packed', 'dense'):
        l, r, worst, e, rec = figures[tag]
        assert abs(l - r) < 2e-3 * r, (tag, l, r)
        assert e < BF16_GRAD_BOUND, (tag, worst, e)
        rec.check_flips()


def test_a_dense_launch_with_the_switch_off_still_prints_the_notice():
    """the notice is printed once per process: a fresh one, B4C_ATTN_LONG unset, one dense bf16 forward at S = 600"""
    code = ('import torch\n'
            'from bert4clickpath_amd import ops\n'
            'assert not ops.long_attn\n'
            'q = torch.zeros(600, 3 * 64, dtype=torch.bfloat16, device="cuda")\n'
            'o, lse = ops.attn_fwd(q, torch.zeros(1, 600, dtype=torch.uint8, device="cuda"), 1, 600, 1, 64)\n'
            'torch.cuda.synchronize()\n'
            'print("lse", float(lse[0, 0, 0]))\n')
    env = {k: v for k, v in os.environ.items() if k != 'B4C_ATTN_LONG'}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env['PYTHONPATH'] = root + os.pathsep + env.get('PYTHONPATH', '')
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=120, cwd=root)
    assert out.returncode == 0, out.stderr
    assert 'using the fp32-math row kernels (exact, several times slower)' in out.stderr and 'S=600' in out.stderr
    assert abs(float(out.stdout.split()[-1]) - float(np.log(600.0))) < 1e-4


def test_causal_pre_ln_model_through_next_item_loss(ops, monkeypatch):
    """A causal norm='pre' model (every layer the full layer), a device-built next-item batch of width 597: encoder length 600.
    Streamed kernels on the packed layout against the same model on the dense layout with the switch off (the row kernels)."""
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    V, W = 200, S_ENC - 3
    rng = np.random.default_rng(5)
    lens = np.array([W + 1, 560, 640])                              # holdout 1: training views of 597, 559 and 597 + 42 items
    items = rng.integers(0, V, int(lens.sum())).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dc = DeviceCloze(items, offsets, V=V, max_len=W)
    win = np.argsort(-dc.next_item_counts(np.arange(dc.n_windows)))[:B]
    batch = dc.next_item_window_batch(win, seed=13, width=W)
    assert tuple(batch['items'].shape) == (B, W) and batch['n_real_tokens'] > 512 * B and batch['n_targets'] > 512 * B
    model = _model(V, 64, (32, 64), seed=9, attention='causal', norm='pre', ffn_activation='gelu')
    monkeypatch.setattr(ops, 'long_attn', True)
    calls = []
    monkeypatch.setattr(ops, 'attn_long_bwd', lambda *a, _f=ops.attn_long_bwd, **k: (calls.append(k.get('causal')), _f(*a, **k))[1])
    l_long, g_long = _grads(model, model.next_item_loss(batch))
    assert model._packed is not None and calls == [True, True]      # both layers, causal, on the packed layout
    monkeypatch.setattr(ops, 'long_attn', False)
    feats = {'asin': batch['items']}
    l_rows, g_rows = _grads(model, model.cloze_loss(feats, batch['labels'], training=True, flat_idx=batch['flat_idx'], packed=False))
    assert model._packed is None and calls == [True, True] and np.isfinite(l_long)
    worst = _two_evaluations('attn long causal pre-LN model against the row kernels', l_long, g_long, l_rows, g_rows)
    print('attn long causal pre-LN model: loss %.6f, row kernels %.6f, worst gradient tensor %.3f' % (l_long, l_rows, worst))
