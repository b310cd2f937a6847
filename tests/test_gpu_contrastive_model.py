"""model.contrastive_loss on the device (NO REFERENCE ORACLE: an extension; the float64 restatement is tests/nce_ref.py), at the smoke
model's size (V = 300, B = 6, S = 24, 2 layers), bidirectional and causal, fp32 and bf16: the loss is the restatement applied to the
rows _masked_rows returns; every encoder and embedding parameter's gradient is torch autograd's over the dense InfoNCE on the same
rows, through the same model; dropout views; same_target; one combined optimizer step.

Gates.  From the rows on: nce_ref.bounds times max(2, 2 x MEASURED_RATIO) (tests/test_gpu_nce.py).  Parameter gradients: the suite's own
model-level gates (tests/test_gpu_candidate_loss.py::test_softmax_over_every_item_equals_cloze_loss, tests/test_gpu_causal_model.py):
fp32 -- a gradient within 2e-4 of its largest entry (1e-5 absolute where it is identically zero); bf16 -- bf16_gates.BF16_GRAD_BOUND
in relative L2; both sides here share the encoder's kernels, so one gate, not the sum of two."""
import numpy as np
import pytest
import torch

import nce_ref as nr

pytestmark = pytest.mark.gpu

V, B, S = 300, 6, 24
GATE = nr.gate_factor()
FORMS = [pytest.param('bidirectional', torch.float32, id='bidirectional-fp32'), pytest.param('causal', torch.float32, id='causal-fp32'),
         pytest.param('bidirectional', torch.bfloat16, id='bidirectional-bf16'), pytest.param('causal', torch.bfloat16, id='causal-bf16')]


@pytest.fixture(scope='module')
def ops():
    from bert4clickpath_amd import ops as o
    return o


def _model(attention, dtype, dropout=0.0, seed=0):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    torch.manual_seed(seed)
    d = 32 if dtype == torch.float32 else 64
    head = SoftMaxHead([64, d], V)
    return ClickstreamTransformer({'items': ['asin']}, {'items': ['item%d' % i for i in range(V)]}, {'items': d}, head,
                                  value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, dropout_rate=dropout,
                                  compute_dtype=dtype, attention=attention).to('cuda')


def _items(seed):
    """(B, S - 3) unmasked item ids of a synthetic batch, right-padded, and their lengths"""
    from bert4clickpath_amd import input_pipeline
    b = input_pipeline.synthetic_cloze_batch(B, S, V, seed=seed, min_len=5)
    ids = b['ids'].copy()
    ids.reshape(-1)[b['flat_idx']] = b['labels'] + 10
    items = ids[:, 2:S - 1]
    return torch.from_numpy(np.ascontiguousarray(items)).cuda(), (items != 0).sum(1)


def _spy_rows(ops, monkeypatch, replace=None):
    """note the z the autograd block is called with (and, with `replace`, compute the loss by it instead)"""
    seen = {}
    orig = ops.InfoNCEFn.apply

    def apply(z, pos, group, temperature, similarity):
        seen.update(z=z, pos=pos, group=group, temperature=temperature, similarity=similarity)
        return orig(z, pos, group, temperature, similarity) if replace is None else replace(z, pos, group, temperature, similarity)
    monkeypatch.setattr(ops.InfoNCEFn, 'apply', staticmethod(apply))
    return seen


def _dense(z, pos, group, temperature, similarity):
    """torch autograd over the dense float64 evaluation of the definition, on the device, from the rows the model produced"""
    g = None if group is None else group.cpu().numpy()
    return nr.dense_loss(z.double(), pos.cpu().numpy(), g, nr.inv_temp(temperature), similarity == 'cos').to(torch.float32)


def _grads(model, loss):
    model.zero_grad(set_to_none=True)
    loss.backward()
    return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}


def _restated(seen, bf16):
    z = seen['z'].detach().float().cpu().numpy()
    g = None if seen['group'] is None else seen['group'].cpu().numpy()
    it, cos = nr.inv_temp(seen['temperature']), seen['similarity'] == 'cos'
    ref = nr.restate(z, seen['pos'].cpu().numpy(), g, it, cos)
    return ref, nr.bounds(z, ref, it, cos, bf16=bf16)


def _loss_gate(ref, bd):
    n = ref['item'].shape[0]
    nlive = max(int(ref['live'].sum()), 1)
    return GATE * ((bd['item'].sum() + nr.gamma(n + 2) * np.abs(ref['item']).sum()) / nlive + 4 * nr.U_F32 * abs(float(ref['loss'])))


@pytest.mark.parametrize('similarity,temperature', [('dot', 1.0), ('cos', 0.07)])
@pytest.mark.parametrize('attention,dtype', FORMS)
def test_two_views_against_the_restatement_and_torch_autograd(ops, monkeypatch, attention, dtype, similarity, temperature):
    bf16 = dtype == torch.bfloat16
    model = _model(attention, dtype)
    a, lens = _items(3)
    b, _ = _items(4)
    seen = _spy_rows(ops, monkeypatch)
    loss = model.contrastive_loss({'asin': a}, {'asin': b}, temperature=temperature, similarity=similarity)
    got = _grads(model, loss)
    # the rows: one per sequence and view, at the last item of each sequence (row b of the first view: position lens[b] + 1)
    z = seen['z']
    assert z.shape == (2 * B, model.transformer.d_model) and z.dtype == dtype
    assert seen['pos'].cpu().tolist() == list(range(B, 2 * B)) + list(range(B)) and seen['group'] is None
    flat = (torch.arange(B) * S + torch.from_numpy(lens) + 1).to(torch.int32).cuda()
    with torch.no_grad():
        rows, _ = model._masked_rows({'asin': a}, True, flat, row_offsets=torch.arange(B + 1, dtype=torch.int32, device='cuda'))
    assert torch.equal(rows, z[:B].detach())
    ref, bd = _restated(seen, bf16)
    print('loss %.6f, restated %.6f' % (float(loss.detach()), float(ref['loss'])))
    assert abs(float(loss.detach()) - float(ref['loss'])) <= _loss_gate(ref, bd)
    # the same rows through torch autograd, back-propagated through the same model
    monkeypatch.undo()
    _spy_rows(ops, monkeypatch, replace=_dense)
    want = _grads(model, model.contrastive_loss({'asin': a}, {'asin': b}, temperature=temperature, similarity=similarity))
    params = dict(model.named_parameters())
    body = [n for n in params if not n.startswith('head.')]
    assert body and set(body) <= set(got) and set(got) == set(want), sorted(set(body) - set(got))
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    if bf16:
        from bf16_gates import BF16_GRAD_BOUND, grad_errors
        for n, p in params.items():
            p.grad = None if n not in got else got[n].to(p.dtype).to(p.device)
        errs = grad_errors([(n, p) for n, p in params.items() if n in got], want)
        print(errs)
        assert len(errs) >= len(want) - 2 and max(errs.values()) <= BF16_GRAD_BOUND, errs
        return
    for n, gr in want.items():
        if n.endswith('mha.wk.bias') or float(gr.abs().max()) < 1e-9:      # (the key bias: identically zero, rounding noise on both sides)
            assert float(got[n].abs().max()) < 1e-5, n
        else:
            assert float((got[n] - gr).abs().max()) <= 2e-4 * float(gr.abs().max()), n


@pytest.mark.parametrize('attention,dtype', FORMS[1:3])
def test_flat_idx_names_the_rows(ops, monkeypatch, attention, dtype):
    """flat_idx: the representation is the row at the named position of both views"""
    model = _model(attention, dtype)
    a, lens = _items(3)
    b, _ = _items(4)
    flat = (torch.arange(B) * S + 2).to(torch.int32).cuda()          # the first item of every sequence
    seen = _spy_rows(ops, monkeypatch)
    loss = model.contrastive_loss({'asin': a}, {'asin': b}, flat_idx=flat)
    off = torch.arange(B + 1, dtype=torch.int32, device='cuda')
    with torch.no_grad():
        ra, _ = model._masked_rows({'asin': a}, True, flat, row_offsets=off)
        rb, _ = model._masked_rows({'asin': b}, True, flat, row_offsets=off)
    assert torch.equal(seen['z'].detach(), torch.cat([ra, rb]))
    ref, bd = _restated(seen, dtype == torch.bfloat16)
    assert abs(float(loss.detach()) - float(ref['loss'])) <= _loss_gate(ref, bd)
    with pytest.raises(ops.B4CError, match='one position per sequence'):
        model.contrastive_loss({'asin': a}, {'asin': b}, flat_idx=flat[:3])


@pytest.mark.parametrize('attention,dtype', FORMS[:2] + FORMS[3:])
def test_dropout_views(ops, attention, dtype):
    """inputs_b=None: two dropout realisations of one batch -- the loss differs between two seeds and is reproducible for one;
    without dropout (rate 0, or training=False) there are no two views: B4CError"""
    from bert4clickpath_amd.clickstream_transformer import transformer as tr
    model = _model(attention, dtype, dropout=0.2)
    a, _ = _items(3)

    def run(seed):
        tr.set_dropout_seed(seed)
        return float(model.contrastive_loss({'asin': a}, temperature=0.5).detach())
    one, two, again = run(11), run(12), run(11)
    assert np.isfinite([one, two]).all() and one == again and one != two and one > 0
    with pytest.raises(ops.B4CError, match='dropout'):
        model.contrastive_loss({'asin': a}, training=False)
    with pytest.raises(ops.B4CError, match='dropout'):
        _model(attention, dtype, dropout=0.0).contrastive_loss({'asin': a})
    with pytest.raises(ops.B4CError, match='similarity'):
        model.contrastive_loss({'asin': a}, similarity='l2')


@pytest.mark.parametrize('attention,dtype', FORMS[:1] + FORMS[3:])
def test_same_target_changes_the_loss_as_the_restatement_says(ops, monkeypatch, attention, dtype):
    bf16 = dtype == torch.bfloat16
    model = _model(attention, dtype)
    a, _ = _items(3)
    b, _ = _items(4)
    seen = _spy_rows(ops, monkeypatch)
    plain = float(model.contrastive_loss({'asin': a}, {'asin': b}, similarity='cos', temperature=0.2).detach())
    target = torch.tensor([7, 3, 7, -1, 9, -1], device='cuda')          # sequences 0 and 2 share their target; -1: none
    grouped = float(model.contrastive_loss({'asin': a}, {'asin': b}, similarity='cos', temperature=0.2, same_target=target).detach())
    assert seen['group'].dtype == torch.int32 and seen['group'].cpu().tolist() == [7, 3, 7, -1, 9, -1] * 2
    ref, bd = _restated(seen, bf16)
    key = ref['key']
    assert not key[0, 2] and not key[0, 2 + B] and not key[2 + B, 0] and key[0, B] and key[3, 5] and key[0, 1]
    assert abs(grouped - float(ref['loss'])) <= _loss_gate(ref, bd)
    seen['group'] = None
    ref0, bd0 = _restated(seen, bf16)
    assert abs(plain - float(ref0['loss'])) <= _loss_gate(ref0, bd0)
    assert float(ref0['loss']) > float(ref['loss']) and plain > grouped          # fewer keys: a smaller log-sum-exp
    with pytest.raises(ops.B4CError, match='same_target'):
        model.contrastive_loss({'asin': a}, {'asin': b}, same_target=target[:4])


def test_a_combined_step_under_adam(ops):
    """loss = next_item_loss + 0.1 * contrastive_loss on a device-built next-item batch, one Adam step: it runs and the weights move"""
    from bert4clickpath_amd import optim
    from bert4clickpath_amd.cloze_batches import DeviceCloze
    rng = np.random.default_rng(2)
    lengths = rng.integers(6, 30, size=40)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    items = rng.integers(0, V, size=int(offsets[-1])).astype(np.int32)
    dc = DeviceCloze(items, offsets, V=V, max_len=S - 3, holdout=2)
    batch = next(iter(dc.next_item_batches(B, 21, 1)))
    model = _model('causal', torch.float32, dropout=0.1)
    opt = optim.Adam(model.parameters())
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    main = model.next_item_loss(batch)
    aux = model.contrastive_loss(model._next_item_inputs(batch), temperature=0.5, similarity='cos', same_target=batch['items'][:, 0] - 10)
    loss = main + 0.1 * aux
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.detach())) and float(aux.detach()) > 0
    moved = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert any(n.startswith('transformer.') for n in moved) and len(moved) >= len(before) - 2, sorted(set(before) - set(moved))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
