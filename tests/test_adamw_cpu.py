"""Decoupled weight decay (optim.Adam(weight_decay=..., exclude_from_weight_decay=...), Keras AdamW): the host side, without a
GPU -- argument handling, optim.no_decay_params, the per-block decay flags against the arena's layout, the history of decay
factors the row-lazy kernel replays from, and the new entry points' argument checks."""
import math
import struct

import numpy as np
import pytest
import torch

import abi_pin


def _param(*shape):
    return torch.nn.Parameter(torch.randn(*shape) if shape else torch.randn(10, 8))


def _f32(x):
    return struct.unpack('f', struct.pack('f', x))[0]


def test_weight_decay_argument():
    from bert4clickpath_amd import optim
    o = optim.Adam([_param()])
    assert o.weight_decay is None
    for bad in (-1e-9, -1.0, float('nan'), float('inf'), float('-inf')):
        with pytest.raises(ValueError):
            optim.Adam([_param()], weight_decay=bad)
        with pytest.raises(ValueError):
            o.weight_decay = bad
    assert o.weight_decay is None
    o = optim.Adam([_param()], weight_decay=0)
    assert o.weight_decay == 0.0 and isinstance(o.weight_decay, float)
    o.weight_decay = 0.01                     # a plain attribute, like global_clipnorm
    assert o.weight_decay == 0.01
    o.weight_decay = None
    assert o.weight_decay is None
    # the exclusion list: parameters of this optimizer only
    a, b, stranger = _param(), _param(7), _param(7)
    optim.Adam([a, b], weight_decay=0.01, exclude_from_weight_decay=[b])
    optim.Adam([a, b], weight_decay=0.01, exclude_from_weight_decay=iter([b]))      # any iterable
    with pytest.raises(ValueError):
        optim.Adam([a, b], weight_decay=0.01, exclude_from_weight_decay=[stranger])
    frozen = _param(7)
    frozen.requires_grad_(False)              # not in the arena either
    with pytest.raises(ValueError):
        optim.Adam([a, b, frozen], weight_decay=0.01, exclude_from_weight_decay=[frozen])


def test_state_dict_stores_weight_decay_for_the_record_only(tmp_path):
    from bert4clickpath_amd import optim
    o = optim.Adam([_param()], weight_decay=0.02)
    sd = o.state_dict()
    assert sd['weight_decay'] == 0.02
    assert optim.Adam([_param()]).state_dict()['weight_decay'] is None
    fresh = optim.Adam([_param()], weight_decay=0.5)
    fresh.load_state_dict(sd)
    assert fresh.weight_decay == 0.5          # the constructor's argument governs
    off = optim.Adam([_param()])
    off.load_state_dict(sd)
    assert off.weight_decay is None
    # a state without the key (written before the feature) still loads
    off.load_state_dict({'iterations': 3, 'lr': 7e-4, 'm': off.m, 'v': off.v})
    assert off.iterations == 3 and off.weight_decay is None


def test_checkpoint_stores_weight_decay_for_the_record_only(tmp_path):
    from bert4clickpath_amd import checkpoint, optim
    model = torch.nn.Linear(8, 4)
    o = optim.Adam(model.parameters(), weight_decay=0.03, exclude_from_weight_decay=optim.no_decay_params(model))
    path = checkpoint.save_checkpoint(str(tmp_path / 'ckpt-a'), model, o)
    blob = torch.load(path, map_location='cpu', weights_only=True)
    assert blob['optimizer']['weight_decay'] == 0.03
    other = torch.nn.Linear(8, 4)
    o2 = optim.Adam(other.parameters(), weight_decay=0.5)
    checkpoint.load_checkpoint(path, other, o2)
    assert o2.weight_decay == 0.5
    # a checkpoint written before the feature (no such key) still loads
    del blob['optimizer']['weight_decay']
    torch.save(blob, str(tmp_path / 'ckpt-old.pt'))
    checkpoint.load_checkpoint(str(tmp_path / 'ckpt-old.pt'), other, o2)
    assert o2.weight_decay == 0.5
    plain = optim.Adam(torch.nn.Linear(8, 4).parameters())
    assert torch.load(checkpoint.save_checkpoint(str(tmp_path / 'ckpt-b'), torch.nn.Linear(8, 4), None),
                      weights_only=True).get('optimizer') is None
    assert plain.state_dict()['weight_decay'] is None


def test_no_decay_params_on_a_small_model():
    from bert4clickpath_amd import optim
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    V = 50
    model = ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(V)]}, {'items': 32}, SoftMaxHead([16, 32], V),
                                   value_to_head='[MASK]', num_encoder_layers=2, num_attention_heads=2, dropout_rate=0.1)
    got = optim.no_decay_params(model)
    want = [p for p in model.parameters() if p.dim() < 2]
    assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    names = {id(p): n for n, p in model.named_parameters()}
    assert got and len(got) < len(list(model.parameters()))
    assert all(p.dim() >= 2 for p in model.parameters() if id(p) not in {id(q) for q in got})
    # the embedding table decays; some bias (the vocabulary head's among them) and the LayerNorm vectors do not
    table = model.transformer.embedding_layers['items'].weight
    assert not any(q is table for q in got)
    assert any(n.startswith('head.') for n in (names[id(q)] for q in got))
    optim.Adam(model.parameters(), weight_decay=0.01, exclude_from_weight_decay=got)


def test_block_flags_follow_the_arena_layout():
    """interleaved decayed / excluded parameters of ragged sizes, in a shuffled arena order: every 64-element block of an
    excluded parameter is 0, every block of a decayed one is 1, no block belongs to two parameters and every block to one"""
    from bert4clickpath_amd import optim
    shapes = [(10, 8), (5,), (70,), (3, 64), (1,), (64,), (65,), (129, 3), (63,), (2, 2)]
    params = [_param(*s) for s in shapes]
    excluded = [params[i] for i in (1, 2, 5, 8)]
    order = {id(p): k for k, p in zip([3, 0, 7, 1, 9, 2, 8, 5, 4, 6], params)}
    o = optim.Adam(params, weight_decay=0.01, exclude_from_weight_decay=excluded, order=lambda p: order[id(p)])
    a = o.arena
    assert [order[id(p)] for p in a.params] == sorted(order.values())
    blocks = o.decay_blocks_host()
    assert blocks.dtype == torch.uint8 and blocks.numel() == a.numel // 64 and a.numel % 64 == 0
    owner = np.full(a.numel // 64, -1)
    for k, (p, off) in enumerate(zip(a.params, a.offsets)):
        assert off % 64 == 0
        lo, hi = off // 64, (off + p.numel() + 63) // 64
        assert (owner[lo:hi] == -1).all(), 'a block belongs to two parameters'
        owner[lo:hi] = k
        want = 0 if any(p is q for q in excluded) else 1
        assert (blocks[lo:hi] == want).all(), (k, tuple(p.shape))
    assert (owner >= 0).all()
    assert 0 < int(blocks.sum()) < blocks.numel()
    # without an exclusion list everything decays
    assert bool(optim.Adam([_param(), _param(5)], weight_decay=0.01).decay_blocks_host().all())
    # a row-lazy table decays, or not, as a whole
    t1, t2, b = _param(20, 8), _param(20, 8), _param(8)
    o = optim.Adam([t1, t2, b], lazy_rows=[t1, t2], weight_decay=0.01, exclude_from_weight_decay=[t2, b])
    assert t1._b4c_lazy.decay is True and t2._b4c_lazy.decay is False


def _host_steps(opt, n):
    """the host side of n steps (optim.Adam._begin_step: what step() does before it launches), on a CPU optimizer"""
    out = []
    for _ in range(n):
        t, lr_t, d = opt._begin_step()
        out.append(d)
    return out


def test_decay_history_holds_each_steps_own_factor():
    """d_s = fp32(lr(s - 1) * weight_decay): the scalar the dense kernel is handed at step s and entry s of the table the row
    kernel reads are the same fp32 value -- under a float lr, an lr and a weight_decay changed in mid-run, and a schedule"""
    from bert4clickpath_amd import optim
    from clickstream_transformer.training_utils import WarmupLinearDecay
    wd = 0.01
    # float lr, changed before step 6; weight_decay changed before step 9, switched off before step 12
    table = _param(16, 8)
    o = optim.Adam([table], learning_rate=1e-3, lazy_rows=[table], weight_decay=wd)
    want, got = [0.0], [None]
    lr, w = 1e-3, wd
    for t in range(1, 15):
        if t == 6:
            o.lr = lr = 3.17e-4
        if t == 9:
            o.weight_decay = w = 0.05
        if t == 12:
            o.weight_decay = w = None
        if t == 4:
            o.decay_hist(8)                    # somebody looked ahead: later changes must still show from their first step
        got += _host_steps(o, 1)
        want.append(np.float32(np.float64(lr) * np.float64(w)) if w is not None else None)
    for t in range(1, 15):
        assert (got[t] is None) == (want[t] is None)
        assert got[t] is None or np.float32(got[t]) == want[t] and got[t] == float(want[t]), t
    hist = o.decay_hist(14)
    assert hist.dtype == torch.float32 and hist.numel() == o.lr_hist(14).numel() >= 15       # the same capacity
    table_want = np.array([0.0 if w is None else w for w in want], dtype=np.float32)
    assert np.array_equal(hist[:15].numpy(), table_want), (hist[:15], table_want)
    assert len({float(x) for x in table_want}) == 4                                           # 0 (and off again), three factors
    # one entry per step: the table object stays, the entries of past steps never change
    again = o.decay_hist(14)
    assert again is hist
    _host_steps(o, 1)
    assert o.decay_hist(15) is hist and np.array_equal(hist[:15].numpy(), table_want)
    # reset_rows() rebuilds the history from the present settings
    o.weight_decay = 0.02
    o.reset_rows()
    assert np.array_equal(o.decay_hist(15)[:16].numpy(),
                          np.array([0.0] + [np.float32(np.float64(3.17e-4) * 0.02)] * 15, dtype=np.float32))
    # a schedule: step s decays with schedule(s - 1), the plain learning rate, not the bias-corrected lr_t
    sched = WarmupLinearDecay(2e-3, 3, 40)
    table = _param(16, 8)
    s = optim.Adam([table], learning_rate=sched, lazy_rows=[table], weight_decay=wd)
    got = [0.0] + _host_steps(s, 45)
    want = np.array([0.0] + [np.float64(sched(t - 1)) * wd for t in range(1, 46)]).astype(np.float32)
    assert np.array_equal(np.array(got, dtype=np.float32), want) and all(g == _f32(g) for g in got)
    assert np.array_equal(s.decay_hist(45)[:46].numpy(), want)
    assert want[1] == 0.0 and want[4] == np.float32(2e-3 * wd) and len(set(want.tolist())) > 30
    assert s._lr_host[4] == sched(3) * math.sqrt(1 - 0.999 ** 4) / (1 - 0.9 ** 4)            # lr_t is another number
    # with weight_decay None no decay table is ever made
    table = _param(16, 8)
    n = optim.Adam([table], lazy_rows=[table])
    assert _host_steps(n, 3) == [None] * 3 and n._wd_dev is None and n._decay_blocks_dev is None


def test_adamw_entry_points_are_exported_and_check_their_arguments():
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    E = _lib.declared_symbols()
    for name in ('b4c_adamw_step', 'b4c_adamw_rows'):
        assert name in E and hasattr(L, name)
    assert [s for s in E if not hasattr(L, s)] == []
    assert L.b4c_abi_version() == abi_pin.ABI_VERSION == _lib.ABI_VERSION          # additive: no existing signature changed
    A = 1 << 20                                                   # a well-aligned, never dereferenced "pointer"
    # dense form: (p, g, m, v, n, lr_t, b1, b2, eps, grad_mul, coef | NULL, decay, blocks, stream)
    assert L.b4c_adamw_step(None, A, A, A, 64, 1e-3, 0.9, 0.999, 1e-9, 1.0, None, 1e-5, A, None) == -1
    assert b'adamw_step' in L.b4c_last_error()
    assert L.b4c_adamw_step(A, A + 4, A, A, 64, 1e-3, 0.9, 0.999, 1e-9, 1.0, None, 1e-5, A, None) == -1
    assert b'16-byte aligned' in L.b4c_last_error()
    assert L.b4c_adamw_step(A, A, A, A, 64, 1e-3, 0.9, 0.999, 1e-9, 1.0, None, 1e-5, None, None) == -1
    assert b'block table' in L.b4c_last_error()
    assert L.b4c_adamw_step(A, A, A, A, 64, 1e-3, 0.9, 0.999, 1e-9, 1.0, A + 2, 1e-5, A, None) == -1
    assert b'misaligned coefficient' in L.b4c_last_error()
    for bad in (-1e-5, float('nan'), float('inf')):
        assert L.b4c_adamw_step(A, A, A, A, 64, 1e-3, 0.9, 0.999, 1e-9, 1.0, None, bad, A, None) == -1
        assert b'decay factor' in L.b4c_last_error()
    # row form: (p, g, m, v, stamp, ids, n, row_lo, rows, width, lr_hist, decay_hist, t, b1, b2, eps, grad_mul, coef | NULL, mode, stream)
    assert L.b4c_adamw_rows(A, A, A, A, A, None, 4, 0, 16, 8, A, None, 1, 0.9, 0.999, 1e-9, 1.0, None, 1, None) == -1
    assert b'adamw_rows' in L.b4c_last_error() and b'decay history' in L.b4c_last_error()
    assert L.b4c_adamw_rows(A, A, A, A, A, None, 4, 0, 16, 6, A, A, 1, 0.9, 0.999, 1e-9, 1.0, None, 1, None) == -1
    assert b'multiple of 4' in L.b4c_last_error()
    assert L.b4c_adamw_rows(A, A, A, A, A, None, 4, 14, 16, 8, A, A, 1, 0.9, 0.999, 1e-9, 1.0, None, 0, None) == -1
    assert b'outside the table' in L.b4c_last_error()
    assert L.b4c_adamw_rows(A, A, A, A, A, None, 4, 0, 16, 8, A, A, 1, 0.9, 0.999, 1e-9, 1.0, None, 2, None) == -1
    assert L.b4c_adamw_rows(A, A, A, A, A, A, 0, 0, 16, 8, A, A, 1, 0.9, 0.999, 1e-9, 1.0, None, 1, None) == 0     # empty: no launch
