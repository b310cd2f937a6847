"""Learning-rate schedules (clickstream_transformer/training_utils.py of the reference, :15-59) and the host side of
optim.Adam(learning_rate=<schedule>, global_clipnorm=...): argument handling and the new entry points' argument checks, all
without a GPU."""
import math

import pytest
import torch

import abi_pin

REL = 1e-12          # float64 host arithmetic against hand-computed float64 values


def _close(got, want):
    return abs(got - want) <= REL * abs(want)


def test_custom_lr_schedule_values_and_quirks():
    from clickstream_transformer.training_utils import CustomLRSchedule
    s = CustomLRSchedule(128, 4000)
    assert _close(s(4000), 128 ** -0.5 * 4000 ** -0.5) and abs(s(4000) - 1.397542e-3) < 1e-9
    assert _close(s(1000), 128 ** -0.5 * 1000 * 4000 ** -1.5) and abs(s(1000) - 3.493856e-4) < 1e-10
    assert _close(s(16000), 128 ** -0.5 * 16000 ** -0.5)           # past the warm-up: the rsqrt branch
    assert s(0) == 0.0                                              # min(inf, 0)
    assert isinstance(s(7), float)
    # `scale` is applied twice, as the reference applies it
    for step in (1, 1000, 4000, 9000):
        assert _close(CustomLRSchedule(128, 4000, scale=2)(step), 4.0 * s(step))
    assert CustomLRSchedule(64).warmup_steps == 4000 and CustomLRSchedule(64).scale == 1
    assert s.get_config() == {'d_model': 128.0, 'warmup_steps': 4000, 'scale': 1}
    assert list(s.get_config()) == ['d_model', 'warmup_steps', 'scale']


def test_exponential_decay_values_and_config_keys():
    from clickstream_transformer.training_utils import CustomExponentialDecayLR
    init, limit, steps, rate = 1e-3, 1e-5, 250, 0.5
    s = CustomExponentialDecayLR(init, limit, steps, rate)
    assert _close(s(steps), (init - limit) * rate + limit)
    assert _close(s(0), init)
    assert _close(s(2 * steps), (init - limit) * rate ** 2 + limit)
    assert _close(s(125), (init - limit) * math.sqrt(rate) + limit)
    assert s(10 ** 9) == limit
    assert s.get_config() == {'init_lr': init, 'limit_lr': limit, 'decay_steps': steps, 'decay_rate': rate}


def test_warmup_linear_decay_shape():
    from clickstream_transformer.training_utils import WarmupLinearDecay
    s = WarmupLinearDecay(1e-3, 10, 110, end_lr=1e-5)
    assert s(0) == 0.0 and _close(s(5), 5e-4) and _close(s(10), 1e-3)
    assert _close(s(60), 1e-5 + (1e-3 - 1e-5) * 0.5)
    assert s(110) == 1e-5 and s(10 ** 6) == 1e-5
    assert WarmupLinearDecay(2e-3, 0, 100)(0) == 2e-3 and WarmupLinearDecay(2e-3, 0, 100)(100) == 0.0
    with pytest.raises(ValueError):
        WarmupLinearDecay(1e-3, 100, 100)
    assert set(s.get_config()) == {'peak_lr', 'warmup_steps', 'total_steps', 'end_lr'}


def test_both_import_paths_give_the_same_classes():
    import bert4clickpath_amd.clickstream_transformer.training_utils as impl
    import clickstream_transformer.training_utils as alias
    for name in ('CustomLRSchedule', 'CustomExponentialDecayLR', 'WarmupLinearDecay', 'load_vocabulary'):
        assert getattr(alias, name) is getattr(impl, name)


def _param():
    return torch.nn.Parameter(torch.zeros(10, 8))


def test_adam_takes_a_float_or_a_schedule():
    from bert4clickpath_amd import checkpoint, optim
    from clickstream_transformer.training_utils import CustomLRSchedule
    B1, B2 = 0.9, 0.999
    o = optim.Adam([_param()], learning_rate=2e-3)
    assert o.lr == 2e-3 and not o.scheduled and o.global_clipnorm is None and o.last_grad_norm is None
    o.lr = 5e-4
    assert o.lr == 5e-4 and o._lr_t(3) == 5e-4 * math.sqrt(1 - B2 ** 3) / (1 - B1 ** 3)
    checkpoint.ReduceLROnPlateau(o, patience=1)

    sched = CustomLRSchedule(64, warmup_steps=10)
    s = optim.Adam([_param()], learning_rate=sched)
    assert s.scheduled and s.lr == sched(0) == 0.0
    # step t (1-based) is taken with schedule(t - 1): the number of steps already taken
    for t in (1, 2, 11, 40):
        assert s._lr_t(t) == sched(t - 1) * math.sqrt(1 - B2 ** t) / (1 - B1 ** t)
    s.iterations = 7
    assert s.lr == sched(7)
    with pytest.raises(TypeError):
        s.lr = 1e-3
    with pytest.raises(TypeError):
        checkpoint.ReduceLROnPlateau(s)
    # a plain function is a schedule too
    f = optim.Adam([_param()], learning_rate=lambda step: 1e-3 / (1 + step))
    assert f.lr == 1e-3 and f._lr_t(2) == 5e-4 * math.sqrt(1 - B2 ** 2) / (1 - B1 ** 2)
    # the state keeps the float and the step count; loading into a scheduled optimizer keeps the schedule
    s.load_state_dict({'iterations': 12, 'lr': 123.0, 'm': s.m, 'v': s.v})
    assert s.iterations == 12 and s.lr == sched(12)
    assert s._lr_host == [0.0] + [s._lr_t(t) for t in range(1, 13)]
    o.load_state_dict({'iterations': 3, 'lr': 7e-4, 'm': o.m, 'v': o.v})
    assert o.lr == 7e-4


def test_global_clipnorm_argument():
    from bert4clickpath_amd import optim
    for bad in (0, 0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            optim.Adam([_param()], global_clipnorm=bad)
    o = optim.Adam([_param()], global_clipnorm=5)
    assert o.global_clipnorm == 5.0
    o.global_clipnorm = None
    assert o.global_clipnorm is None
    o.global_clipnorm = 0.25
    with pytest.raises(ValueError):
        o.global_clipnorm = -3
    assert o.global_clipnorm == 0.25


def test_new_entry_points_check_their_arguments_without_a_gpu():
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    E = _lib.declared_symbols()
    for name in ('b4c_grad_sumsq', 'b4c_grad_sumsq_rows', 'b4c_grad_clip_coef', 'b4c_adam_step_clipped', 'b4c_adam_rows_clipped'):
        assert name in E
    assert L.b4c_abi_version() == abi_pin.ABI_VERSION                      # additive: no existing signature changed
    A = 1 << 20                                           # a well-aligned, never dereferenced "pointer"
    # null pointers
    assert L.b4c_grad_sumsq(None, 4096, 0, 4096, A, None) == -1 and b'grad_sumsq' in L.b4c_last_error()
    assert L.b4c_grad_sumsq(A, 4096, 0, 4096, None, None) == -1
    assert L.b4c_grad_sumsq_rows(A, 4096, 0, 16, 8, None, 4, A, None) == -1 and b'grad_sumsq_rows' in L.b4c_last_error()
    assert L.b4c_grad_clip_coef(None, 4, A, 1, 1.0, 1.0, None, A, None) == -1 and b'grad_clip_coef' in L.b4c_last_error()
    assert L.b4c_grad_clip_coef(A, 4, A, 1, 1.0, 1.0, None, None, None) == -1
    # misaligned
    assert L.b4c_grad_sumsq(A + 4, 4096, 0, 4096, A, None) == -1 and b'aligned' in L.b4c_last_error()
    assert L.b4c_grad_sumsq(A, 4096, 0, 4096, A + 4, None) == -1 and b'aligned' in L.b4c_last_error()
    assert L.b4c_grad_sumsq_rows(A + 8, 4096, 0, 16, 8, A, 4, A, None) == -1 and b'aligned' in L.b4c_last_error()
    assert L.b4c_grad_clip_coef(A, 4, A + 4, 1, 1.0, 1.0, None, A, None) == -1 and b'misaligned' in L.b4c_last_error()
    # ranges / shapes
    assert L.b4c_grad_sumsq(A, 4096, 64, 4097, A, None) == -1 and b'outside the arena' in L.b4c_last_error()
    assert L.b4c_grad_sumsq(A, 4096, 128, 64, A, None) == -1
    assert L.b4c_grad_sumsq_rows(A, 4096, 4000, 16, 8, A, 4, A, None) == -1 and b'outside the arena' in L.b4c_last_error()
    assert L.b4c_grad_clip_coef(A, 5000, A, 1, 1.0, 1.0, None, A, None) == -1 and b'group sums' in L.b4c_last_error()
    assert L.b4c_grad_clip_coef(A, 4, A, 1, 0.0, 1.0, None, A, None) == -1 and b'positive' in L.b4c_last_error()
    assert L.b4c_grad_clip_coef(A, 4, A, 1, float('nan'), 1.0, None, A, None) == -1
    # the clipped Adam forms need the coefficient, and check the rest as the plain forms do
    assert L.b4c_adam_step_clipped(A, A, A, A, 64, 1e-3, 0.9, 0.999, 1e-9, 1.0, None, None) == -1
    assert b'adam_step_clipped' in L.b4c_last_error()
    assert L.b4c_adam_step_clipped(A, A + 4, A, A, 64, 1e-3, 0.9, 0.999, 1e-9, 1.0, A, None) == -1
    assert b'16-byte aligned' in L.b4c_last_error()
    assert L.b4c_adam_rows_clipped(A, A, A, A, A, None, 4, 0, 16, 8, A, 1, 0.9, 0.999, 1e-9, 1.0, None, 1, None) == -1
    assert b'adam_rows_clipped' in L.b4c_last_error()
    assert L.b4c_adam_rows_clipped(A, A, A, A, A, None, 4, 0, 16, 6, A, 1, 0.9, 0.999, 1e-9, 1.0, A, 1, None) == -1
    assert b'multiple of 4' in L.b4c_last_error()
    # empty work is no error and launches nothing
    assert L.b4c_grad_sumsq(A, 4096, 64, 64, A, None) == 0
    assert L.b4c_grad_sumsq_rows(A, 4096, 0, 16, 8, A, 0, A, None) == 0
