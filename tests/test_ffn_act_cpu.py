"""Host side of the fused GELU feed-forward kernels (no GPU): the two entry points in the header and the library at the pinned ABI version, the
switch and what it does to the vocabulary head's sweep, and the argument checks that refuse a call before any launch."""
import subprocess
import sys
import os

import torch

import abi_pin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 1 << 20                                                       # a well-aligned, never dereferenced "pointer"


def test_the_entry_points_are_declared_and_exported_at_abi_12():
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    sig = _lib.signatures()
    for name, n_args in (('b4c_ffn_act_fwd', 25), ('b4c_ffn_act_bwd', 33)):
        assert name in sig and name in _lib.declared_symbols() and hasattr(L, name)
        assert len(sig[name][1]) == n_args
    # the ReLU pair's lists plus act and U, ldu; the old lists are as they were
    assert len(sig['b4c_ffn_fwd'][1]) == 22 and len(sig['b4c_ffn_bwd'][1]) == 30
    assert [s for s in _lib.declared_symbols() if not hasattr(L, s)] == []
    assert len(_lib.signatures()) == abi_pin.ENTRY_POINTS == len(_lib.declared_symbols())
    assert _lib.ABI_VERSION == abi_pin.ABI_VERSION and L.b4c_abi_version() == abi_pin.ABI_VERSION      # additive: no existing signature changed


def test_the_switch_is_off_by_default():
    """(a fresh interpreter without the variable: this process may have been started with it)"""
    env = {k: v for k, v in os.environ.items() if k != 'B4C_FUSED_FFN_GELU'}
    out = subprocess.run([sys.executable, '-c', 'from bert4clickpath_amd import ops; print(ops.fused_ffn_gelu)'], cwd=ROOT, env=env,
                         capture_output=True, text=True, check=True).stdout.split()
    assert out[-1] == 'False'


def test_background_sweep_follows_the_switch_for_gelu_models_only():
    from bert4clickpath_amd import ops
    bf16, f32 = torch.bfloat16, torch.float32
    prev = ops.fused_ffn_gelu, ops.overlap_vocab_dw, ops.fused_ffn_bwd
    try:
        ops.overlap_vocab_dw, ops.fused_ffn_bwd = None, True
        for flag in (False, True):
            ops.fused_ffn_gelu = flag
            for act in ('gelu', 'gelu_tanh'):
                assert ops.background_dw_expected(128, 100, bf16, act) is (not flag)
                # outside the fused shape a GELU model keeps the background sweep either way
                assert ops.background_dw_expected(128, 512, bf16, act) is True
                assert ops.background_dw_expected(256, 100, bf16, act) is True
                assert ops.background_dw_expected(128, 100, f32, act) is True
            # the ReLU answers do not depend on it
            assert ops.background_dw_expected(128, 100, bf16) is False
            assert ops.background_dw_expected(128, 100, bf16, 'relu') is False
            assert ops.background_dw_expected(128, 512, bf16, 'relu') is True
            assert ops.background_dw_expected(128, 100, f32, 'relu') is True
        ops.fused_ffn_gelu, ops.fused_ffn_bwd = True, False          # without the fused backward nothing holds whole CUs
        assert ops.background_dw_expected(128, 100, bf16, 'gelu') is True
    finally:
        ops.fused_ffn_gelu, ops.overlap_vocab_dw, ops.fused_ffn_bwd = prev


def _fwd(L, act, U, Z, ldu=104):
    # (X, ldx, W1t, ldw1, b1, W2t, ldw2, b2, gamma, beta, F, Fp, act, H, ldh, U, ldu, Z, Out, stats, M, eps, rate, seed, stream)
    return L.b4c_ffn_act_fwd(A, 128, A, 128, A, A, 104, A, A, A, 100, 104, act, A, 104, U, ldu, Z, A, A if Z else None, 4096, 1e-6, 0.1,
                             1, None)


def _bwd(L, act, U, M=4096, ws_bytes=1 << 30):
    # (dout, z, stats, gamma, rate, seed, act, H, ldh, U, ldu, X, ldx, W2c, ldw2, W1c, ldw1, F, Fp, dX, ldo, dW1, ld_dw1, db1, dW2,
    #  ld_dw2, db2, dgamma, dbeta, M, workspace, workspace_bytes, stream)
    return L.b4c_ffn_act_bwd(A, A, A, A, 0.1, 1, act, A, 104, U, 104, A, 128, A, 128, A, 104, 100, 104, A, 128, A, 100, A, A, 128, A, A, A,
                             M, A, ws_bytes, None)


def test_bad_arguments_are_refused_without_a_launch():
    """(every call here would fault on its made-up pointers if it were launched, and there is no device to launch on)"""
    from bert4clickpath_amd import _lib
    L = _lib.lib()
    for act in (_lib.ACT_NONE, _lib.ACT_RELU, 4, -1):
        assert _fwd(L, act, A, A) == -1
        assert b'ffn_act_fwd: act' in L.b4c_last_error()
        assert _bwd(L, act, A) == -1
        assert b'ffn_act_bwd: act' in L.b4c_last_error()
    for act in (_lib.ACT_GELU, _lib.ACT_GELU_TANH):
        assert _fwd(L, act, None, A) == -1                            # a training call (Z given) without U
        assert b'ffn_act_fwd' in L.b4c_last_error() and b'pre-activation' in L.b4c_last_error()
        assert _fwd(L, act, A + 8, A) == -1
        assert b'16-byte aligned' in L.b4c_last_error()
        assert _fwd(L, act, A, A, ldu=96) == -1                       # a pitch below the padded width
        assert b'ffn_act_fwd: shape' in L.b4c_last_error()
        assert _bwd(L, act, None) == -1
        assert b'ffn_act_bwd: null pointer' in L.b4c_last_error()
        assert _bwd(L, act, A, M=1 << 24) == -1                       # the row limit of b4c_ffn_bwd
        assert b'ffn_act_bwd' in L.b4c_last_error() and b'16,777,216' in L.b4c_last_error()
        assert _bwd(L, act, A, ws_bytes=L.b4c_ffn_bwd_workspace_bytes(4096) - 1) == -1
        assert b'workspace too small' in L.b4c_last_error()
