"""The long-attention section of include/b4c.h, its binding, the argument refusals of its entry points (NULL device pointers: nothing
is launched), the workspace arithmetic and the host routing of the streamed attention kernels, without a GPU; and the emulated
rounding of route 'mfma' (tests/local_bounds.py) on the shapes tests/test_gpu_attn_long.py runs: what the element bounds must accept."""
import ctypes
import os

import pytest
import torch

import abi_pin
import local_bounds as lb

V_, I, I64, F, U32, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint32, ctypes.c_uint64
FWD = [V_, I, V_, V_, V_, I, V_, I, I, I, I, V_, F, U64, U32]
BWD = [V_, I, V_, V_, V_, I, V_, I, V_, V_, V_, I, I, I, I, I, V_, I64, V_, F, U64, U32]
NAMES = ('o', 'lse', 'dq', 'dk', 'dv')
# the cases of tests/test_gpu_attn_long.py
DENSE = [(2, 513, 2, 64), (2, 768, 1, 32), (2, 769, 4, 32), (2, 1057, 2, 64), (1, 2048, 1, 32), (3, 31, 2, 32), (2, 300, 2, 64)]
PACKED = [([1100, 513, 1, 512, 40, 700, 257], 2, 64), ([600, 33, 1024], 4, 32)]


@pytest.fixture(scope='module')
def L():
    from bert4clickpath_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def ops():
    from bert4clickpath_amd import ops as o
    return o


# ---- header and binding -----------------------------------------------------------------------------------------------------------
def test_header_parses_to_the_declared_table(L):
    sig = L.signatures()
    assert sig['b4c_attn_long_fwd'] == (I, FWD) and sig['b4c_attn_long_bwd'] == (I, BWD)
    assert sig['b4c_attn_long_bwd_workspace_bytes'] == (I64, [I64, I, I])
    const = L.header_constants(L._header_text(L.HEADER_PATH))
    assert {k: v for k, v in const.items() if k.startswith('B4C_ATTN_LONG_')} == {'B4C_ATTN_LONG_MAX_S': 2048}
    assert L.ATTN_LONG_MAX_S == 2048


def test_no_name_is_declared_twice_and_one_header_declares_the_family(L):
    sig = L.signatures()
    assert len(sig) == abi_pin.ENTRY_POINTS and L.ABI_VERSION == abi_pin.ABI_VERSION
    assert os.listdir(os.path.dirname(L.HEADER_PATH)) == ['b4c.h']
    assert {'b4c_attn_long_fwd', 'b4c_attn_long_bwd_workspace_bytes', 'b4c_attn_long_bwd'} <= set(sig)
    with pytest.raises(L.B4CError, match='declares b4c_attn_long_fwd twice'):
        L.parse_header(L._header_text(L.HEADER_PATH) + '\nint b4c_attn_long_fwd(const void *z, int ld_z);\n')


def test_the_binding_checks_the_names(L, monkeypatch, tmp_path):
    lib = L.lib()
    assert lib.b4c_attn_long_fwd.argtypes == FWD and lib.b4c_attn_long_bwd.argtypes == BWD
    assert lib.b4c_attn_long_bwd_workspace_bytes.restype is I64
    more = tmp_path / 'b4c_more.h'
    with open(L.HEADER_PATH) as f:
        more.write_text(f.read() + '\nint b4c_attn_long_not_there(int n);\n')
    monkeypatch.setattr(L, 'HEADER_PATH', str(more))
    monkeypatch.setattr(L, '_lib', None)
    with pytest.raises(L.B4CError, match=r'does not export b4c_attn_long_not_there; rebuild it'):
        L.lib()


# ---- argument refusals: before any pointer is looked at ----------------------------------------------------------------------------
GOOD = dict(B=2, S=600, H=2, dh=64, rate=0.0, flags=0, ws=2 * 600 * 2 * 64 * 4)
NAN = float('nan')
BAD = [('S', dict(S=0)), ('S', dict(S=2049)), ('dh', dict(dh=16)), ('dh', dict(dh=128)), ('dropout_rate', dict(rate=1.0)),
       ('dropout_rate', dict(rate=NAN)), ('flags', dict(flags=2)), ('flags', dict(flags=0x80000001))]


def _fwd(lib, a):
    d = a['H'] * a['dh']
    return lib.b4c_attn_long_fwd(None, 3 * d, None, None, None, d, None, a['B'], a['S'], a['H'], a['dh'], None, a['rate'], 7, a['flags'])


def _bwd(lib, a):
    d = a['H'] * a['dh']
    return lib.b4c_attn_long_bwd(None, 3 * d, None, None, None, d, None, d, None, None, None, 3 * d, a['B'], a['S'], a['H'], a['dh'], None, a['ws'],
                                 None, a['rate'], 7, a['flags'])


@pytest.mark.parametrize('call,who', [(_fwd, 'attn_long_fwd'), (_bwd, 'attn_long_bwd')], ids=['fwd', 'bwd'])
@pytest.mark.parametrize('name,change', BAD, ids=['%s-%s' % (n, '-'.join(str(v) for v in c.values())) for n, c in BAD])
def test_bad_arguments_are_refused_before_any_pointer_is_looked_at(L, call, who, name, change):
    lib = L.lib()
    rc = call(lib, dict(GOOD, **change))
    msg = lib.b4c_last_error().decode()
    assert rc == L._C['B4C_EINVAL'], (rc, msg)
    assert msg.startswith(who + ':') and name in msg, msg


def test_a_short_workspace_and_null_pointers_are_refused(L):
    lib = L.lib()
    rc = _bwd(lib, dict(GOOD, ws=GOOD['ws'] - 1))
    msg = lib.b4c_last_error().decode()
    assert rc == L._C['B4C_EINVAL'] and msg.startswith('attn_long_bwd:') and 'workspace_bytes' in msg, msg
    for call in (_fwd, _bwd):           # every scalar good: the pointers are what is left
        assert call(lib, GOOD) == L._C['B4C_EINVAL'] and 'null pointer' in lib.b4c_last_error().decode()


def test_workspace_bytes_arithmetic(L):
    ws = L.lib().b4c_attn_long_bwd_workspace_bytes
    assert ws(2 * 600, 2, 64) == 2 * 600 * 2 * 64 * 4 and ws(1, 1, 32) == 128 and ws(0, 4, 32) == 0
    assert ws(2 ** 31, 4, 64) == 2 ** 31 * 4 * 64 * 4                  # 64-bit
    assert ws(10, 2, 16) == -1 and ws(10, 2, 128) == -1 and ws(-1, 2, 64) == -1 and ws(10, 0, 64) == -1


# ---- routing ------------------------------------------------------------------------------------------------------------------------
def _model(dtype, d=64, H=2):
    from bert4clickpath_amd.clickstream_transformer import ClickstreamTransformer, SoftMaxHead
    return ClickstreamTransformer({'items': ['asin']}, {'items': ['i%d' % i for i in range(20)]}, {'items': d}, SoftMaxHead([16], 20),
                                  value_to_head='[MASK]', num_encoder_layers=1, num_attention_heads=H, dropout_rate=0.0, compute_dtype=dtype)


def test_routing_predicates_with_the_switch_on_and_off(ops, monkeypatch):
    from bert4clickpath_amd._lib import B4CError
    assert ops.long_attn is (os.environ.get('B4C_ATTN_LONG', '0') == '1') and ops.ATTN_LONG_MAX_S == 2048
    bf, f32 = torch.bfloat16, torch.float32
    assert ops.attn_long_supported(bf, 513, 64) and ops.attn_long_supported(bf, 2048, 32) and ops.attn_long_supported(bf, 1, 64)
    assert not ops.attn_long_supported(bf, 2049, 64) and not ops.attn_long_supported(bf, 0, 64)
    assert not ops.attn_long_supported(bf, 600, 16) and not ops.attn_long_supported(bf, 600, 128) and not ops.attn_long_supported(f32, 600, 64)
    m, m32, m16 = _model(bf), _model(f32), _model(bf, d=64, H=4)
    feats = {'asin': torch.zeros(2, 597, dtype=torch.int64)}                 # encoder length 597 + 3 = 600
    monkeypatch.setattr(ops, 'long_attn', False)
    assert m.transformer.packed_supported(512) and not m.transformer.packed_supported(513) and not m.transformer.packed_supported(600)
    assert m._use_packed(feats, None, 100) is False
    with pytest.raises(B4CError, match=r'^packed=True needs bf16 compute, head depth 32 / 64 and an encoder length <= 512$'):
        m._use_packed(feats, True, None)
    monkeypatch.setattr(ops, 'long_attn', True)
    assert m.transformer.packed_supported(600) and m.transformer.packed_supported(2048) and not m.transformer.packed_supported(2049)
    assert not m32.transformer.packed_supported(600) and not m16.transformer.packed_supported(600)        # fp32; head depth 16
    assert m._use_packed(feats, None, 100) is True and m._use_packed(feats, True, None) is True
    assert m._use_packed(feats, False, 100) is False
    with pytest.raises(B4CError, match='<= 2048'):
        m32._use_packed(feats, True, None)


# ---- the rounding steps of route 'mfma' stay inside the bounds on the GPU test's shapes -------------------------------------------------
@pytest.mark.parametrize('pattern', lb.PATTERNS)
@pytest.mark.parametrize('B,S,H,dh', DENSE)
def test_dense_emulated_rounding_is_accepted(B, S, H, dh, pattern):
    qkv, pad, do = lb.dense_inputs(torch.bfloat16, B, S, H, dh, pattern)
    res = lb.attn_dense(qkv, pad, do, B, S, H, dh, 'mfma')
    d = H * dh
    items = [(b * S, (b + 1) * S, b * S, (b + 1) * S) for b in range(B)]
    em = lb.attn_emulate(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], do, items, ~pad.bool().reshape(-1), H, dh, 'mfma')
    em['lse'] = em['lse'].reshape(B, S, H).permute(0, 2, 1)
    ratios = {n: lb.check('(%d,%d,%d,%d)-%s %s' % (B, S, H, dh, pattern, n), em[n], *res[n]) for n in NAMES}
    print('RATIO attn long emulated (%d,%d,%d,%d)-%s %s' % (B, S, H, dh, pattern, ' '.join('%s=%.3f' % (n, ratios[n]) for n in NAMES)))


@pytest.mark.parametrize('lens,H,dh', PACKED, ids=lambda v: str(v).replace(' ', ''))
def test_packed_emulated_rounding_is_accepted(lens, H, dh):
    qkv, cu, do = lb.packed_inputs(lens, H, dh)
    res = lb.attn_packed(qkv, cu, do, H, dh, 'mfma')
    d = H * dh
    items = [(int(cu[b]), int(cu[b + 1]), int(cu[b]), int(cu[b + 1])) for b in range(len(lens))]
    em = lb.attn_emulate(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], do, items, torch.ones(sum(lens), dtype=torch.bool), H, dh, 'mfma')
    for n in NAMES:
        lb.check('packed %s %s' % (lens, n), em[n], *res[n])
