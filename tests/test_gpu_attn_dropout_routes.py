"""Attention-probability dropout on every kernel body and launch route of the full layer (ops.attn_fwd / ops.attn_bwd with
rate > 0: the DROP = true instantiations of csrc/attn.hip and csrc/attn_mfma.hip, which a training step with
attention_dropout_rate > 0 launches instead of the widely tested DROP = false ones).  The checker is the float64 restatement
tests/attn_dropout_ref.py with the keep masks regenerated on the host (ops.attn_keep_mask); tests/test_attn_dropout_cpu.py shows
the recovery construction of part 1 on that restatement alone.

1. exact mask recovery at any length (test_outputs_are_the_masks*): q = k = 0 and one-hot V / dO windows of dh keys / queries, in
   ceil(S / dh) passes; the nonzero patterns of o and dV ARE mask AND NOT pad, per (sequence, head), no tolerance.
2. float64 parity on the attention grid of tests/test_gpu_kernels.py (test_parity_*), that file's bounds unwidened.
3. a bf16 encoder, dense and packed, with every mask regenerated (test_encoder_bf16_*).

Which case reaches which kernel body (the routes follow from the launch code of attn_mfma.hip: head depth 32 / 64 and S <= 512
run the matrix-core kernels; the forward takes QPW = 2 for S > 256; the backward is resident while its LDS image fits -- S <= 224
at depth 64, S <= 256 at depth 32 --, else walks blocks of 256 keys, with a workspace iff S > 256, which every case asserts):

  row forward, row dQ, row dKV
      recovery: fp32 (2,70,1,16) (2,130,2,64) (2,257,1,32) (1,300,2,128) -- a second key tile (S > 64), a second query block
                (S > 256), every head depth; the bf16 fallbacks (2,70,1,16) (1,40,1,128) (1,516,1,32)
      parity:   fp32 (2,70,1,16) (2,129,3,64) (2,257,1,32) (1,300,2,128); the bf16 fallbacks (2,70,1,16) (1,300,2,128)
  MFMA forward, QPW = 1
      recovery: every bf16 case with S <= 256 and depth 32 / 64
      parity:   (3,13,2,32) (2,200,2,64) (2,256,2,64) (2,33,4,32) (2,129,3,64), sparse dO, 260 items
  MFMA forward, QPW = 2
      recovery: (2,300,1,64): a partial last key tile; (1,512,2,32); packed, max_len 300
      parity:   (3,257,2,64) (2,300,2,32) (1,481,1,64) (2,512,4,64)
  resident backward
      recovery: (2,224,2,64): 7 key tiles, its limit at depth 64; (2,256,2,32): 8 tiles; (2,5,2,64): S4 = 8 != S; (1,1,1,32);
                (130,33,2,64); packed [224,7,97] at depth 32
      parity:   (3,13,2,32) (2,200,2,64) (2,33,4,32) (2,129,3,64), sparse dO, 260 items
  key-block backward, one block
      recovery: (2,256,2,64): 8 key tiles
      parity:   (2,256,2,64)
  key-block backward, two blocks
      recovery: (2,300,1,64); (1,512,2,32): the largest lane part of the hash counter; packed [257,1,40,300,33] at depth 64:
                sequences that end before the second block
      parity:   (3,257,2,64) (2,300,2,32) (1,481,1,64) (2,512,4,64)

Skip paths run together with DROP:
  sLive / tile_live (key tiles whose keys are all padded: skipped by the forward, zero dS columns in both backward bodies):
      sequence 1 of every dense case with B > 1 pads its keys 5 .. S-2, whole key tiles in the middle, in (1) and in (2).
  sNZ (query tiles whose dO is all +0, resident backward): every backward pass of (1) -- a window of dh queries leaves the other
      query tiles zero --, test_parity_sparse_do and the 260-item case of (2).
  the item loop of the resident backward (attn_ctr_base(item, S_arg), B*H above the CU count): (130,33,2,64) of (1), every item
      compared; (130,72,2,64) of (2).
  the fp32 row dQ kernel loads its hash before the sPad skip: every padded fp32 case of (1) and (2).
The row dKV kernel hashes one element per (query, key), the forward and dQ four keys at a time: (1) compares both against the
host mask at every key of every fp32 case."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_dropout_ref as ref  # noqa: E402
import bf16_gates  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
# bounds of tests/test_gpu_kernels.py::test_attention_fwd_bwd, unwidened (dropout only scales kept terms by 1 / (1 - rate))
TOL_O = {F32: 2e-5, BF16: 1.2e-2}           # relative L2
TOL_LSE = {F32: 1e-4, BF16: 3e-2}           # absolute
TOL_G = {F32: 1e-4, BF16: 2.5e-2}           # relative L2


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    from bert4clickpath_amd import ops
    return ops


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _workspace_route(ops, dtype, B, S_arg, H, dh):
    """the one observable of the launch code: the key-block backward with more than one block wants a workspace"""
    need = ops.L.lib().b4c_attn_bwd_workspace_bytes(B, S_arg, H, dh, ops.dt_code(dtype))
    mfma = dtype == BF16 and dh in (32, 64) and S_arg <= 512
    assert (need > 0) == (mfma and S_arg > 256), (need, S_arg, dh)
    return need


# ---- 1. exact mask recovery ---------------------------------------------------------------------------------------------------
def _recover(ops, dtype, lens, packed, H, dh, seed, rate=0.25):
    """runs the passes -> (fwd, bwd: bool [H, L, L] per sequence, [h][query][key]; want: the same from the host mask; pad [T])"""
    B, S_arg = len(lens), max(lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    d, T = H * dh, int(off[-1])
    cu = torch.tensor(off, dtype=torch.int32, device='cuda') if packed else None
    pad = torch.zeros(T, dtype=torch.uint8) if packed else ref.recovery_pads(B, S_arg).reshape(-1)      # packed: no pads
    padd = pad.cuda()
    n_real = [int((pad[off[b]:off[b] + L] == 0).sum()) for b, L in enumerate(lens)]
    assert min(n_real) >= 1
    keep = ops.attn_keep_mask(seed, B, H, S_arg, rate)
    fwd = [torch.zeros(H, L, L, dtype=torch.bool) for L in lens]
    bwd = [torch.zeros(H, L, L, dtype=torch.bool) for L in lens]
    for p in range(ref.recovery_passes(S_arg, dh)):
        qkv, do = ref.recovery_operands(lens, H, dh, p, dtype)
        qkv, do = qkv.cuda(), do.cuda()
        o, lse = ops.attn_fwd(qkv, padd, B, S_arg, H, dh, cu, rate, seed)
        dqkv = ops.attn_bwd(qkv, padd, o, do, lse, B, S_arg, H, dh, cu, None, rate, seed)
        torch.cuda.synchronize()
        assert not dqkv[:, :2 * d].any(), ('dQ, dK', p)                       # exactly zero: k = 0, and q = 0
        lse = lse.cpu()
        for b, L in enumerate(lens):                                          # that of the undropped softmax: uniform probabilities
            assert float((lse[b, :, :L] - float(np.log(n_real[b]))).abs().max()) < 1e-4, ('lse', b, p)
        ref.recovery_collect(fwd, bwd, o.float().cpu(), dqkv[:, 2 * d:].float().cpu(), lens, H, dh, p)
    want = [keep[b, :, :L, :L] & (pad[off[b]:off[b] + L] == 0)[None, None, :] for b, L in enumerate(lens)]
    return fwd, bwd, want


def _assert_masks(fwd, bwd, want):
    for b, w in enumerate(want):
        for h in range(w.shape[0]):
            for name, got in (('o', fwd), ('dV', bwd)):
                if not torch.equal(got[b][h], w[h]):
                    bad = (got[b][h] != w[h]).nonzero()
                    raise AssertionError('%s of sequence %d, head %d differs from mask AND NOT pad at %d (query, key) pairs, the first %s'
                                         % (name, b, h, bad.shape[0], bad[:6].tolist()))
    kept = torch.cat([w.reshape(-1) for w in want]).float().mean()
    return float(kept)


DENSE_BF16 = [(2, 224, 2, 64), (2, 256, 2, 64), (2, 256, 2, 32), (2, 300, 1, 64), (1, 512, 2, 32), (2, 5, 2, 64), (1, 1, 1, 32),
              (130, 33, 2, 64)]
DENSE_F32 = [(2, 70, 1, 16), (2, 130, 2, 64), (2, 257, 1, 32), (1, 300, 2, 128)]
DENSE_BF16_ROWS = [(2, 70, 1, 16), (1, 40, 1, 128), (1, 516, 1, 32)]          # bf16 outside the MFMA kernels: the row kernels


@pytest.mark.parametrize('dtype,B,S,H,dh', [(BF16,) + c for c in DENSE_BF16] + [(F32,) + c for c in DENSE_F32]
                         + [(BF16,) + c for c in DENSE_BF16_ROWS])
def test_outputs_are_the_masks(ops, dtype, B, S, H, dh):
    """dense layout.  Sequence 0 pads its last 4 keys, sequence 1 the keys 5 .. S-2 (key 0 stays real at S = 5 and S = 1)."""
    _workspace_route(ops, dtype, B, S, H, dh)
    if (B, S) == (130, 33):
        assert B * H > torch.cuda.get_device_properties(0).multi_processor_count      # several items per workgroup
    fwd, bwd, want = _recover(ops, dtype, [S] * B, False, H, dh, 0xA11CE + 131 * S + dh + B)
    kept = _assert_masks(fwd, bwd, want)                                      # every sequence, every head
    if S >= 70:         # the masks are masks: 0.75 of the unpadded (query, key) pairs, thousands of them, within a tenth
        real = float((ref.recovery_pads(B, S) == 0).float().mean())
        assert 0.9 * 0.75 * real < kept < 1.1 * 0.75 * real


@pytest.mark.parametrize('lens,H,dh', [([257, 1, 40, 300, 33], 2, 64), ([224, 7, 97], 2, 32)])
def test_outputs_are_the_masks_packed(ops, lens, H, dh):
    """packed layout, bf16: q, k count from cu[b] and the pitch of the rule is max_len; no pads (the packed layout has none)"""
    _workspace_route(ops, BF16, len(lens), max(lens), H, dh)
    fwd, bwd, want = _recover(ops, BF16, lens, True, H, dh, 0xBEE5 + sum(lens) + dh)
    kept = _assert_masks(fwd, bwd, want)
    assert 0.72 < kept < 0.78


# ---- 2. parity against float64 ---------------------------------------------------------------------------------------------------
def _grid_pad(B, S):
    pad = torch.zeros(B, S, dtype=torch.uint8)              # tests/test_gpu_kernels.py::test_attention_fwd_bwd
    pad[0, S - 4:] = 1
    if B > 1:
        pad[1, 5:S - 1] = 1
    return pad


def _run(ops, qd, padd, dod, B, S, H, dh, rate, seed):
    o, lse = ops.attn_fwd(qd, padd, B, S, H, dh, None, rate, seed)
    dqkv = ops.attn_bwd(qd, padd, o, dod, lse, B, S, H, dh, None, None, rate, seed)
    return o, lse, dqkv


PARITY_BF16 = [(3, 13, 2, 32), (2, 200, 2, 64), (2, 256, 2, 64), (2, 33, 4, 32), (2, 129, 3, 64), (3, 257, 2, 64), (2, 300, 2, 32),
               (1, 481, 1, 64), (2, 512, 4, 64), (2, 70, 1, 16), (1, 300, 2, 128)]
PARITY_F32 = [(2, 70, 1, 16), (2, 129, 3, 64), (2, 257, 1, 32), (1, 300, 2, 128)]


@pytest.mark.parametrize('dtype,B,S,H,dh', [(BF16,) + c for c in PARITY_BF16] + [(F32,) + c for c in PARITY_F32])
def test_parity_on_the_attention_grid(ops, dtype, B, S, H, dh):
    rate, seed = 0.2, 0xD0D0 + 17 * S + dh
    _workspace_route(ops, dtype, B, S, H, dh)
    g = torch.Generator().manual_seed(S + dh)
    d = H * dh
    qd = (torch.randn(B * S, 3 * d, generator=g) * 0.8).to(dtype).cuda()
    dod = torch.randn(B * S, d, generator=g).to(dtype).cuda()
    pad = _grid_pad(B, S)
    padd = pad.cuda()
    keep = ops.attn_keep_mask(seed, B, H, S, rate)
    o_ref, lse_ref, g_ref = ref.attention_grads(qd, dod, pad, B, S, H, dh, keep, rate)
    o, lse, dqkv = _run(ops, qd, padd, dod, B, S, H, dh, rate, seed)
    e_o, e_g = rel_err(o, o_ref), rel_err(dqkv, g_ref)
    e_l = float((lse.double().cpu() - lse_ref).abs().max())
    print('attention dropout %s (%d,%d,%d,%d): rel_err(o) %.3e  |dlse| %.3e  rel_err(dqkv) %.3e' % (dtype, B, S, H, dh, e_o, e_l, e_g))
    assert e_o < TOL_O[dtype]
    assert e_l < TOL_LSE[dtype]
    assert e_g < TOL_G[dtype]
    kv_grad = dqkv[:, d:].reshape(B, S, 2 * d)                                # padded keys: exactly zero dK / dV
    assert float(kv_grad[0, S - 4:].abs().max()) == 0.0
    if B > 1:
        assert float(kv_grad[1, 5:S - 1].abs().max()) == 0.0
    again = ops.attn_bwd(qd, padd, o, dod, lse, B, S, H, dh, None, None, rate, seed)
    assert torch.equal(again, dqkv)
    o0, lse0 = ops.attn_fwd(qd, padd, B, S, H, dh)                            # the rate-0 launch: another o, the same lse bits
    assert not torch.equal(o0, o)
    assert torch.equal(lse0, lse)


@pytest.mark.parametrize('B,S,H,dh', [(3, 200, 2, 64), (2, 224, 1, 64), (3, 130, 2, 32)])
def test_parity_sparse_do(ops, B, S, H, dh):
    """the shapes and the dO / pad layout of tests/test_gpu_kernels.py::test_attention_bwd_zero_do_tiles, with dropout: the query
    tiles the resident backward skips (sNZ) next to the keep bits of the tiles it visits"""
    rate, seed = 0.2, 0x5A5A + S
    g = torch.Generator().manual_seed(7 * S + dh)
    d = H * dh
    qkv = torch.randn(B * S, 3 * d, generator=g) * 0.8
    pad = torch.zeros(B, S, dtype=torch.uint8)
    pad[0, 70:S - 1] = 1
    pad[1, 33:] = 1
    do = torch.randn(B, S, d, generator=g)
    do[0, 64:S - 1] = 0.0
    do[1, 32:] = 0.0
    if B > 2:
        do[2] = 0.0
    qd, dod, padd = qkv.to(BF16).cuda(), do.reshape(B * S, d).to(BF16).cuda(), pad.cuda()
    keep = ops.attn_keep_mask(seed, B, H, S, rate)
    _, _, g_ref = ref.attention_grads(qd, dod, pad, B, S, H, dh, keep, rate)
    o, lse, dqkv = _run(ops, qd, padd, dod, B, S, H, dh, rate, seed)
    e_g = rel_err(dqkv, g_ref)
    print('attention dropout, sparse dO (%d,%d,%d,%d): rel_err(dqkv) %.3e' % (B, S, H, dh, e_g))
    assert e_g < 2.5e-2
    dq = dqkv[:, :d].reshape(B, S, d)
    assert float(dq[1, 32:].abs().max()) == 0.0 and float(dq[0, 64:S - 1].abs().max()) == 0.0
    if B > 2:
        assert float(dqkv.reshape(B, S, 3 * d)[2].abs().max()) == 0.0
    dneg = dod.clone()                                                        # the zero rows as -0: the dense path; dK / dV must not move
    dneg[(dod == 0).all(dim=1)] = -0.0
    dqkv2 = ops.attn_bwd(qd, padd, o, dneg, lse, B, S, H, dh, None, None, rate, seed)
    assert torch.equal(dqkv2[:, d:], dqkv[:, d:])
    assert torch.equal(dqkv2[:, :d].float().abs(), dqkv[:, :d].float().abs())


def test_parity_more_items_than_workgroups(ops):
    """B * H = 260 items on 256 CUs with dropout: the persistent grid of the resident backward hands some workgroups a second item,
    whose hash counter starts at attn_ctr_base(item, S_arg).  Bounds: those of test_attention_bwd_more_items_than_workgroups."""
    rate, seed = 0.2, 0x17E45
    g = torch.Generator().manual_seed(11)
    B, S, H, dh = 130, 72, 2, 64
    d = H * dh
    assert B * H > torch.cuda.get_device_properties(0).multi_processor_count
    qkv = torch.randn(B * S, 3 * d, generator=g) * 0.7
    lens = torch.randint(5, S + 1, (B,), generator=g)
    pad = (torch.arange(S)[None, :] >= lens[:, None]).to(torch.uint8)
    do = torch.randn(B, S, d, generator=g)
    do[pad.bool()] = 0.0
    do[::7] = 0.0
    qd, dod, padd = qkv.to(BF16).cuda(), do.reshape(B * S, d).to(BF16).cuda(), pad.cuda()
    keep = ops.attn_keep_mask(seed, B, H, S, rate)
    o_ref, _, g_ref = ref.attention_grads(qd, dod, pad, B, S, H, dh, keep, rate)
    o, lse, dqkv = _run(ops, qd, padd, dod, B, S, H, dh, rate, seed)
    e_o, e_g = rel_err(o, o_ref), rel_err(dqkv, g_ref)
    print('attention dropout, 260 items: rel_err(o) %.3e  rel_err(dqkv) %.3e' % (e_o, e_g))
    assert e_o < 1.2e-2
    assert e_g < 2.5e-2
    assert float(dqkv.reshape(B, S, 3 * d)[::7].abs().max()) == 0.0
    again = ops.attn_bwd(qd, padd, o, dod, lse, B, S, H, dh, None, None, rate, seed)     # the item order differs, the result does not
    assert torch.equal(again, dqkv)


# ---- 3. encoder level, bf16 ------------------------------------------------------------------------------------------------------
ENC_LENS = [70, 33, 9]          # of S = 72: ragged pads; the packed pitch max_len = 70 is not S


def _scatter(rows, real, B, S, d):
    """[T, d] values of the packed rows -> [B, S, d], ones at the pads (which the packed layout does not compute)"""
    full = torch.ones(B * S, d, dtype=rows.dtype)
    full[real.reshape(-1)] = rows
    return full.view(B, S, d)


@pytest.mark.parametrize('layout', ['dense', 'packed'])
@pytest.mark.parametrize('d', [128, 64])                   # two heads: head depth 64 and 32, both matrix-core depths
def test_encoder_bf16_matches_fp64_with_every_mask_regenerated(ops, d, layout):
    """A two-layer bf16 encoder with GELU (no ReLU: no gate pattern to share with the reference, as tests/test_gpu_paper_model.py
    argues), residual dropout 0.1 and attention dropout 0.2, against the float64 restatement with every mask regenerated in the
    order the encoder draws its seeds (input, then per layer residual 1, residual 2, attention).  In the packed layout the masks of
    the residual branches run over the T packed rows and the pitch of the attention mask is max_len.

    Bound: bf16_gates.BF16_GRAD_BOUND (0.03 relative L2) for the output, x.grad and every parameter gradient (the key bias left
    out by bf16_gates.grad_errors).  Measured on the MI355X (relative L2: output; worst parameter gradient; x.grad):
        d_model 128, dense    6.0e-3   1.14e-2 (enc_layers.1.mha.wk.kernel)   9.1e-3
        d_model 128, packed   5.8e-3   1.22e-2 (enc_layers.1.mha.wq.kernel)   8.7e-3
        d_model  64, dense    6.0e-3   1.41e-2 (enc_layers.1.mha.wq.bias)     9.0e-3
        d_model  64, packed   5.8e-3   1.14e-2 (enc_layers.1.mha.wk.kernel)   8.3e-3
    This bound does NOT see a single wrong four-key group of a mask: at S = 72 that moves a gradient by well under the bf16
    rounding error.  test_outputs_are_the_masks is the check for that; this test holds the arithmetic of the rescaling, of lse
    and of delta across two layers and through both layouts."""
    from bert4clickpath_amd.clickstream_transformer import transformer as T
    torch.manual_seed(5 + d)
    B, S, H, NL, rate, a_rate, act = 3, 72, 2, 2, 0.1, 0.2, 'gelu_tanh'
    enc = T.Encoder(num_layers=NL, d_model=d, num_heads=H, dff=100, dropout_rate=rate, attention_dropout_rate=a_rate,
                    ffn_activation=act).cuda()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith('bias') or n.endswith('beta'):
                p.normal_(0, 0.05)
    lens = torch.tensor(ENC_LENS)
    pad = (torch.arange(S)[None, :] >= lens[:, None]).to(torch.uint8)
    real = pad == 0
    xh = torch.randn(B, S, d).to(BF16)
    wgt = torch.randn(B, S, d).to(BF16)
    T_tok, max_len = int(real.sum()), int(lens.max())
    T.set_dropout_seed(2024)
    if layout == 'packed':
        src = real.reshape(-1).nonzero().reshape(-1)
        cu = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).to(torch.int32)
        packed_of = torch.full((B * S,), -1, dtype=torch.int32)
        packed_of[src] = torch.arange(T_tok, dtype=torch.int32)
        pk = ops.Packed(cu.cuda(), src.to(torch.int32).cuda(), packed_of.cuda(), B, S, T_tok, max_len)
        x = xh[real].view(1, T_tok, d).cuda().requires_grad_(True)
        out = enc(x, training=True, mask=torch.zeros(T_tok, dtype=torch.uint8, device='cuda'), packed=pk)
        w_dev = wgt[real].view(1, T_tok, d).cuda()
        wgt = wgt * real[:, :, None]                      # the pads of the reference reach no loss
    else:
        x = xh.cuda().requires_grad_(True)
        out = enc(x, training=True, mask=pad.cuda())
        w_dev = wgt.cuda()
    (out.float() * w_dev.float()).sum().backward()
    torch.cuda.synchronize()

    stream = T._SeedStream(2024)
    rows, S_attn = (T_tok, max_len) if layout == 'packed' else (B * S, S)

    def res_mask(seed):
        m = torch.from_numpy(ops.keep_mask(seed, rows * d, rate)).view(rows, d)
        return _scatter(m, real, B, S, d) if layout == 'packed' else m.view(B, S, d)

    def attn_mask(seed):
        full = torch.ones(B, H, S, S, dtype=torch.bool)
        full[:, :, :S_attn, :S_attn] = ops.attn_keep_mask(seed, B, H, S_attn, a_rate)
        return full
    keep_in = res_mask(stream.next())
    keep_res, keep_attn = {}, []
    for i in range(NL):
        keep_res['l%d.1' % i] = res_mask(stream.next())
        keep_res['l%d.2' % i] = res_mask(stream.next())
        keep_attn.append(attn_mask(stream.next()))
    assert T.dropout_seeds.counter == stream.counter == 1 + 3 * NL
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in enc.named_parameters()}
    xr = xh.double().requires_grad_(True)
    ro = ref.encoder_forward(ref.dropout(xr, rate, keep_in), pad, P, NL, H, rate, a_rate, keep_res, keep_attn, act)
    (ro * wgt.double()).sum().backward()

    if layout == 'packed':
        out_ref, gx_ref, gx = ro.detach()[real], xr.grad[real], x.grad.view(T_tok, d)
        e_out = rel_err(out.view(T_tok, d), out_ref)
    else:
        out_ref, gx_ref, gx = ro.detach(), xr.grad, x.grad
        e_out = rel_err(out, out_ref)
    errs = bf16_gates.grad_errors(enc.named_parameters(), {n: t.grad for n, t in P.items()})
    assert len(errs) == len(P) - NL                                           # every tensor but the key biases
    errs['x'] = rel_err(gx, gx_ref)
    worst = max(errs, key=errs.get)
    print('encoder bf16 with attention dropout, d_model %d, %s: rel_err(out) %.3e  worst gradient %s %.3e  x.grad %.3e'
          % (d, layout, e_out, worst, errs[worst], errs['x']))
    assert e_out < bf16_gates.BF16_GRAD_BOUND
    for n, e in errs.items():
        assert e < bf16_gates.BF16_GRAD_BOUND, (n, e)
