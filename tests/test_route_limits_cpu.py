"""Row limits of the fused backward routes (CPU: the predicates only look at shapes, so meta tensors of 16.7 M rows cost nothing).

b4c_ffn_bwd and b4c_attn_out_bwd address their row chunks with 32-bit byte offsets and refuse M >= 2^24; b4c_gemm_dxdw with a
residual refuses M * pitch * 2 >= 2^32.  The predicates that pick these routes must refuse the same shapes, so that the autograd
blocks fall back to the unfused kernels instead of raising B4CError in backward (tests/test_gpu_route_limits.py runs that)."""
import torch

from bert4clickpath_amd import ops

LIMIT = 1 << 24


def _t(rows, cols, dtype=torch.bfloat16):
    return torch.empty(rows, cols, dtype=dtype, device='meta')


def test_ffn_bwd_supported_row_limit():
    for rows, ok in ((4096, True), (LIMIT - 1, True), (LIMIT, False), (LIMIT + 13, False)):
        assert ops.ffn_bwd_supported(_t(rows, 128), _t(rows, 104), _t(rows, 128)) is ok, rows
    # the shape check alone (it also decides the foreground dW sweep) does not depend on the row count
    assert ops.ffn_bwd_shape_ok(_t(LIMIT, 128), _t(LIMIT, 104), _t(LIMIT, 128))


def test_attn_out_bwd_supported_row_limit():
    for rows, ok in ((4096, True), (LIMIT - 1, True), (LIMIT, False), (LIMIT + 13, False)):
        assert ops.attn_out_bwd_supported(_t(rows, 128), _t(rows, 128)) is ok, rows


def test_dxdw_supported_residual_byte_bound():
    # Q | K | V route: residual = dz [M, 128]: M * 128 * 2 < 2^32 <=> M < 2^24
    for rows, ok in ((LIMIT - 1, True), (LIMIT, False)):
        assert ops.dxdw_supported(_t(rows, 128), _t(rows, 384), 3, residual=_t(rows, 128)) is ok, rows
    # the bound is on the residual's pitch, not its width: a wider pitch reaches it with fewer rows
    res = _t(LIMIT // 2, 256)[:, :128]
    assert ops.dxdw_supported(_t(LIMIT // 2, 128), _t(LIMIT // 2, 384), 3, residual=res) is False
    res = _t(LIMIT // 2 - 1, 256)[:, :128]
    assert ops.dxdw_supported(_t(LIMIT // 2 - 1, 128), _t(LIMIT // 2 - 1, 384), 3, residual=res) is True
    # without a residual there is no byte bound (the tiles' DMA descriptors carry 64-bit bases)
    for n_seg in (1, 2, 3):
        assert ops.dxdw_supported(_t(LIMIT + 13, 128), _t(LIMIT + 13, 128 * n_seg), n_seg) is True
