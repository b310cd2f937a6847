"""The small row and elementwise kernels of csrc/elemwise.hip through their raw entry points, element by element against the float64
/ integer restatements of side_kernels_ref.py, on the smallest shapes that cross each threshold of their geometry:

  dropout, sigmoid_fwd / _bwd, relu_gate     8 elements per thread, 2048 x 256 threads: second trip from element 8 * 524,288
  masked_bce, binary_counts                  their own 512-workgroup cap: second trip from element 131,072; float atomics
  softmax_rows_bwd, sparse_ce_from_probs_bwd,
  sampled_ce_fwd_bwd                         4096 workgroups (row 4096 is a second row), 2048 columns per 256-thread trip,
                                             the j < V tail of the last 8-column chunk, pitches rup8(V) and rup8(V) + 8
  row_dot                                    4 rows per workgroup x 2048 (row 8192), 512 columns per lane trip
  row_scale_f32, rows_add                    R * width / 8 work items past 524,288; pitched rows; skipped (-1) rows
  rows_gather_f32, rows_scatter_add_f32      n * width / 4 work items past 524,288; a row that 1,000 sources reach
  scatter_add_1d, gather_i64                 n past 524,288; values past 2^32
  transpose_add                              32 x 32 tiles with ragged edges in both directions
  poison_rows                                rows * width past 524,288, ld > width, three element types
  label_scale, sum_scaled                    the 16-byte body and the scalar tail, and the scalar branch of an unaligned pointer

Outputs are sentinel-filled and 64 elements longer than needed (row outputs: 8 gap columns per row); accumulators start from
non-zero integers.  What each check accepts and rejects is shown on the CPU in test_side_kernels_cpu.py.

Two bounds rest on the accuracy of the device's expf / logf.  Worst err / bound observed on the MI355X (printed by the tests):
  masked BCE, 1e-6 + 1e-6 |ref|:             probabilities in fp32 0.219, in bf16 0.187
  sampled-softmax Z / dtrue, 2e-5 gs:        fp32 0.017
  the same beside one bf16 ulp (bf16 rows):  0.968 -- above 0.5, and all of it the rounding to bf16: the float64 restatement
                                             rounded once to bf16 sits at the same 0.968 (half an ulp of a value just above a
                                             power of two is nearly 2^-8 of it); the fp32 work in front of the rounding is the
                                             0.017 of the fp32 rows"""
import pytest
import torch

import side_kernels_ref as sk

pytestmark = pytest.mark.gpu

F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
DTYPES = pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])


def _lib():
    from bert4clickpath_amd import _lib as LB
    return LB


def _rc(name, *args):
    LB = _lib()
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    return getattr(LB.lib(), name)(*conv, torch.cuda.current_stream().cuda_stream)


def _call(name, *args):
    assert _rc(name, *args) == 0, _lib().lib().b4c_last_error().decode()


def _dt(dtype):
    LB = _lib()
    return LB._C['B4C_I32'] if dtype == I32 else (LB.F32 if dtype == F32 else LB.BF16)      # (int32: poison_rows only)


def _refused(name, *args):
    """the entry point returns an error and launches nothing"""
    assert _rc(name, *args) != 0, name + ' accepted a call it must refuse'
    assert _lib().lib().b4c_last_error().decode()


def _sent(n, dtype):
    return sk.flat_buffer(n, dtype).cuda()


# ------------------------------------------------------------------------------------------ 1. eight elements per thread
@DTYPES
@pytest.mark.parametrize('n', sk.VEC8_N)
def test_dropout_is_the_keep_mask_times_the_fp32_factor(n, dtype):
    for rate, seed in ((0.1, 4242), (0.5, 4242), (0.1, (1 << 40) + 5), (0.5, (1 << 40) + 5)):
        c = sk.dropout_case(n, dtype, rate, seed)
        y = _sent(n, dtype)
        _call('b4c_dropout', c['x'].cuda(), y, n, rate, seed, _dt(dtype))
        sk.exact_check(sk.dropout_ref(c), y.cpu(), 'dropout n=%d rate=%g seed=%d %s' % (n, rate, seed, dtype))


@DTYPES
@pytest.mark.parametrize('n', sk.VEC8_N)
def test_relu_gate_is_where(n, dtype):
    c = sk.relu_gate_case(n, dtype)
    out = _sent(n, dtype)
    _call('b4c_relu_gate', c['g'].cuda(), c['act'].cuda(), out, n, _dt(dtype))
    sk.exact_check(sk.relu_gate_ref(c), out.cpu(), 'relu_gate n=%d %s' % (n, dtype))


@DTYPES
@pytest.mark.parametrize('n', sk.VEC8_N)
def test_sigmoid_forward_and_backward(n, dtype):
    c = sk.sigmoid_fwd_case(n, dtype)
    y = _sent(n, dtype)
    _call('b4c_sigmoid_fwd', c['x'].cuda(), y, n, _dt(dtype))
    ref = sk.sigmoid_fwd_ref(c)
    sk.bounded_check(ref, sk.sigmoid_fwd_bound(ref, dtype), y.cpu(), 'sigmoid_fwd n=%d %s' % (n, dtype))
    c = sk.sigmoid_bwd_case(n, dtype)
    dx = _sent(n, dtype)
    _call('b4c_sigmoid_bwd', c['y'].cuda(), c['dy'].cuda(), dx, n, _dt(dtype))
    ref = sk.sigmoid_bwd_ref(c)
    sk.bounded_check(ref, sk.sigmoid_bwd_bound(ref, dtype), dx.cpu(), 'sigmoid_bwd n=%d %s' % (n, dtype))


@DTYPES
def test_vec8_kernels_refuse_what_they_cannot_do(dtype):
    x, y = torch.ones(16, dtype=dtype, device='cuda'), _sent(16, dtype)
    _refused('b4c_dropout', x, y, 12, 0.1, 1, _dt(dtype))
    _refused('b4c_dropout', x, y, 16, 0.0, 1, _dt(dtype))
    _refused('b4c_dropout', x, y, 16, 1.0, 1, _dt(dtype))
    _refused('b4c_sigmoid_fwd', x, y, 12, _dt(dtype))
    _refused('b4c_sigmoid_bwd', x, x, y, 12, _dt(dtype))
    _refused('b4c_relu_gate', x, x, y, 12, _dt(dtype))
    torch.cuda.synchronize()
    assert bool((y == sk.SENT).all())


# ----------------------------------------------------------------------------- 2. masked binary CE and the binary counts
_worst = {}


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print('worst err / bound so far, %s: %.3f' % (key, _worst[key]))


@DTYPES
@pytest.mark.parametrize('n', sk.BCE_N)
def test_masked_bce_items_gradients_count_and_sum(n, dtype):
    for c in (sk.bce_case(n, dtype), sk.bce_case(n, dtype, all_pad=True)):
        p, lab = c['p'].cuda(), c['labels'].cuda()
        for pw in sk.BCE_POS_WEIGHT:
            item, d = _sent(n, F32), _sent(n, F32)
            sums = torch.tensor(sk.BCE_SUMS_START, device='cuda')
            _call('b4c_masked_bce', p, lab, pw, item, sums, d, n, _dt(dtype))
            _note('masked_bce %s' % dtype, sk.bce_check(c, pw, item.cpu(), d.cpu(), sums.cpu()))
            # without the optional outputs (null pointers), and with one of them
            sums2 = torch.tensor(sk.BCE_SUMS_START, device='cuda')
            _call('b4c_masked_bce', p, lab, pw, None, sums2, None, n, _dt(dtype))
            sk.bce_check(c, pw, None, None, sums2.cpu(), item_for_sum=item.cpu())
            d3 = _sent(n, F32)
            sums3 = torch.tensor(sk.BCE_SUMS_START, device='cuda')
            _call('b4c_masked_bce', p, lab, pw, None, sums3, d3, n, _dt(dtype))
            sk.bce_check(c, pw, None, d3.cpu(), sums3.cpu(), item_for_sum=item.cpu())


@DTYPES
@pytest.mark.parametrize('n', sk.BCE_N)
def test_binary_counts_are_the_integer_counts_and_accumulate(n, dtype):
    c = sk.counts_case(n, dtype)
    out = torch.tensor(sk.COUNTS_START, device='cuda')
    for _ in range(2):
        _call('b4c_binary_counts', c['y_true'].cuda(), c['y_pred'].cuda(), out, n, _dt(dtype))
    sk.counts_check(c, out.cpu())


# ------------------------------------------------------------------------------------------------ 3. a workgroup per row
@DTYPES
@pytest.mark.parametrize('R,V', sk.ROW_SHAPES)
def test_softmax_rows_backward(R, V, dtype):
    for extra in sk.ROW_PITCH_EXTRA:
        c = sk.softmax_bwd_case(R, V, extra, dtype)
        dx, _ = sk.row_buffer(R, c['ld'], dtype)
        dx = dx.cuda()
        _call('b4c_softmax_rows_bwd', c['p_buf'].cuda(), c['ld'], c['g_buf'].cuda(), sk.rup8(V) + 8 - extra, dx, c['ld'], R, V, _dt(dtype))
        sk.softmax_bwd_check(c, dx.cpu())


@DTYPES
@pytest.mark.parametrize('R,V', sk.ROW_SHAPES)
def test_sparse_ce_from_probs_backward_both_variants(R, V, dtype):
    LB = _lib()
    assert (LB.CE_TF, LB.CE_PLAIN) == (sk.CE_TF, sk.CE_PLAIN)
    for extra in sk.ROW_PITCH_EXTRA:
        c = sk.sparse_bwd_case(R, V, extra, dtype)
        p, lab = c['p_buf'].cuda(), c['labels'].cuda()
        gs = torch.tensor([sk.SPARSE_GS], device='cuda')
        for variant in (sk.CE_TF, sk.CE_PLAIN):
            dp, _ = sk.row_buffer(R, c['ld'], dtype)
            dp = dp.cuda()
            _call('b4c_sparse_ce_from_probs_bwd', p, sk.rup8(V) + 8 - extra, lab, gs, dp, c['ld'], R, V, variant, _dt(dtype))
            sk.sparse_bwd_check(c, variant, dp.cpu())


@DTYPES
@pytest.mark.parametrize('R,K', sk.ROW_SHAPES)
def test_sampled_ce_forward_and_backward(R, K, dtype):
    from bert4clickpath_amd import ops
    drawn = ops.log_uniform_sample(77 + K, K, sk.SAMPLED_RANGE, 'cuda')[0].cpu()
    assert torch.equal(drawn, sk.log_uniform_ids_host(77 + K, K, sk.SAMPLED_RANGE))      # the draw the CPU tests show their teeth on
    for extra, gs in zip(sk.ROW_PITCH_EXTRA, sk.SAMPLED_GS):
        for all_hits in (False, True):
            c = sk.sampled_case(R, K, extra, dtype, gs, drawn, all_hits)
            Z, item, dtrue = c['Z_buf'].cuda(), _sent(R, F32), _sent(R, F32)
            _call('b4c_sampled_ce_fwd_bwd', Z, c['ld'], c['ztrue'].cuda(), c['samples'].cuda(), c['labels'].cuda(), sk.SAMPLED_RANGE,
                  item, dtrue, torch.tensor([gs], device='cuda'), R, K, _dt(dtype))
            _note('sampled_ce %s' % dtype, sk.sampled_check(c, Z.cpu(), item.cpu(), dtrue.cpu()))
            if dtype == BF16:                # how much of that is the rounding to bf16 itself: the float64 restatement, rounded once
                _note('sampled_ce, the float64 restatement rounded to bf16', sk.sampled_check(c, *sk.sampled_emulate(c)))


# ----------------------------------------------------------------------------------- 4. a wave per row, a vector per element
@DTYPES
@pytest.mark.parametrize('width', sk.ROW_DOT_WIDTH)
def test_row_dot(width, dtype):
    for R in sk.ROW_DOT_R:
        for integers in (True, False):
            for pitch_a in (True, False):
                c = sk.row_dot_case(R, width, dtype, integers, pitch_a)
                out = _sent(R, F32)
                _call('b4c_row_dot', c['a_buf'].cuda(), c['lda'], c['b_buf'].cuda(), c['ldb'], out, R, width, _dt(dtype))
                sk.row_dot_check(c, out.cpu())


@DTYPES
@pytest.mark.parametrize('R,width', sk.ROWS8_SHAPES)
def test_row_scale_f32(R, width, dtype):
    c = sk.row_scale_case(R, width, dtype)
    out, _ = sk.row_buffer(R, c['ld_out'], F32)
    out = out.cuda()
    _call('b4c_row_scale_f32', c['src_buf'].cuda(), c['ld'], c['scale'].cuda(), out, c['ld_out'], R, width, _dt(dtype))
    sk.row_scale_check(c, out.cpu())


@pytest.mark.parametrize('dtype,src_dtype', sk.ROWS_ADD_DTYPES, ids=['fp32', 'bf16', 'bf16 from fp32'])
@pytest.mark.parametrize('R,width', sk.ROWS8_SHAPES)
def test_rows_add_is_index_add(R, width, dtype, src_dtype):
    c = sk.rows_add_case(R, width, dtype, src_dtype)
    dst = c['dst_buf'].cuda()
    _call('b4c_rows_add', dst, c['ld_dst'], c['idx'].cuda(), c['src_buf'].cuda(), c['ld_src'], R, width, _dt(dtype), _dt(src_dtype))
    sk.rows_add_check(c, dst.cpu())


@pytest.mark.parametrize('n,width', sk.ROWS4_SHAPES)
def test_rows_gather_and_scatter_add_f32(n, width):
    c = sk.rows_gather_case(n, width)
    out, _ = sk.row_buffer(n, c['ld_out'], F32)
    out = out.cuda()
    _call('b4c_rows_gather_f32', c['table_buf'].cuda(), c['ld_src'], c['idx'].cuda(), out, c['ld_out'], n, width)
    sk.rows_gather_check(c, out.cpu())
    c = sk.rows_scatter_case(n, width)
    dst = c['dst_buf'].cuda()
    _call('b4c_rows_scatter_add_f32', c['src_buf'].cuda(), c['ld_src'], c['idx'].cuda(), dst, c['ld_dst'], n, width)
    sk.rows_scatter_check(c, dst.cpu())


@pytest.mark.parametrize('n', sk.FLAT_N)
def test_scatter_add_1d_and_gather_i64(n):
    c = sk.scatter_1d_case(n)
    dst = sk.elemwise_emulate(c['dst']).cuda()
    _call('b4c_scatter_add_1d', c['src'].cuda(), c['idx'].cuda(), dst, n)
    sk.scatter_1d_check(c, dst.cpu())
    c = sk.gather_i64_case(n)
    out = _sent(n, torch.int64)
    _call('b4c_gather_i64', c['src'].cuda(), c['idx'].cuda(), out, n)
    sk.gather_i64_check(c, out.cpu())


@pytest.mark.parametrize('K,N', sk.TRANSPOSE_SHAPES)
def test_transpose_add(K, N):
    for extra_src, extra_dst in ((0, 0), (8, 0), (0, 8), (8, 8)):
        c = sk.transpose_add_case(K, N, extra_src, extra_dst)
        dst = c['dst_buf'].cuda()
        _call('b4c_transpose_add', c['src_buf'].cuda(), c['ld_src'], dst, c['ld_dst'], K, N)
        sk.transpose_add_check(c, dst.cpu())


@pytest.mark.parametrize('dtype', sk.POISON_DTYPES, ids=['fp32', 'bf16', 'int32'])
@pytest.mark.parametrize('rows,width', sk.POISON_SHAPES)
def test_poison_rows(rows, width, dtype):
    for extra in (0, 3):
        c = sk.poison_case(rows, width, extra, dtype)
        for flag in (-1, 0, 5):
            x = c['x_buf'].cuda()
            _call('b4c_poison_rows', x, c['ld'], rows, width, torch.tensor([flag], dtype=I32, device='cuda'), _dt(dtype))
            sk.poison_check(c, flag, x.cpu())


@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'one element off'])
@pytest.mark.parametrize('R', sk.BOOKKEEPING_R)
def test_label_scale_and_sum_scaled(R, off):
    c = sk.label_scale_case(R)
    lab = c['buf'].cuda()
    assert lab.data_ptr() % 16 == 0
    out = _sent(2, F32)
    _call('b4c_label_scale', lab.data_ptr() + 4 * off, R, c['V'], out)
    sk.label_scale_check(c, off, out.cpu())
    c = sk.sum_scaled_case(R)
    item = c['buf'].cuda()
    assert item.data_ptr() % 16 == 0
    scale = torch.tensor([c['scale'], 0.0], device='cuda')
    got = []
    for flag in (None, 5, -7):
        out = _sent(1, F32)
        poison = None if flag is None else torch.tensor([flag], dtype=I32, device='cuda')
        _call('b4c_sum_scaled', item.data_ptr() + 4 * off, R, scale, poison, out)
        sk.assert_tail(out.cpu(), 1, 'sum_scaled')
        got.append(float(out[0]))
    sk.sum_scaled_check(c, off, *got)
