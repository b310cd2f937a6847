"""side_kernels_ref.py on the CPU: every restatement agrees with what the project already has for the same operation, the planted
inputs land where they claim, and -- since a wrong kernel cannot be run on purpose -- every check of test_gpu_side_kernels.py
accepts the restatement and rejects the restatement with one geometry mistake built in (the elements of the second grid trip
left out, a row's last chunk or its columns from 2048 on left out, the pad columns counted, rows >= 4096 untouched, add turned
into overwrite, one duplicate of a scatter lost, float64 clip bounds, the positive weight on the negatives, half-up rounding)
at the very inputs the GPU test uses."""
import numpy as np
import pytest
import torch

import side_kernels_ref as sk
from oracle import numpy_ref as nr
from oracle import torch_ref as tr

F32, BF16 = sk.F32, sk.BF16
DTYPES = pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])


def rejected(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def samples(K):
    return sk.log_uniform_ids_host(77 + K, K, sk.SAMPLED_RANGE)


# ------------------------------------------------------------------------------------------ agreement with what exists
def test_sigmoid_restatements_are_autograd_of_torch_sigmoid():
    x = (torch.randn(500, generator=sk.gen(1)) * 6.0).double().requires_grad_(True)
    y = torch.sigmoid(x)
    dy = torch.randn(500, generator=sk.gen(2)).double()
    y.backward(dy)
    assert float((sk.sigmoid_fwd_ref({'x': x.detach()}) - y.detach()).abs().max()) < 1e-15
    assert float((sk.sigmoid_bwd_ref({'y': y.detach(), 'dy': dy}) - x.grad).abs().max()) < 1e-15


def test_softmax_backward_restatement_is_autograd_of_torch_softmax():
    logits = torch.randn(6, 45, generator=sk.gen(3)).double().requires_grad_(True)
    p = torch.softmax(logits, dim=1)
    g = torch.randn(6, 45, generator=sk.gen(4)).double()
    p.backward(g)
    assert float((sk.softmax_bwd_ref({'p': p.detach(), 'g': g}) - logits.grad).abs().max()) < 1e-14


@pytest.mark.parametrize('variant', [sk.CE_TF, sk.CE_PLAIN])
def test_sparse_ce_backward_restatement_is_autograd_of_the_loss(variant):
    c = sk.sparse_bwd_case(40, 13, 0, F32)
    ref, _, pad, bad = sk.sparse_bwd_ref(c, variant)
    p = c['p'].double().requires_grad_(True)
    good = ~pad & ~bad
    y = c['labels'].long().clamp(0, c['V'] - 1)
    if variant == sk.CE_TF:
        pc = p.clamp(sk.F32_EPS, sk.F32_HI)
        loss = torch.log(pc.sum(dim=1)) - torch.log(pc.gather(1, y[:, None])[:, 0])
    else:
        loss = -torch.log(p.gather(1, y[:, None])[:, 0])
    (loss[good].sum() * c['gs']).backward()
    assert bool(good.any() and pad.any() and bad.any())
    rel = (ref[good] - p.grad[good]).abs() / p.grad[good].abs().clamp(min=1.0)
    assert float(rel.max()) < 1e-12
    assert bool((ref[pad] == 0).all() and torch.isnan(ref[bad]).all())


@pytest.mark.parametrize('pos_weight', sk.BCE_POS_WEIGHT)
def test_masked_bce_restatement_is_the_oracles_masked_loss(pos_weight):
    c = sk.bce_case(257, F32)
    item, d = sk.bce_ref(c, pos_weight)
    # the oracle holds eps and 1 - eps in float64, the kernel in fp32: they are the same function strictly inside the clip range
    inside = (c['p'].double() > 1.1e-7) & (c['p'].double() < 1 - 1.3e-7)
    assert bool((~inside).any() and (inside & (c['labels'] == -1.0)).any())
    labels = c['labels'].double()[inside]
    item, d = item[inside], d[inside]
    p = c['p'].double()[inside].requires_grad_(True)
    want = tr.masked_loss(labels, p, tr.binary_ce_tf, pos_weight if pos_weight > 0 else None)
    want.backward()
    n_valid = float((labels != -1.0).sum())
    norm = (pos_weight + 1.0) / 2 if pos_weight > 0 else 1.0
    assert abs(float(item.sum()) / n_valid / norm - float(want.detach())) < 1e-7 * float(want.detach())
    assert float(((d / n_valid / norm - p.grad).abs() / p.grad.abs().clamp(min=1.0)).max()) < 1e-6
    assert bool((sk.bce_ref(c, pos_weight)[1][sk.bce_outside_clip(c)] == 0).all())


@DTYPES
def test_binary_counts_restatement_is_the_oracles_binary_metrics(dtype):
    c = sk.counts_case(257, dtype)
    k = sk.counts_ref(c).double()
    m = nr.binary_metrics(c['y_true'].numpy(), c['y_pred'].float().numpy())
    assert abs(float(k[0] / k[1]) - m['positive_rate']) < 1e-12 and abs(float(k[2] / k[1]) - m['pred_positives']) < 1e-12
    assert abs(float(2 * k[3] / (k[4] + k[5])) - m['f1']) < 1e-12


def test_sampled_ce_restatement_is_logsumexp_with_the_oracles_logq_and_its_autograd():
    K = 24
    c = sk.sampled_case(40, K, 0, F32, 0.37, samples(K))
    loss, dZ, dtrue, ign = sk.sampled_ref(c)
    lab = c['labels'].long()
    Z = c['Z'].double().requires_grad_(True)
    zt_in = c['ztrue'].double().requires_grad_(True)
    zt = zt_in - torch.from_numpy(nr.log_uniform_logq(lab.clamp(0, sk.SAMPLED_RANGE - 1).numpy(), sk.SAMPLED_RANGE, K))
    zn = torch.where(sk.sampled_hits(c), torch.full_like(Z, -float('inf')), Z)
    want = torch.logsumexp(torch.cat([zt[:, None], zn], dim=1), dim=1) - zt
    (want[~ign].sum() * c['gs']).backward()
    assert bool(ign.any() and (~ign).any())
    assert float((loss - want.detach())[~ign].abs().max()) < 1e-12 and bool((loss[ign] == 0).all())
    assert float((dZ - Z.grad).abs().max()) < 1e-14 and float((dtrue - zt_in.grad).abs().max()) < 1e-14


def test_dropout_restatement_follows_keep_mask():
    from bert4clickpath_amd import ops
    c = sk.dropout_case(2056, F32, 0.1, 4242)
    y = sk.dropout_ref(c)
    keep = torch.from_numpy(ops.keep_mask(4242, 2056, 0.1))
    assert torch.equal(y != 0, keep & (c['x'] != 0)) and abs(float(keep.float().mean()) - 0.9) < 0.03
    assert torch.equal(y[keep], c['x'][keep] * float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))))


def test_host_sampler_is_log_uniform():
    ids = sk.log_uniform_ids_host(5, 8192, sk.SAMPLED_RANGE)
    assert int(ids.min()) >= 0 and int(ids.max()) < sk.SAMPLED_RANGE
    assert abs(float((ids < int(sk.SAMPLED_RANGE ** 0.5)).float().mean()) - 0.5) < 0.03      # half of the mass below sqrt(range_max)


# ------------------------------------------------------------------------------------------------ the plants land
@DTYPES
@pytest.mark.parametrize('n', sk.BCE_N)
def test_masked_bce_inputs_leave_the_clip_range_under_both_labels(n, dtype):
    c = sk.bce_case(n, dtype)
    out = sk.bce_outside_clip(c)
    assert int(out.sum()) > 0
    if n >= 12:
        assert bool((out & (c['labels'] == 1.0)).any() and (out & (c['labels'] == 0.0)).any())
    if n >= 257:
        assert bool((c['labels'] == -1.0).any()) and 0.2 < float((c['labels'] == -1.0).float().mean()) < 0.4
    pads = sk.bce_case(n, dtype, all_pad=True)
    assert bool((pads['labels'] == -1.0).all())


@DTYPES
@pytest.mark.parametrize('n', sk.BCE_N)
def test_binary_counts_inputs_hold_ties_and_pads_on_predicted_positives(n, dtype):
    c = sk.counts_case(n, dtype)
    yp, yt = c['y_pred'].double(), c['y_true']
    assert bool(((yp == 0.5) & (yt != -1.0)).any())
    if n >= 255:
        assert bool(((yp == 1.5) & (yt != -1.0)).any() and (yp == 2.5).any())
        assert bool(((torch.round(yp) == 1.0) & (yt == -1.0)).any())


@pytest.mark.parametrize('R,K', sk.ROW_SHAPES)
def test_sampled_ce_labels_hit_the_columns_they_claim(R, K):
    for extra in sk.ROW_PITCH_EXTRA:
        c = sk.sampled_case(R, K, extra, F32, 1.0, samples(K))
        hits = sk.sampled_hits(c)
        assert int(hits.sum()) > 0 and bool(hits[0, K - 1])
        if K > 2047:
            assert bool(hits[1, 2047])
        lab = c['labels']
        assert bool((lab == -1).any() or (lab >= sk.SAMPLED_RANGE).any())
        if R > 8:
            assert bool((lab == -1).any() and (lab >= sk.SAMPLED_RANGE).any() and hits[R - 1].any())
    c = sk.sampled_case(R, K, 0, F32, 1.0, samples(K), all_hits=True)
    assert bool(sk.sampled_hits(c)[0].all())
    loss, dZ, dtrue, _ = sk.sampled_ref(c)
    assert float(loss[0]) == 0.0 and float(dtrue[0]) == 0.0 and bool((dZ[0] == 0).all())


@pytest.mark.parametrize('R,V', sk.ROW_SHAPES)
def test_sparse_ce_inputs_hold_every_kind_of_row(R, V):
    kinds = set()
    for extra in sk.ROW_PITCH_EXTRA:
        c = sk.sparse_bwd_case(R, V, extra, F32)
        _, _, pad, bad = sk.sparse_bwd_ref(c, sk.CE_TF)
        lab, p = c['labels'], c['p'].double()
        kinds |= {'pad'} if bool(pad.any()) else set()
        kinds |= {'bad'} if bool(bad.any()) else set()
        assert bool((lab == 0).any() and (lab == V - 1).any())
        assert bool((p < sk.F32_EPS).any()) or V < 3
        assert bool((p > sk.F32_HI).any())
        good = ~pad & ~bad
        assert bool((p[good].gather(1, lab[good].long()[:, None]) > 0).all())
    assert kinds == {'pad', 'bad'}


# ------------------------------------------------------------------------------------------------------------ teeth
@DTYPES
def test_vec8_checks_reject_a_lost_second_trip(dtype):
    n = sk.VEC8_N[-1]
    assert n > sk.VEC8_TRIP
    d = sk.dropout_case(n, dtype, 0.1, 11)
    r = sk.relu_gate_case(n, dtype)
    for ref, what in ((sk.dropout_ref(d), 'dropout'), (sk.relu_gate_ref(r), 'relu_gate')):
        sk.exact_check(ref, sk.elemwise_emulate(ref), what)
        rejected(sk.exact_check, ref, sk.elemwise_emulate(ref, 'second_trip'), what)
    f = sk.sigmoid_fwd_case(n, dtype)
    b = sk.sigmoid_bwd_case(n, dtype)
    for ref, bound in ((sk.sigmoid_fwd_ref(f), sk.sigmoid_fwd_bound), (sk.sigmoid_bwd_ref(b), sk.sigmoid_bwd_bound)):
        assert sk.bounded_check(ref, bound(ref, dtype), sk.elemwise_emulate(ref.to(dtype)), 'sigmoid') <= 1.0
        rejected(sk.bounded_check, ref, bound(ref, dtype), sk.elemwise_emulate(ref.to(dtype), 'second_trip'), 'sigmoid')


@DTYPES
@pytest.mark.parametrize('n', sk.VEC8_N[:-1])
def test_vec8_restatements_pass_their_own_checks_at_every_size(n, dtype):
    for ref, bound in ((sk.sigmoid_fwd_ref(sk.sigmoid_fwd_case(n, dtype)), sk.sigmoid_fwd_bound),
                       (sk.sigmoid_bwd_ref(sk.sigmoid_bwd_case(n, dtype)), sk.sigmoid_bwd_bound)):
        sk.bounded_check(ref, bound(ref, dtype), sk.elemwise_emulate(ref.to(dtype)), 'sigmoid')
        wrong = sk.elemwise_emulate(ref.to(dtype))
        wrong[n - 1] = wrong[n - 1] * 1.02 + 0.01                # an element two percent off is no rounding
        rejected(sk.bounded_check, ref, bound(ref, dtype), wrong, 'sigmoid')


@DTYPES
@pytest.mark.parametrize('n', sk.BCE_N)
def test_masked_bce_check_rejects_every_wrong_variant(n, dtype):
    c = sk.bce_case(n, dtype)
    for pw in sk.BCE_POS_WEIGHT:
        assert sk.bce_check(c, pw, *sk.bce_emulate(c, pw)) < 0.2
        item, d, sums = sk.bce_emulate(c, pw)
        sk.bce_check(c, pw, None, None, sums, item_for_sum=item)
        rejected(sk.bce_check, c, pw, *sk.bce_emulate(c, pw, 'overwrite'))
        if n >= 12:                                              # (a single element carries one of the plants only)
            rejected(sk.bce_check, c, pw, *sk.bce_emulate(c, pw, 'f64_clip'))
        if pw > 0 and n >= 12:
            rejected(sk.bce_check, c, pw, *sk.bce_emulate(c, pw, 'weight_on_negatives'))
        if n > sk.BCE_THREADS:
            rejected(sk.bce_check, c, pw, *sk.bce_emulate(c, pw, 'second_trip'))
            lost = sk.bce_emulate(c, pw, 'second_trip')[2]       # the sums alone, as the call without the optional outputs is checked
            rejected(sk.bce_check, c, pw, None, None, lost, item)
    pads = sk.bce_case(n, dtype, all_pad=True)
    sk.bce_check(pads, 3.0, *sk.bce_emulate(pads, 3.0))
    assert float(sk.bce_emulate(pads, 3.0)[2][1]) == sk.BCE_SUMS_START[1]


@DTYPES
@pytest.mark.parametrize('n', sk.BCE_N)
def test_binary_counts_check_rejects_every_wrong_variant(n, dtype):
    c = sk.counts_case(n, dtype)
    sk.counts_check(c, sk.counts_emulate(c))
    rejected(sk.counts_check, c, sk.counts_emulate(c, 'overwrite'))
    rejected(sk.counts_check, c, sk.counts_emulate(c, 'half_up'))
    if n > sk.BCE_THREADS:
        rejected(sk.counts_check, c, sk.counts_emulate(c, 'second_trip'))


def wrong_variants_of(R, V):
    yield 'last_chunk'
    if V > sk.ROW_TRIP:
        yield 'from_2048'
    if V % 8:
        yield 'tail_counts'
    if R > sk.ROW_CAP:
        yield 'rows_4096'


def test_row_shapes_cover_every_wrong_variant():
    seen = set()
    for R, V in sk.ROW_SHAPES:
        seen |= set(wrong_variants_of(R, V))
    assert seen == set(sk.WRONG_ROWS)


@DTYPES
@pytest.mark.parametrize('R,V', sk.ROW_SHAPES)
def test_softmax_backward_check_rejects_every_wrong_variant(R, V, dtype):
    for extra in sk.ROW_PITCH_EXTRA:
        c = sk.softmax_bwd_case(R, V, extra, dtype)
        sk.softmax_bwd_check(c, sk.softmax_bwd_emulate(c))
        for wrong in wrong_variants_of(R, V):
            rejected(sk.softmax_bwd_check, c, sk.softmax_bwd_emulate(c, wrong))


@DTYPES
@pytest.mark.parametrize('R,V', sk.ROW_SHAPES)
def test_sparse_ce_backward_check_rejects_every_wrong_variant(R, V, dtype):
    for extra in sk.ROW_PITCH_EXTRA:
        c = sk.sparse_bwd_case(R, V, extra, dtype)
        for variant in (sk.CE_TF, sk.CE_PLAIN):
            sk.sparse_bwd_check(c, variant, sk.sparse_bwd_emulate(c, variant))
            for wrong in wrong_variants_of(R, V):
                if variant == sk.CE_PLAIN and wrong == 'tail_counts':
                    continue                                     # (the plain variant has no row sum for the pad columns to enter)
                rejected(sk.sparse_bwd_check, c, variant, sk.sparse_bwd_emulate(c, variant, wrong))


@DTYPES
@pytest.mark.parametrize('R,K', sk.ROW_SHAPES)
def test_sampled_ce_check_rejects_every_wrong_variant(R, K, dtype):
    for extra, gs in zip(sk.ROW_PITCH_EXTRA, sk.SAMPLED_GS):
        for all_hits in (False, True):
            c = sk.sampled_case(R, K, extra, dtype, gs, samples(K), all_hits)
            assert sk.sampled_check(c, *sk.sampled_emulate(c)) <= 1.0
            for wrong in wrong_variants_of(R, K):
                if all_hits and wrong in ('last_chunk', 'from_2048') and R <= 3:
                    continue                                     # (three rows of which the first has no negatives left: see the drawn case)
                rejected(sk.sampled_check, c, *sk.sampled_emulate(c, wrong))


@DTYPES
@pytest.mark.parametrize('width', sk.ROW_DOT_WIDTH)
def test_row_dot_check_rejects_every_wrong_variant(width, dtype):
    for R in sk.ROW_DOT_R:
        for integers in (True, False):
            c = sk.row_dot_case(R, width, dtype, integers, True)
            sk.row_dot_check(c, sk.row_dot_emulate(c))
            if R >= 3:                                           # (one row alone may lose eight products that happen to cancel)
                rejected(sk.row_dot_check, c, sk.row_dot_emulate(c, 'last_chunk'))
                if width > sk.ROW_DOT_LANE_TRIP:
                    rejected(sk.row_dot_check, c, sk.row_dot_emulate(c, 'lane_trip'))
            if R > sk.ROW_DOT_ROW_TRIP:
                rejected(sk.row_dot_check, c, sk.row_dot_emulate(c, 'second_trip'))


@DTYPES
def test_row_scale_and_rows_add_checks_reject_every_wrong_variant(dtype):
    for R, width in sk.ROWS8_SHAPES:
        big = R * (width // 8) > sk.EW_THREADS
        c = sk.row_scale_case(R, width, dtype)
        sk.row_scale_check(c, sk.row_scale_emulate(c))
        if big:
            rejected(sk.row_scale_check, c, sk.row_scale_emulate(c, 'second_trip'))
        for dst_dtype, src_dtype in sk.ROWS_ADD_DTYPES:
            if dst_dtype != dtype:
                continue
            c = sk.rows_add_case(R, width, dst_dtype, src_dtype)
            sk.rows_add_check(c, sk.rows_add_emulate(c))
            if R > 1:                                            # (the single source row of the smallest shape may be a skipped one)
                rejected(sk.rows_add_check, c, sk.rows_add_emulate(c, 'overwrite'))
            if big:
                rejected(sk.rows_add_check, c, sk.rows_add_emulate(c, 'second_trip'))
    assert any(R * (width // 8) > sk.EW_THREADS for R, width in sk.ROWS8_SHAPES)


def test_gather_and_scatter_checks_reject_every_wrong_variant():
    for n, width in sk.ROWS4_SHAPES:
        big = n * (width // 4) > sk.EW_THREADS
        c = sk.rows_gather_case(n, width)
        sk.rows_gather_check(c, sk.rows_gather_emulate(c))
        c = sk.rows_scatter_case(n, width)
        sk.rows_scatter_check(c, sk.rows_scatter_emulate(c))
        rejected(sk.rows_scatter_check, c, sk.rows_scatter_emulate(c, 'overwrite'))
        rejected(sk.rows_scatter_check, c, sk.rows_scatter_emulate(c, 'lost_duplicate'))
        if n >= sk.HOT_SOURCES:
            assert int((c['idx'] == 3).sum()) >= sk.HOT_SOURCES
        if big:
            rejected(sk.rows_scatter_check, c, sk.rows_scatter_emulate(c, 'second_trip'))
            g = sk.rows_gather_case(n, width)
            rejected(sk.rows_gather_check, g, sk.rows_gather_emulate(g, 'second_trip'))
    assert any(n * (width // 4) > sk.EW_THREADS for n, width in sk.ROWS4_SHAPES)
    for n in sk.FLAT_N:
        c = sk.scatter_1d_case(n)
        sk.scatter_1d_check(c, sk.scatter_1d_emulate(c))
        g = sk.gather_i64_case(n)
        sk.gather_i64_check(g, sk.gather_i64_emulate(g))
        assert int(g['src'].abs().max()) > 2 ** 32
        if n > 8:
            rejected(sk.scatter_1d_check, c, sk.scatter_1d_emulate(c, 'overwrite'))
            rejected(sk.scatter_1d_check, c, sk.scatter_1d_emulate(c, 'lost_duplicate'))
        if n > sk.EW_THREADS:
            rejected(sk.scatter_1d_check, c, sk.scatter_1d_emulate(c, 'second_trip'))
            rejected(sk.gather_i64_check, g, sk.gather_i64_emulate(g, 'second_trip'))
    assert sk.FLAT_N[-1] > sk.EW_THREADS


def test_transpose_add_and_poison_checks_reject_every_wrong_variant():
    for K, N in sk.TRANSPOSE_SHAPES:
        for es, ed in ((0, 0), (8, 0), (0, 8), (8, 8)):
            c = sk.transpose_add_case(K, N, es, ed)
            sk.transpose_add_check(c, sk.transpose_add_emulate(c))
            if K * N > 1:
                rejected(sk.transpose_add_check, c, sk.transpose_add_emulate(c, 'overwrite'))
    for rows, width in sk.POISON_SHAPES:
        for extra in (0, 3):
            for dtype in sk.POISON_DTYPES:
                c = sk.poison_case(rows, width, extra, dtype)
                for flag in (-1, 0, 5):
                    sk.poison_check(c, flag, sk.poison_emulate(c, flag))
                rejected(sk.poison_check, c, -1, sk.poison_emulate(c, 0))
                rejected(sk.poison_check, c, 0, sk.poison_emulate(c, -1))
                if rows * width > sk.EW_THREADS:
                    rejected(sk.poison_check, c, -1, sk.poison_emulate(c, -1, 'second_trip'))
    assert any(rows * width > sk.EW_THREADS for rows, width in sk.POISON_SHAPES)


def test_bookkeeping_checks_reject_a_lost_scalar_tail():
    for R in sk.BOOKKEEPING_R:
        for off in (0, 1):
            c = sk.label_scale_case(R)
            sk.label_scale_check(c, off, sk.elemwise_emulate(sk.label_scale_ref(c, off)))
            s = sk.sum_scaled_case(R)
            sk.sum_scaled_check(s, off, sk.sum_scaled_ref(s, off), sk.sum_scaled_ref(s, off), float('nan'))
            rejected(sk.sum_scaled_check, s, off, sk.sum_scaled_ref(s, off), sk.sum_scaled_ref(s, off), sk.sum_scaled_ref(s, off))
            if R in (1023, 4099):
                rejected(sk.label_scale_check, c, off, sk.elemwise_emulate(sk.label_scale_ref(c, off, 'scalar_tail')))
                rejected(sk.sum_scaled_check, s, off, sk.sum_scaled_ref(s, off, 'scalar_tail'), sk.sum_scaled_ref(s, off), float('nan'))
