"""tests/fused_rows_ref.py without a GPU: the launch geometry against a brute-force ownership table, the conditions of the two input
families, a CPU emulation of each kernel's rounding steps held to every check of tests/test_gpu_fused_rows.py at the shared inputs,
and nine wrong variants of that emulation, each of which has to fail one of those checks."""
import numpy as np
import pytest
import torch

import fused_rows_ref as fr


def _table(M, cap):
    """brute force: tile, workgroup and turn of every row"""
    T = -(-M // fr.TILE)
    G = min(T, cap)
    tile = np.arange(M) // fr.TILE
    return tile, tile % G, tile // G, T, G


@pytest.mark.parametrize('M,cap', [(M, fr.CAP_BWD) for M in fr.BWD_M] + [(M, fr.CAP_FWD) for M in fr.FWD_M])
def test_tile_edges_against_the_ownership_table(M, cap):
    tile, wg, turn, T, G = _table(M, cap)
    rows = np.arange(M)
    want = {0, 31, 32, M - 2, M - 1}
    first_last = lambda sel: {int(rows[sel][0]), int(rows[sel][-1])} if sel.any() else set()      # noqa: E731
    want |= first_last(tile == T - 1)
    sizes = np.bincount(tile, minlength=T)
    full = np.nonzero(sizes == fr.TILE)[0]
    if len(full):
        want |= first_last(tile == full[-1])
    want |= first_last(tile == G - 1)
    for t in (G, 4 * G):
        if (tile == t).any():
            want.add(int(rows[tile == t][0]))
    for w in (0, G - 1):
        mine = wg == w
        want.add(int(rows[mine & (turn == turn[mine].max())][0]))
    want = sorted(r for r in want if 0 <= r < M)
    assert fr.tile_edges(M, cap) == want


def test_the_row_counts_reach_the_cases_they_were_chosen_for():
    for cap, step, big in ((fr.CAP_BWD, 8192, 40929), (fr.CAP_FWD, 16384, 81889)):
        for k in (1, 2, 3, 4):
            tile, wg, turn, T, G = _table(step * k + 1, cap)
            assert G == cap and turn[wg == 0].max() == k and (tile == T - 1).sum() == 1 and wg[-1] == 0
            assert ((tile == 4 * G).any()) == (k == 4)                 # the first re-use of a ring stage
        tile, wg, turn, T, G = _table(big, cap)
        assert (tile == T - 1).sum() == 1 and wg[-1] == cap - 1 and turn[-1] == 4
    for M in (2, 3, 31, 32, 33, 63, 64, 65):
        assert _table(M, fr.CAP_BWD)[4] in (1, 2, 3)                   # grids of one to three workgroups


def test_rows_a_listed_shift_apart_have_unlike_statistics():
    m, s = fr.row_params(40000)
    for d in fr.SHIFTS:
        assert d % 15 != 0
        same = (m[:-d] == m[d:]) & (s[:-d] == s[d:])
        assert not bool(same.any()), d


def _bwd_shapes(kind):
    return fr.shapes('bwd', with_width=kind != 'ao')


BWD_PARAMS = [(kind, M, F, rate) for kind in fr.BWD_KINDS for M, F, rate in _bwd_shapes(kind)]


@pytest.mark.parametrize('kind,M,F,rate', BWD_PARAMS)
def test_impulse_family_condition_and_emulation(kind, M, F, rate):
    """in every one-row launch at least half of the entries of each row sum exceed twice their own bound (a lost row fails), and the
    emulation passes every check: one launch per edge row, one with all of them"""
    c = fr.bwd_case(kind, M, F)
    edges = fr.tile_edges(M, fr.CAP_BWD)
    for r in edges:
        share = fr.share_condition(c, r, rate)
        assert min(share.values()) >= 0.5, (r, share)
        fr.check_bwd(c, [r], rate, fr.emulate_bwd(c, [r], rate), tag='row %d ' % r)
    fr.check_bwd(c, edges, rate, fr.emulate_bwd(c, edges, rate), tag='edges ')


@pytest.mark.parametrize('kind,M,F,rate', [p for p in BWD_PARAMS if p[1] in fr.BWD_UNLIKE_M])
def test_unlike_rows_backward_emulation(kind, M, F, rate):
    c = fr.bwd_case(kind, M, F)
    rows = torch.arange(M)
    fr.check_bwd(c, rows, rate, fr.emulate_bwd(c, rows, rate))


@pytest.mark.parametrize('kind', fr.FWD_KINDS)
@pytest.mark.parametrize('M,F,rate', [s for s in fr.shapes('fwd') if s[0] in fr.FWD_UNLIKE_M or s[1:] == (100, 0.1)])
def test_unlike_rows_forward_emulation(kind, M, F, rate):
    """every row count at F = 100 and rate 0.1; the other widths and rate 0 at the three row counts of the unlike-rows family"""
    c = fr.fwd_case(M, F)
    for act in (('gelu', 'gelu_tanh') if kind == 'act' and F == 100 and rate > 0 else ('gelu',)):
        fr.check_fwd(fr.fwd_ref(c, kind, rate, act), fr.emulate_fwd(c, kind, rate, act))


def test_measured_size_of_the_fp32_activation_terms():
    """the figures of the module docstring: a few 2^-24 |u|"""
    u = torch.linspace(-9, 9, 2000001)
    for act, a_max, g_max in (('gelu', 4.5e-7, 1.4e-7), ('gelu_tanh', 4.5e-7, 5.7e-7)):
        assert float(fr.act_term(act, u).max()) / 2 <= a_max
        assert float(fr.act_grad_term(act, u).max()) / 2 <= g_max


# ---- the wrong variants -------------------------------------------------------------------------------------------------------
def _rejected_bwd(kind, M, F, rate, rows, mutant):
    c = fr.bwd_case(kind, M, F)
    with pytest.raises(AssertionError):
        fr.check_bwd(c, rows, rate, fr.emulate_bwd(c, rows, rate, mutant))


# the launch that has to expose each variant: (M, the row with dOut as a function of M and G, rate, F)
BWD_MUTANT_LAUNCH = {
    'last_row_left_out': (8193, lambda M, G: M - 1, 0.1, 100),
    'tile_G_twice': (8193, lambda M, G: 32 * G, 0.1, 100),
    'odd_last_row_stats': (8193, lambda M, G: M - 1, 0.1, 100),
    'stats_halves_swapped': (8193, lambda M, G: 32, 0.1, 100),
    'keep_shifted': (8193, lambda M, G: 32 * (G - 1), 0.1, 100),
    'past_M_into_dbeta': (8193, lambda M, G: M - 1, 0.1, 100),
    'padded_hidden_columns': (8193, lambda M, G: 31, 0.1, 100),
    'tile_4G_previous_occupant': (32769, lambda M, G: 128 * G, 0.1, 100),
}


@pytest.mark.parametrize('kind,mutant', [(k, m) for k in fr.BWD_KINDS for m in sorted(BWD_MUTANT_LAUNCH)
                                         if not (m == 'padded_hidden_columns' and k == 'ao')])     # (the attention tail has no hidden width)
def test_wrong_backward_variants_fail_a_one_row_launch(kind, mutant):
    assert mutant in fr.MUTANTS
    M, row, rate, F = BWD_MUTANT_LAUNCH[mutant]
    G = min(-(-M // 32), fr.CAP_BWD)
    r = row(M, G)
    assert r in fr.tile_edges(M, fr.CAP_BWD)
    _rejected_bwd(kind, M, F, rate, [r], mutant)


@pytest.mark.parametrize('kind', fr.BWD_KINDS)
@pytest.mark.parametrize('mutant,M', [('odd_last_row_stats', 8193), ('stats_halves_swapped', 8193), ('keep_shifted', 8193),
                                      ('past_M_into_dbeta', 33)])
def test_wrong_backward_variants_fail_the_unlike_rows(kind, mutant, M):
    """what the dense family sees on its own (it cannot see one lost or doubled row: its row-sum bounds grow with M)"""
    _rejected_bwd(kind, M, 100, 0.1, torch.arange(M), mutant)


@pytest.mark.parametrize('kind', fr.FWD_KINDS)
@pytest.mark.parametrize('mutant,M', [('fwd_stats_row_xor_1', 33), ('tile_4G_previous_occupant', 65537)])
def test_wrong_forward_variants_fail_the_unlike_rows(kind, mutant, M):
    assert mutant in fr.MUTANTS
    c = fr.fwd_case(M, 100)
    with pytest.raises(AssertionError):
        fr.check_fwd(fr.fwd_ref(c, kind, 0.1), fr.emulate_fwd(c, kind, 0.1, mutant=mutant))


def test_every_wrong_variant_is_rejected_somewhere():
    seen = set(BWD_MUTANT_LAUNCH) | {'fwd_stats_row_xor_1', 'tile_4G_previous_occupant'}
    assert seen == set(fr.MUTANTS)
