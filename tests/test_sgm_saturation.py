"""Preconditions of the saturated SGM parity tests (tests/test_gpu_sgm_edges.py), on the CPU.

The concurrent SGM form stores L_r as u16 and is taken only while max cost + P2 < 65535
(dsx_plan.h sgm_concurrent()).  Textured ``stereo_pair`` inputs leave L_r below a third of that
bound (largest L_r of the older tests: 18,955 of 66,375), so the GPU tests use thresholded and striped
inputs instead.  These tests assert with the oracle that those inputs really put L_r and the sums on
the limits, so a later change of the generators cannot quietly turn the GPU tests back into easy
ones.  The figures in the docstrings were measured with the oracle (seed 7)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from depthestimation_amd.synthetic import STRIPE_COLS, binary_pair, stereo_pair, striped_pair
from oracle.bt_cost import cost_volume_bt, max_cost_bt
from oracle.sgm import DIRECTIONS, path_costs
from oracle.sgm_cases import SATURATED, make_pair
from oracle.stereo_bm import cost_volume, max_cost, wta_epilogue

MODES = ("sgbm_3way", "sgbm", "hh")


@functools.lru_cache(maxsize=None)
def _paths(name):
    """(C, [L_r for the 8 directions of 'hh']) of a SATURATED case; shared, never modified."""
    c = SATURATED[name]
    L, R = make_pair(c)
    C = cost_volume(L, R, c["m"], c["D"], c["bs"], "sad")
    Ls = [path_costs(C, r, c["p1"], c["p2"]) for r in DIRECTIONS["hh"]]
    for a in [C] + Ls:
        a.setflags(write=False)
    return C, Ls


def _lr_max(name):
    return [int(L.max()) for L in _paths(name)[1]]


def _sums(name, mode):
    _, Ls = _paths(name)
    return sum(Ls[DIRECTIONS["hh"].index(r)] for r in DIRECTIONS[mode])


def _map_stats(name, mode, u, lr):
    """(distinct valid integer disparities, valid share) of the oracle's map."""
    c = SATURATED[name]
    fixed = wta_epilogue(_sums(name, mode), c["m"], u, lr, True)["fixed"]
    valid = fixed >= c["m"] * 16
    return len(np.unique(fixed[valid] >> 4)), float(valid.mean())


def test_generators():
    L0, R0, d0 = stereo_pair(21, 75, -2, 24, seed=5)
    Lb, Rb, db = binary_pair(21, 75, -2, 24, seed=5)
    np.testing.assert_array_equal(Lb, np.where(L0 > 127, 255, 0))
    np.testing.assert_array_equal(Rb, np.where(R0 > 127, 255, 0))
    np.testing.assert_array_equal(db, d0)
    assert Lb.dtype == Rb.dtype == np.uint8 and set(np.unique(Lb)) == {0, 255} == set(np.unique(Rb))
    Ls, Rs, _ = striped_pair(21, 75, -2, 24, seed=5)
    stripes = np.tile((np.arange(STRIPE_COLS) % 2) * 255, (21, 1))
    assert STRIPE_COLS == 40
    np.testing.assert_array_equal(Ls[:, :40], stripes)
    np.testing.assert_array_equal(Rs[:, :40], stripes)
    np.testing.assert_array_equal(Ls[:, 40:], Lb[:, 40:])
    np.testing.assert_array_equal(Rs[:, 40:], Rb[:, 40:])
    assert Ls.dtype == Rs.dtype == np.uint8
    Ln, Rn, _ = striped_pair(5, 9, 0, 4, seed=1)  # narrower than the stripes
    np.testing.assert_array_equal(Ln, Rn)
    np.testing.assert_array_equal(Ln[0], [0, 255, 0, 255, 0, 255, 0, 255, 0])


def test_striped_block_costs_alternate():
    """Where the window and its shifted copy stay inside the stripes, every odd disparity costs
    255 * bs^2 = 2295 and every even one 0."""
    C, _ = _paths("striped_at_bound")
    inside = C[:, 16:39, :]  # x - 1 - 15 >= 0 and x + 1 <= 39
    assert (inside[:, :, 1::2] == 2295).all() and (inside[:, :, 0::2] == 0).all()
    assert int(C.max()) == 2295 == max_cost(3, "sad")


def test_striped_pair_sits_on_the_concurrent_bound():
    """P1 = P2 = 63239, bs 3: 2295 + 63239 = 65,534, the last bound the concurrent form accepts.
    Measured: C.max() = 2295; L_r max = 65,534 in each of the 8 directions; S.max() ('hh') = 350,114."""
    c = SATURATED["striped_at_bound"]
    C, Ls = _paths("striped_at_bound")
    assert max_cost(c["bs"], "sad") + c["p2"] == 65534
    assert int(C.max()) == 2295
    assert _lr_max("striped_at_bound") == [65534] * 8
    for L in Ls:
        assert (L >= C).all() and (L <= C + c["p2"]).all()
    assert int(_sums("striped_at_bound", "hh").max()) == 350114


def test_striped_pair_one_past_the_bound():
    """P1 = P2 = 63240: bound 65,535, the first that must go sequential (65,535 is the u16 pad).
    Measured: L_r max = 65,535 in every direction; S.max() ('hh') = 350,115."""
    c = SATURATED["striped_over_bound"]
    assert max_cost(c["bs"], "sad") + c["p2"] == 65535
    assert _lr_max("striped_over_bound") == [65535] * 8
    assert int(_sums("striped_over_bound", "hh").max()) == 350115


def test_binary_pair_reaches_the_bound_with_a_varied_map():
    """binary_pair(33, 96, 0, 16), bs 3, P1 = P2 = 63239.  Measured L_r max per direction ('hh'
    order): 65024, 65534, 54315, 54315, 32895, 37995, 39015, 32895; S.max() = 201,705.  With
    uniqueness 10 and disp12 1 the map has 9 distinct valid integer disparities in each mode and
    72.3 % (sgbm_3way), 66.6 % (sgbm), 65.7 % (hh) valid pixels."""
    mx = _lr_max("binary_at_bound")
    assert max(mx) >= 65534 and min(mx) >= 32000, mx
    assert max(mx) <= 65534
    for mode in MODES:
        distinct, share = _map_stats("binary_at_bound", mode, 10, 1)
        assert distinct >= 6 and 0.3 <= share <= 0.9, (mode, distinct, share)


def test_binary_pair_four_disparities_per_lane():
    """binary_pair(H, W, -2, 144), bs 5, P1 = 100, P2 = 59159: Dp = 256, bound 6375 + 59159 = 65,534.

    (40, 100): measured L_r max per direction 65534, 65279, 65279, 65534, 65279, 65279, 65279,
    65279; S.max() = 442,661.  W = 100 < m + D, so the valid band m + D - 1 <= x <= W - 1 + m is
    empty: the map is invalid at every pixel for every seed and every uniqueness / disp12 setting,
    and a map of that shape cannot tell a wrong path sum from a right one.
    (30, 230) has the band (x >= 141, 37.8 % of the pixels): measured L_r max = 65,534 in all 8
    directions, S.max() = 412,788, and with uniqueness 0 and disp12 -1 the map has 20 (sgbm_3way),
    20 (sgbm), 9 (hh) distinct valid integer disparities."""
    c = SATURATED["binary_npl4_at_bound"]
    assert max_cost(c["bs"], "sad") + c["p2"] == 65534
    for name in ("binary_npl4_at_bound", "binary_npl4_wide"):
        mx = _lr_max(name)
        assert min(mx) >= 65000 and max(mx) <= 65534, (name, mx)
    for mode in MODES:
        assert _map_stats("binary_npl4_at_bound", mode, 0, -1) == (0, 0.0)
        distinct, share = _map_stats("binary_npl4_wide", mode, 0, -1)
        assert distinct >= 6 and 0.3 <= share <= 0.9, (mode, distinct, share)


def test_largest_penalties_need_32_bit_sums():
    """binary_pair(24, 64, 0, 32), bs 15, P1 = P2 = 65535 (the largest legal penalties).  Measured:
    C.max() = 45,135 of 57,375; L_r max per direction 110670, 110670, 109650, 110670, 109650, 107355,
    110670, 110670; S.max() ('hh') = 858,840.  Every direction exceeds what a u16 can hold."""
    L, R, _ = binary_pair(24, 64, 0, 32, seed=7)
    C = cost_volume(L, R, 0, 32, 15, "sad")
    mx = [int(path_costs(C, r, 65535, 65535).max()) for r in DIRECTIONS["hh"]]
    assert min(mx) > 0xFFFF, mx
    assert max(mx) <= max_cost(15, "sad") + 65535


@pytest.mark.parametrize("gen", [binary_pair, striped_pair])
def test_bt_costs_stay_below_the_bound_the_host_trusts(gen):
    """sgm_concurrent() trusts max_cost_bt = bs^2 (2 ftzero + 63) (42,525 at bs 15, cap 63).  Measured
    C.max() over the volume: binary_pair(24, 64, 0, 32) 16,435 (38.6 % of the bound), striped_pair
    15,087 (35.5 %): the two channels cannot both be extreme at one pixel (a saturated gradient
    needs an edge, a saturated raw difference flat regions), so the bound is safe but not tight.
    A block of 255 against 0 saturates the raw channel alone: bs^2 * 63, a third of the bound; the
    inputs must reach at least that."""
    L, R, _ = gen(24, 64, 0, 32, seed=7)
    C = cost_volume_bt(L, R, 0, 32, 15, 63)
    bound = max_cost_bt(15, 63)
    assert bound == 42525
    print(gen.__name__, "BT C.max()", int(C.max()), "of", bound)
    assert 0 <= int(C.min()) and int(C.max()) <= bound
    assert int(C.max()) >= bound // 3
