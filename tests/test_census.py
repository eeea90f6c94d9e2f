"""Census costs ('census9x7', 'census5x5'; include/dsx.h DSX_COST_CENSUS*): the host restatement
(depthestimation_amd/census.py) against plain loops written from the contract, known answers, the
robustness rows of DESIGN.md 4.3e and the parameter validation.  The device side is tests/test_gpu_census.py."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from depthestimation_amd import _dsx
from depthestimation_amd.census import (census_bits, census_transform, cost_volume_census, max_cost_census,
                                        popcount64)
from depthestimation_amd.synthetic import stereo_pair
from oracle.sgm import aggregate
from oracle.stereo_bm import wta_epilogue

WIN = {"census9x7": (9, 7), "census5x5": (5, 5)}


# ---------------------------------------------------------------- loops from the contract ----
def _loop_code(I, x, y, wx, wy):
    H, W = len(I), len(I[0])
    rx, ry = wx // 2, wy // 2
    code, k = 0, 0
    for j in range(-ry, ry + 1):
        for i in range(-rx, rx + 1):
            if i == 0 and j == 0:
                continue
            xx = min(max(x + i, 0), W - 1)
            yy = min(max(y + j, 0), H - 1)
            if I[yy][xx] < I[y][x]:
                code |= 1 << k
            k += 1
    return code


def _loop_volume(L, R, m, D, bs, wx, wy):
    H, W = len(L), len(L[0])
    TL = [[_loop_code(L, x, y, wx, wy) for x in range(W)] for y in range(H)]
    TR = [[_loop_code(R, x, y, wx, wy) for x in range(W)] for y in range(H)]
    r = bs // 2
    C = np.zeros((H, W, D), np.int64)
    for y in range(H):
        for x in range(W):
            for d in range(D):
                s = 0
                for j in range(-r, r + 1):
                    yy = min(max(y + j, 0), H - 1)
                    for i in range(-r, r + 1):
                        xl = min(max(x + i, 0), W - 1)
                        xr = min(max(x + i - m - d, 0), W - 1)
                        s += bin(TL[yy][xl] ^ TR[yy][xr]).count("1")
                C[y, x, d] = s
    return TL, C


@pytest.mark.parametrize("cost", ["census9x7", "census5x5"])
@pytest.mark.parametrize("H,W,m,D,bs", [(5, 9, 0, 4, 3), (4, 7, -2, 5, 1), (1, 1, 0, 2, 1), (3, 2, 0, 3, 3),
                                        (2, 13, 1, 7, 7), (7, 3, 0, 2, 15)])
def test_vectorised_matches_loop_restatement(H, W, m, D, bs, cost):
    rng = np.random.default_rng(H * 100 + W)
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    wx, wy = WIN[cost]
    TL, C = _loop_volume(L.tolist(), R.tolist(), m, D, bs, wx, wy)
    T = census_transform(L, cost)
    assert T.dtype == np.uint64
    assert T.tolist() == TL
    got = cost_volume_census(L, R, m, D, bs, cost)
    assert got.dtype == np.int64 and got.shape == (H, W, D)
    np.testing.assert_array_equal(got, C)


# ---------------------------------------------------------------- known answers ---------------
@pytest.mark.parametrize("cost", ["census9x7", "census5x5"])
def test_known_answers(cost):
    wx, wy = WIN[cost]
    rx, ry = wx // 2, wy // 2
    n = wx * wy - 1
    assert census_bits(cost) == n == {"census9x7": 62, "census5x5": 24}[cost]
    assert max_cost_census(15, cost) == 225 * n
    np.testing.assert_array_equal(popcount64(np.array([0, 1, 2 ** 62 - 1, 2 ** 64 - 1], np.uint64)), [0, 1, 62, 64])
    # a constant image codes to 0 (the comparison is strict)
    assert not census_transform(np.full((9, 12), 77, np.uint8), cost).any()
    # a monotone map leaves the codes alone
    rng = np.random.default_rng(1)
    a = rng.integers(0, 128, (11, 17), dtype=np.uint8)
    np.testing.assert_array_equal(census_transform(a, cost), census_transform((2 * a + 1).astype(np.uint8), cost))
    # bit order: a single dark pixel at (xd, yd) is neighbour (-rx, -ry) of the pixel at (xd + rx, yd + ry)
    # (bit 0) and neighbour (+rx, +ry) of the pixel at (xd - rx, yd - ry) (the last bit)
    b = np.full((4 * ry + 1, 4 * rx + 1), 200, np.uint8)
    yd, xd = 2 * ry, 2 * rx
    b[yd, xd] = 10
    T = census_transform(b, cost)
    assert int(T[yd + ry, xd + rx]) == 1
    assert int(T[yd - ry, xd - rx]) == 1 << (n - 1)
    assert int(T[yd, xd + 1]) == 1 << (n // 2 - 1)  # the left neighbour: the last one before the centre
    assert int(T[yd, xd - 1]) == 1 << (n // 2)      # the right neighbour: the first one after it
    assert int(T[yd, xd]) == 0
    assert int(T.max()) < 1 << n
    # a view against itself costs 0 at d = 0
    C = cost_volume_census(a, a, 0, 4, 5, cost)
    assert not C[..., 0].any() and C[..., 1:].any()
    # the maximum: every neighbour strictly above or strictly below the centre, against the negation
    ys, xs = np.mgrid[0:12, 0:20]
    c = ((ys * 20 + xs) * 37 % 251).astype(np.uint8)  # 37 is a unit mod 251: distinct values within any window
    inner = (slice(ry, 12 - ry), slice(rx, 20 - rx))
    Tc, Tn = census_transform(c, cost), census_transform(255 - c, cost)
    np.testing.assert_array_equal((Tc ^ Tn)[inner], np.uint64((1 << n) - 1))
    for bs in (1, 3):
        Cn = cost_volume_census(c, 255 - c, 0, 1, bs, cost)
        assert Cn.max() <= max_cost_census(bs, cost)
        r = bs // 2
        assert (Cn[ry + r:12 - ry - r, rx + r:20 - rx - r, 0] == bs * bs * n).all()


def test_restatement_rejects_bad_arguments():
    a = np.zeros((4, 4), np.uint8)
    for bad in (lambda: census_transform(a, "census"), lambda: census_transform(a.astype(np.int32)),
                lambda: cost_volume_census(a, a, 0, 4, 2), lambda: cost_volume_census(a, a, 0, 0, 3),
                lambda: cost_volume_census(a, a[:2], 0, 4, 3), lambda: census_transform(a[:0])):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------- robustness rows -------------
def test_robustness_rows():
    """DESIGN.md 4.3e, on the pair of tests/test_prefilter.py::test_robustness_table (another gain and a
    shading ramp in the right camera; raw SAD 0.515 there).  Measured: census 9x7 block 7 0.983
    (undisturbed 0.984), 5x5 block 7 0.985, 9x7 block 1 0.936, block 1 + sgbm_3way (P1 8, P2 32) 0.998."""
    L, R, gt = stereo_pair(48, 160, 0, 32, seed=3)
    x = np.arange(160)[None, :]
    R2 = np.clip(np.rint(0.7 * R + 0.9 * x), 0, 255).astype(np.uint8)
    want = np.rint(16 * gt)

    def share(C):
        f = wta_epilogue(C, 0, 0, -1, True)["fixed"].astype(np.float64)
        return float((np.abs(f - want)[7:41, 38:153] <= 16).mean())

    b7 = share(cost_volume_census(L, R2, 0, 32, 7, "census9x7"))
    b7u = share(cost_volume_census(L, R, 0, 32, 7, "census9x7"))
    b7s = share(cost_volume_census(L, R2, 0, 32, 7, "census5x5"))
    C1 = cost_volume_census(L, R2, 0, 32, 1, "census9x7")
    b1 = share(C1)
    sgm = share(aggregate(C1, "sgbm_3way", 8, 32))
    sgm5 = share(aggregate(cost_volume_census(L, R2, 0, 32, 1, "census5x5"), "sgbm_3way", 8, 32))
    print(f"correct share: census9x7 b7 {b7:.3f} (undisturbed {b7u:.3f}) census5x5 b7 {b7s:.3f} "
          f"census9x7 b1 {b1:.3f} b1+sgbm_3way 9x7 {sgm:.3f} 5x5 {sgm5:.3f}")
    assert b7 > 0.9
    assert sgm > 0.9


# ---------------------------------------------------------------- validation ------------------
@pytest.mark.parametrize("cost,code,bits", [("census9x7", 3, 62), ("census5x5", 4, 24)])
def test_params_validation(cost, code, bits):
    assert _dsx.COST[cost] == code
    for bs in (1, 15):
        p = _dsx.make_params(cost=cost, block_size=bs, num_disp=512)
        assert p.cost == code
        _dsx.check_params(p)
        for agg in ("sgbm_3way", "hh4", "sgbm", "hh"):
            _dsx.check_params(_dsx.make_params(cost=cost, block_size=bs, num_disp=256, aggregation=agg))
            _dsx.check_params(_dsx.make_params(cost=cost, block_size=bs, num_disp=64, aggregation=agg, p1=8,
                                               p2=60000))
    for kw in (dict(block_size=2), dict(block_size=17), dict(num_disp=513), dict(num_disp=257, aggregation="hh")):
        with pytest.raises(ValueError):
            _dsx.check_params(_dsx.make_params(cost=cost, **kw))
    f = _dsx.make_prefilter()
    _dsx.check_prefilter(_dsx.make_params(cost=cost), f)  # no filter, no threshold: fine
    for kw in (dict(prefilter_type="xsobel"), dict(prefilter_type="mean"),
               dict(prefilter_type="xsobel", texture_threshold=100)):
        with pytest.raises(ValueError, match="census ranks intensities itself"):
            _dsx.check_prefilter(_dsx.make_params(cost=cost), _dsx.make_prefilter(**kw))
    f.texture_threshold = 5  # a threshold without a filter
    with pytest.raises(ValueError, match="census ranks intensities itself"):
        _dsx.check_prefilter(_dsx.make_params(cost=cost), f)


def test_bare_name_and_unknown_codes_stay_invalid():
    with pytest.raises(ValueError):
        _dsx.make_params(cost="census")
    assert "census" not in _dsx.COST
    p = _dsx.make_params()
    for bad in (5, -1):
        p.cost = bad
        with pytest.raises(ValueError, match="CENSUS9X7"):
            _dsx.check_params(p)
    # SSD stays the only cost SGM refuses
    with pytest.raises(ValueError, match="SGM aggregation"):
        _dsx.check_params(_dsx.make_params(cost="ssd", aggregation="hh"))


def test_struct_layout_unchanged():
    assert ctypes.sizeof(_dsx.DsxParams) == 22 * 4
    assert [n for n, _ in _dsx.DsxParams._fields_][-1] == "reserved"
    assert _dsx.DsxParams.reserved.offset == 20 * 4 and _dsx.DsxParams.cost.offset == 3 * 4
    assert hasattr(_dsx.lib(), "dsx_census_device") and "dsx_census_device" in _dsx.EXPORTS


def test_matcher_rejects_census_on_a_prefiltered_matcher():
    from depthestimation_amd.matcher import HipBlockMatcher
    with pytest.raises(ValueError):
        HipBlockMatcher(cost="census9x7", prefilter_type="xsobel")
    with pytest.raises(ValueError):
        HipBlockMatcher(cost="census5x5", prefilter_type="mean", texture_threshold=50)
    m = HipBlockMatcher(cost="sad", prefilter_type="mean", texture_threshold=50)  # no handle yet: host checks only
    before = m.params
    with pytest.raises(ValueError, match="census ranks intensities itself"):
        m.set_params(cost="census9x7")
    assert m.params == before and m.params["cost"] == "sad" and m.params["prefilter_type"] == "mean"
    m.set_params(cost="census9x7", prefilter_type="none", texture_threshold=0)  # filter off in the same set: fine
    assert m.params["cost"] == "census9x7"
    with pytest.raises(ValueError):
        m.set_params(prefilter_type="xsobel")
    assert m.prefilter_params["prefilter_type"] == "none"


def test_stereo_core_census_key():
    from depthestimation_amd.stereo_core import StereoCore
    core = StereoCore()
    core.configure_sgbm(cost="census9x7")
    assert core.sgbm.params["cost"] == "census9x7" and core.get_sgbm_params()["cost"] == "census9x7"
    core.configure_sgbm(cost="census5x5", aggregation="sgm", block_size=1)
    assert core.sgbm.params["cost"] == "census5x5" and core.sgbm.params["aggregation"] == "sgbm_3way"
    assert (core.sgbm.params["p1"], core.sgbm.params["p2"]) == (8, 32)
    with pytest.raises(ValueError):
        core.configure_sgbm(cost="census")
    with pytest.raises(ValueError):
        StereoCore().configure_sgbm(cost="census9x7", prefilter_type="xsobel")


class _StubMatcher:
    def __init__(self, **kw):
        self.params = dict(kw)

    def close(self):
        pass


@pytest.mark.parametrize("kw,r", [
    (dict(block_size=5), 2), (dict(block_size=5, cost="census9x7"), 2 + 3), (dict(block_size=1, cost="census9x7"), 3),
    (dict(block_size=7, cost="census5x5"), 3 + 2), (dict(block_size=15, cost="bt"), 7),
    (dict(block_size=9, cost="sad", prefilter_type="mean", prefilter_size=11), 4 + 5),
])
def test_banded_halo_covers_the_census_window(monkeypatch, kw, r):
    from depthestimation_amd import multigpu
    monkeypatch.setattr(multigpu, "HipBlockMatcher", _StubMatcher)
    monkeypatch.setattr(multigpu._dsx, "device_count", lambda: 4)
    b = multigpu.BandedStereo(devices=[0, 1, 2], **kw)
    assert b.r == r
    b.close()
