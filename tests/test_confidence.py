"""The matcher's confidence map on the host: depthestimation_amd/confidence.py (the restatement K2's
confidence variant is tested against), the C-ABI struct, and the keywords of every layer.  No device needed."""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from depthestimation_amd import _dsx
from depthestimation_amd.census import cost_volume_census
from depthestimation_amd.confidence import apply_threshold, peak_ratio, uniqueness_bound, valid_band
from depthestimation_amd.synthetic import layered_pair, stereo_pair
from oracle.sgm import aggregate
from oracle.stereo_bm import cost_volume, wta_epilogue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vol(costs, W=None, x=None):
    """A 1 x W x D volume whose pixel x (default: the last column) holds `costs`; the others hold 7s."""
    D = len(costs)
    W = W or D + 3
    x = W - 1 if x is None else x
    C = np.full((1, W, D), 7, np.int64)
    C[0, x] = costs
    return C, x


# ---------------------------------------------------------------- known answers ---------------
@pytest.mark.parametrize("costs,want", [
    ([9], 255),                      # D = 1: no rival
    ([9, 3], 255),                   # D = 2
    ([9, 3, 5], 255),                # D = 3, b = 1: both others are neighbours
    ([3, 9, 5], 255 - (255 * 3) // 5),   # D = 3, b = 0: d = 2 is a rival
    ([4, 8, 9, 4], 255 - 255),       # cb == nm (tie, lowest b = 0): 0
    ([0, 5, 0, 3], 0),               # nm == 0: a perfect tie
    ([0, 5, 9, 3], 255),             # cb == 0 < nm
    ([6, 2, 2, 9, 4], 255 - (255 * 2) // 4),  # ties take the lowest b = 1: d = 2 is its neighbour, rival 4
    ([9, 1, 5, 8, 2], 255 - (255 * 1) // 2),
    ([9, 2, 1, 2, 9, 8], 255 - (255 * 1) // 8),  # rivals at b - 1 and b + 1 (cost 2) are ignored: nm = 8
    ([100, 10, 99, 98, 11], 255 - (255 * 10) // 11),
])
def test_known_answers(costs, want):
    C, x = _vol(costs)
    assert x >= len(costs) - 1  # inside the band [D - 1, W - 1]
    q = peak_ratio(C, 0)
    assert q.dtype == np.uint8 and q.shape == (1, C.shape[1])
    assert int(q[0, x]) == want


def test_ssd_15x15_maximum():
    """255 * cb = 3,730,809,375 passes 2^31: the quotient is still exact."""
    top = 225 * 255 * 255
    assert 255 * top == 3730809375 > 2 ** 31
    for dtype in (np.int64, np.uint32):
        C, x = _vol([top, top - 1, top, top, top])          # b = 1, nm = top
        assert int(peak_ratio(C.astype(dtype), 0)[0, x]) == 255 - (255 * (top - 1)) // top == 1
        C, x = _vol([top, top, top, top])                   # all equal: cb == nm
        assert int(peak_ratio(C.astype(dtype), 0)[0, x]) == 0
        C, x = _vol([top // 2, top, top, top])
        assert int(peak_ratio(C.astype(dtype), 0)[0, x]) == 255 - (255 * (top // 2)) // top == 128


@pytest.mark.parametrize("m", [-5, 0, 7])
@pytest.mark.parametrize("lr_form", ["bm", "sgbm"])
def test_bands(m, lr_form):
    W, D = 40, 6
    rng = np.random.default_rng(3)
    C = rng.integers(1, 1000, (2, W, D))
    q = peak_ratio(C, m, lr_form)
    x = np.arange(W)
    band = (x >= m + D - 1) & (x <= W - 1 + m) if lr_form == "bm" else (x >= max(m + D, 0)) & (x < W + min(m, 0))
    np.testing.assert_array_equal(valid_band(W, D, m, lr_form), band)
    assert band.any() and not band.all()
    assert not q[:, ~band].any()
    np.testing.assert_array_equal(q, _loop(C, m, lr_form))
    assert q[:, band].any()
    # the two bands differ: 'sgbm' starts one column later and, for m > 0, runs to the image's edge
    if m == 7:
        assert valid_band(W, D, m, "sgbm")[W - 1] and valid_band(W, D, m, "bm")[W - 1]
        assert valid_band(W, D, m, "bm")[m + D - 1] and not valid_band(W, D, m, "sgbm")[m + D - 1]
    with pytest.raises(ValueError):
        peak_ratio(C, m, "opencv")
    with pytest.raises(ValueError):
        peak_ratio(C.astype(np.float32), m)


def _loop(C, m, lr_form="bm"):
    """The contract, pixel by pixel, in Python integers."""
    H, W, D = C.shape
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            if lr_form == "bm":
                inb = m + D - 1 <= x <= W - 1 + m
            else:
                inb = max(m + D, 0) <= x < W + min(m, 0)
            if not inb:
                continue
            c = [int(v) for v in C[y, x]]
            b = min(range(D), key=lambda d: (c[d], d))
            far = [c[d] for d in range(D) if abs(d - b) > 1]
            if not far:
                out[y, x] = 255
            elif min(far) == 0:
                out[y, x] = 0
            else:
                out[y, x] = 255 - (255 * c[b]) // min(far)
    return out


@pytest.mark.parametrize("seed,D,hi,dtype", [(0, 1, 50, np.int64), (1, 2, 50, np.int32), (2, 3, 4, np.uint16),
                                             (3, 9, 3, np.int64), (4, 17, 60000, np.uint16),
                                             (5, 33, 8 * (57375 + 65535), np.int64),   # SGM-sized sums
                                             (6, 5, 225 * 255 * 255, np.uint32)])
def test_loop_equals_peak_ratio(seed, D, hi, dtype):
    rng = np.random.default_rng(seed)
    C = rng.integers(0, hi + 1, (5, D + 12, D)).astype(dtype)
    if D >= 3:
        C[0, :, :] = C[0, :, :1]          # rows of perfect ties
        C[1, :, 1] = 0                    # cb == 0
    for m, form in ((0, "bm"), (-3, "sgbm"), (4, "bm")):
        np.testing.assert_array_equal(peak_ratio(C, m, form), _loop(C, m, form))


# ---------------------------------------------------------------- uniqueness bound ------------
@functools.lru_cache(maxsize=None)
def _pair_volume():
    L, R, _ = stereo_pair(24, 140, 0, 32, seed=5)
    return cost_volume(L, R, 0, 32, 5, "sad")


@pytest.mark.parametrize("u", [5, 10, 50])
def test_uniqueness_bound(u):
    """Every in-band pixel that uniqueness_ratio u rejects has q <= 255 - (255 (100 - u)) // 100."""
    C = _pair_volume()
    q = peak_ratio(C, 0)
    keep = wta_epilogue(C, 0, 0, -1, True)["fixed"] != -16
    uniq = wta_epilogue(C, 0, u, -1, True)["fixed"] != -16
    rejected = keep & ~uniq
    print(f"u={u}: {int(rejected.sum())} rejected, max q among them {int(q[rejected].max())}, "
          f"bound {uniqueness_bound(u)}")
    assert rejected.sum() > 20
    assert int(q[rejected].max()) <= uniqueness_bound(u)
    assert uniqueness_bound(10) == 26
    # and the converse does not hold pixel for pixel only through the floor: nothing above the bound is rejected
    assert not (rejected & (q > uniqueness_bound(u))).any()


# ---------------------------------------------------------------- the threshold ---------------
def test_threshold_zero_and_monotone():
    C = _pair_volume()
    q = peak_ratio(C, 0)
    ref = wta_epilogue(C, 0, 10, 1, True)
    np.testing.assert_array_equal(apply_threshold(ref["fixed"], q, 0, 0), ref["fixed"])
    np.testing.assert_array_equal(apply_threshold(ref["parabola"], q, 0, 0), ref["parabola"])
    prev = ref["fixed"] != -16
    for t in (1, 16, 32, 64, 128, 255):
        got = apply_threshold(ref["fixed"], q, t, 0)
        assert got.dtype == np.int16
        now = got != -16
        assert not (now & ~prev).any() and now.sum() <= prev.sum()
        np.testing.assert_array_equal(got[now], ref["fixed"][now])
        assert (q[now] >= t).all()
        prev = now
    assert prev.sum() < (ref["fixed"] != -16).sum()
    # the invalid values: (m - 1) * 16 in the fixed map, m - 1 in a float one
    f = apply_threshold(ref["parabola"], q, 255, 3)
    assert f.dtype == np.float32 and (f[q < 255] == np.float32(2)).all()
    assert (apply_threshold(ref["fixed"], q, 255, -4)[q < 255] == -80).all()
    for bad in (-1, 256, 1.5, True):
        with pytest.raises(ValueError):
            apply_threshold(ref["fixed"], q, bad, 0)
    with pytest.raises(ValueError):
        apply_threshold(ref["fixed"], q[:, 1:], 1, 0)


# ---------------------------------------------------------------- quality ---------------------
def _shares(C, gt, D, t):
    """(kept share, share of the kept within 1 px of the truth) on the cropped map, threshold alone."""
    ref = wta_epilogue(C, 0, 0, -1, True)["fixed"]
    fixed = apply_threshold(ref, peak_ratio(C, 0), t, 0)[:, D:]
    kept = fixed != -16
    good = np.abs(fixed.astype(np.float64) / 16.0 - gt[:, D:]) <= 1.0
    return float(kept.mean()), float(good[kept].mean())


@functools.lru_cache(maxsize=None)
def _layered():
    L, R, gt = layered_pair(48, 192, 32)
    sad = cost_volume(L, R, 0, 32, 9, "sad")
    sgm = aggregate(cost_volume_census(L, R, 0, 32, 1, "census9x7"), "sgbm_3way", 8, 32)
    return gt, sad, sgm


@pytest.mark.parametrize("name,floor", [("sad", 0.90), ("census_sgm", 0.95)])
def test_quality_on_layered_scene(name, floor):
    """uniqueness_ratio 0, no LR check: the threshold alone separates right from wrong matches."""
    gt, sad, sgm = _layered()
    C = sad if name == "sad" else sgm
    kept0, good0 = _shares(C, gt, 32, 0)
    kept32, good32 = _shares(C, gt, 32, 32)
    print(f"{name}: t=0 kept {kept0:.3f} good {good0:.3f}; t=32 kept {kept32:.3f} good {good32:.3f}")
    assert kept0 == 1.0
    assert good32 > good0
    assert kept32 >= floor
    if name == "census_sgm":
        kept128, good128 = _shares(C, gt, 32, 128)
        print(f"{name}: t=128 kept {kept128:.3f} good {good128:.3f}")
        assert good128 > good32 and kept128 < kept32


# ---------------------------------------------------------------- C-ABI struct, keywords ------
def test_confidence_struct_matches_header(tmp_path, dsx_lib_path, monkeypatch):
    names = [n for n, _ in _dsx.DsxConfidence._fields_]
    src = tmp_path / "probe_confidence.c"
    body = "".join(f'printf("{f} %zu\\n", offsetof(dsx_confidence, {f}));' for f in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsx.h"\nint main(void){'
                   'printf("sizeof %zu\\n", sizeof(dsx_confidence));'
                   'printf("peak %d\\n", DSX_CONF_PEAK_RATIO);' + body + 'return 0;}\n')
    exe = tmp_path / "probe_confidence"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    lay = dict((k, int(v)) for k, v in (line.split() for line in out.splitlines()))
    assert lay.pop("sizeof") == ctypes.sizeof(_dsx.DsxConfidence) == 32
    assert lay.pop("peak") == _dsx.CONFIDENCE["peak_ratio"] == 1
    assert lay == {n: getattr(_dsx.DsxConfidence, n).offset for n in names}
    assert lay["type"] == 0 and lay["threshold"] == 4 and lay["reserved"] == 8
    import importlib.util
    monkeypatch.setenv("DSX_LIB", dsx_lib_path)
    spec = importlib.util.spec_from_file_location("dsx_matcher_stub", os.path.join(ROOT, "integration", "dsx_matcher.py"))
    stub = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stub)
    assert ctypes.sizeof(stub._Confidence) == 32
    assert [(n, getattr(stub._Confidence, n).offset) for n, _ in stub._Confidence._fields_] == \
           [(n, getattr(_dsx.DsxConfidence, n).offset) for n in names]


def test_check_confidence_accepts_and_rejects():
    L = _dsx.lib()
    d = _dsx.DsxConfidence()
    L.dsx_default_confidence(ctypes.byref(d))
    assert (d.type, d.threshold, list(d.reserved)) == (1, 0, [0] * 6)
    p = _dsx.make_params()
    for t in (0, 1, 255):
        c = _dsx.make_confidence(t)
        assert c.threshold == t
        assert L.dsx_check_confidence(ctypes.byref(p), ctypes.byref(c)) == _dsx.DSX_OK
        assert L.dsx_check_confidence(None, ctypes.byref(c)) == _dsx.DSX_OK
    for t in (-1, 256, 1.5, "3", True, None):
        with pytest.raises((ValueError, TypeError)):
            _dsx.make_confidence(t)
    for t in (-1, 256):
        d.threshold = t
        assert L.dsx_check_confidence(None, ctypes.byref(d)) == _dsx.DSX_EINVAL
        assert "[0, 255]" in _dsx.last_error()
    d.threshold, d.type = 0, 2
    assert L.dsx_check_confidence(None, ctypes.byref(d)) == _dsx.DSX_EINVAL
    assert L.dsx_check_confidence(ctypes.byref(p), None) == _dsx.DSX_EINVAL
    assert L.dsx_set_confidence(None, ctypes.byref(d)) == _dsx.DSX_EINVAL
    # argument errors of the compute calls come before any HIP call (no device here)
    buf = ctypes.create_string_buffer(16)
    assert L.dsx_compute_conf_device(None, buf, buf, 2, 2, 2, None, None, buf, None) == _dsx.DSX_EINVAL
    assert L.dsx_compute_conf_host(None, buf, buf, 2, 2, 2, None, None, buf) == _dsx.DSX_EINVAL
    assert L.dsx_version() == 106


def test_matcher_keyword_and_params_rule():
    from depthestimation_amd.matcher import HipBlockMatcher
    d = HipBlockMatcher()
    assert "confidence_threshold" not in d.params            # off its default only
    assert HipBlockMatcher(**d.params).params == d.params
    on = HipBlockMatcher(confidence_threshold=32)
    assert on.params["confidence_threshold"] == 32
    assert HipBlockMatcher(**on.params).params == on.params
    assert {k: v for k, v in on.params.items() if k != "confidence_threshold"} == d.params
    on.set_params(confidence_threshold=0)                     # no handle yet: only stored
    assert on.params == d.params
    on.set_params(confidence_threshold=255, cost="census9x7")
    assert on.params["confidence_threshold"] == 255 and on.params["cost"] == "census9x7"
    for t in (-1, 256, 2.5, True):
        with pytest.raises(ValueError):
            HipBlockMatcher(confidence_threshold=t)
        with pytest.raises(ValueError):
            on.set_params(confidence_threshold=t)
    assert on.params["confidence_threshold"] == 255
    with pytest.raises(ValueError):
        d.compute(np.zeros((4, 8), np.uint8), np.zeros((4, 8), np.uint8), out_confidence=np.zeros((4, 8), np.int16))
    with pytest.raises(ValueError):
        d.compute(np.zeros((4, 8), np.uint8), np.zeros((4, 8), np.uint8), out_confidence=np.zeros((4, 9), np.uint8))


def test_stereo_core_and_facade_keys():
    from depthestimation_amd.StereoDepthEstimator import StereoDepthEstimator
    from depthestimation_amd.stereo_core import StereoCore
    core = StereoCore()
    p = core.get_sgbm_params()
    assert p["confidence"] is False and p["confidence_threshold"] == 0
    assert core.confidence_map is None
    assert "confidence_threshold" not in core.sgbm.params
    core.configure_sgbm(confidence=True, confidence_threshold=32)
    assert core.get_sgbm_params()["confidence"] is True
    assert core.sgbm.params["confidence_threshold"] == 32
    old = core.sgbm
    for kw in (dict(confidence_threshold=-1), dict(confidence_threshold=256), dict(confidence_threshold=1.5),
               dict(confidence_threshold=True), dict(confidence_threshold="32"), dict(confidence=1),
               dict(confidence="yes"), dict(confidence=None)):
        with pytest.raises(ValueError, match="Invalid parameter value for 'confidence"):
            core.configure_sgbm(**kw)
        assert core.sgbm is old
    with pytest.raises(ValueError):
        core.configure_sgbm(confidence_map=True)  # unknown keys are still rejected
    est = StereoDepthEstimator()
    assert est.confidence_map is None
    with pytest.raises(AttributeError):
        est.confidence_map = np.zeros((2, 2), np.uint8)
