"""Matcher prefilter and texture threshold on the CPU: the host restatements
(depthestimation_amd/prefilter.py) against the oracle's x-derivative channel and against plain loops,
the robustness table of DESIGN.md section 4.3d, parameter validation and the dsx_prefilter layout.  No
test here needs a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from depthestimation_amd import _dsx
from depthestimation_amd.prefilter import (apply_texture_threshold, prefilter_mean, prefilter_xsobel,
                                           texture_sum)
from depthestimation_amd.synthetic import stereo_pair
from oracle.bt_cost import channels
from oracle.stereo_bm import stereo_bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _img(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---------------------------------------------------------------- restatements ----------
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 2), (7, 13)])
@pytest.mark.parametrize("c", [15, 31, 63])
def test_xsobel_is_the_oracles_channel(shape, c):
    a = _img(shape, 5 + shape[0] * 31 + shape[1] + c)
    P = prefilter_xsobel(a, c)
    assert P.dtype == np.uint8 and P.shape == a.shape
    np.testing.assert_array_equal(P, channels(a, c)[0])


def test_xsobel_known_answers():
    for c in (1, 15, 31, 63):
        np.testing.assert_array_equal(prefilter_xsobel(np.full((5, 9), 77, np.uint8), c), c)
        step = np.zeros((4, 8), np.uint8)
        step[:, 4:] = 255
        P = prefilter_xsobel(step, c)
        # the derivative is 4 * 255 at the two columns that straddle the step, 0 elsewhere
        want = np.full((4, 8), c, np.int64)
        want[:, 3:5] = 2 * c
        np.testing.assert_array_equal(P, want)
        Pi = prefilter_xsobel(255 - step, c)
        want[:, 3:5] = 0
        np.testing.assert_array_equal(Pi, want)
    # c = 1: the sign of the derivative
    a = np.array([[10, 20, 30, 30, 5, 5]], np.uint8)
    np.testing.assert_array_equal(prefilter_xsobel(a, 1), [[1, 2, 2, 0, 0, 1]])


def _mean_loops(a, n, c):
    H, W = a.shape
    r = n // 2
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            s = 0
            for j in range(-r, r + 1):
                for i in range(-r, r + 1):
                    s += int(a[min(max(y + j, 0), H - 1), min(max(x + i, 0), W - 1)])
            mu = (s + (n * n) // 2) // (n * n)
            out[y, x] = min(max(int(a[y, x]) - mu, -c), c) + c
    return out


def _texture_loops(p, k, c):
    H, W = p.shape
    r = k // 2
    out = np.zeros((H, W), np.uint16)
    for y in range(H):
        for x in range(W):
            s = 0
            for j in range(-r, r + 1):
                for i in range(-r, r + 1):
                    s += abs(int(p[min(max(y + j, 0), H - 1), min(max(x + i, 0), W - 1)]) - c)
            out[y, x] = s
    return out


@pytest.mark.parametrize("shape,n,c", [((3, 4), 21, 31), ((9, 14), 5, 63), ((6, 7), 9, 1), ((1, 1), 7, 15)])
def test_mean_against_loops(shape, n, c):
    a = _img(shape, n + c)
    P = prefilter_mean(a, n, c)
    assert P.dtype == np.uint8 and int(P.max()) <= 2 * c
    np.testing.assert_array_equal(P, _mean_loops(a, n, c))


@pytest.mark.parametrize("shape,k,c", [((3, 4), 15, 31), ((9, 14), 5, 63), ((6, 7), 1, 7), ((1, 1), 9, 15)])
def test_texture_sum_against_loops(shape, k, c):
    p = np.random.default_rng(k).integers(0, 2 * c + 1, shape, dtype=np.uint8)
    T = texture_sum(p, k, c)
    assert T.dtype == np.uint16
    np.testing.assert_array_equal(T, _texture_loops(p, k, c))


def test_constant_image_has_no_texture():
    a = np.full((8, 11), 200, np.uint8)
    for n in (5, 9, 21):
        P = prefilter_mean(a, n, 31)
        np.testing.assert_array_equal(P, 31)
        np.testing.assert_array_equal(texture_sum(P, 7, 31), 0)
    np.testing.assert_array_equal(texture_sum(prefilter_xsobel(a, 31), 15, 31), 0)


def test_apply_texture_threshold():
    fixed = np.arange(12, dtype=np.int16).reshape(3, 4)
    T = np.array([[0, 9, 10, 11]] * 3, np.uint16)
    out = apply_texture_threshold(fixed, T, 10, min_disp=-2)
    assert out.dtype == np.int16
    np.testing.assert_array_equal(out[:, :2], -48)
    np.testing.assert_array_equal(out[:, 2:], fixed[:, 2:])
    np.testing.assert_array_equal(apply_texture_threshold(fixed, T, 0), fixed)
    np.testing.assert_array_equal(fixed, np.arange(12).reshape(3, 4))  # the input is left alone


def test_restatements_reject_bad_arguments():
    a = _img((4, 4), 0)
    for bad in (lambda: prefilter_xsobel(a, 0), lambda: prefilter_xsobel(a, 64), lambda: prefilter_mean(a, 4),
                lambda: prefilter_mean(a, 3), lambda: prefilter_mean(a, 23), lambda: texture_sum(a, 2),
                lambda: texture_sum(a, 17), lambda: prefilter_xsobel(a.astype(np.int32))):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------- robustness table ------
def test_robustness_table():
    """the same SAD matcher on a pair whose right camera has another gain and a
    horizontal shading ramp.  Measured: raw 0.515, xsobel 0.946, mean 0.980 (undisturbed 0.985)."""
    L, R, gt = stereo_pair(48, 160, 0, 32, seed=3)
    x = np.arange(160)[None, :]
    R2 = np.clip(np.rint(0.7 * R + 0.9 * x), 0, 255).astype(np.uint8)
    want = np.rint(16 * gt)

    def share(a, b):
        f = stereo_bm(a, b, 0, 32, 7, "sad", 0, -1, True)["fixed"].astype(np.float64)
        return float((np.abs(f - want)[7:41, 38:153] <= 16).mean())

    raw = share(L, R2)
    xs = share(prefilter_xsobel(L, 31), prefilter_xsobel(R2, 31))
    mean = share(prefilter_mean(L, 9, 31), prefilter_mean(R2, 9, 31))
    print(f"correct share: raw {raw:.3f} xsobel {xs:.3f} mean {mean:.3f} undisturbed {share(L, R):.3f}")
    assert raw < 0.6
    assert xs > 0.9
    assert mean > 0.9


# ---------------------------------------------------------------- validation ------------
def test_check_prefilter_accepts_and_rejects():
    d = _dsx.DsxPrefilter()
    _dsx.lib().dsx_default_prefilter(ctypes.byref(d))
    assert (d.type, d.size, d.cap, d.texture_threshold) == (0, 9, 31, 0)
    p = _dsx.make_params()
    _dsx.check_prefilter(p, d)
    _dsx.check_prefilter(p, _dsx.make_prefilter())
    _dsx.check_prefilter(p, _dsx.make_prefilter("mean", 21, 63, 65535))
    _dsx.check_prefilter(None, _dsx.make_prefilter("xsobel", 9, 1, 1))
    bad = [dict(prefilter_type="mean", prefilter_size=8), dict(prefilter_type="mean", prefilter_size=3),
           dict(prefilter_type="mean", prefilter_size=23), dict(prefilter_type="xsobel", prefilter_size=6),
           dict(prefilter_type="xsobel", prefilter_cap=0), dict(prefilter_type="mean", prefilter_cap=64),
           dict(prefilter_type="xsobel", texture_threshold=-1), dict(prefilter_type="xsobel", texture_threshold=65536),
           dict(prefilter_type="none", texture_threshold=5)]
    for kw in bad:
        with pytest.raises(ValueError):
            _dsx.check_prefilter(p, _dsx.make_prefilter(**kw))
    f = _dsx.make_prefilter("xsobel")
    f.type = 3
    with pytest.raises(ValueError):
        _dsx.check_prefilter(p, f)
    with pytest.raises(ValueError):
        _dsx.make_prefilter("sobel")
    bt = _dsx.make_params(cost="bt")
    _dsx.check_prefilter(bt, _dsx.make_prefilter())  # no filter: fine
    for t in ("xsobel", "mean"):
        with pytest.raises(ValueError, match="BT"):
            _dsx.check_prefilter(bt, _dsx.make_prefilter(t))
    assert _dsx.lib().dsx_check_prefilter(ctypes.byref(p), None) == _dsx.DSX_EINVAL


def test_prefilter_struct_matches_header(tmp_path, dsx_lib_path, monkeypatch):
    names = [n for n, _ in _dsx.DsxPrefilter._fields_]
    src = tmp_path / "probe_prefilter.c"
    body = "".join(f'printf("{f} %zu\\n", offsetof(dsx_prefilter, {f}));' for f in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsx.h"\nint main(void){'
                   'printf("sizeof %zu\\n", sizeof(dsx_prefilter));' + body + 'return 0;}\n')
    exe = tmp_path / "probe_prefilter"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    lay = dict((k, int(v)) for k, v in (line.split() for line in out.splitlines()))
    assert lay.pop("sizeof") == ctypes.sizeof(_dsx.DsxPrefilter) == 32
    assert lay == {n: getattr(_dsx.DsxPrefilter, n).offset for n in names}
    # the reference-side binding declares the same struct
    import importlib.util
    monkeypatch.setenv("DSX_LIB", dsx_lib_path)
    spec = importlib.util.spec_from_file_location("dsx_matcher_stub", os.path.join(ROOT, "integration", "dsx_matcher.py"))
    stub = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(stub)
    assert ctypes.sizeof(stub._Prefilter) == 32
    assert [(n, getattr(stub._Prefilter, n).offset) for n, _ in stub._Prefilter._fields_] == \
           [(n, getattr(_dsx.DsxPrefilter, n).offset) for n in names]


def test_matcher_keywords_validate_without_a_device():
    from depthestimation_amd.matcher import HipBlockMatcher
    m = HipBlockMatcher(prefilter_type="mean", prefilter_size=21, prefilter_cap=63, texture_threshold=100)
    assert m.params["prefilter_type"] == "mean" and m.params["prefilter_size"] == 21
    assert m.params["texture_threshold"] == 100 and m.params["prefilter_cap"] == 63
    m.set_params(prefilter_type="xsobel", texture_threshold=0)  # no handle yet: only stored
    assert m.params["prefilter_type"] == "xsobel"
    with pytest.raises(ValueError):
        m.set_params(cost="bt")
    assert m.params["cost"] == "sad"
    m.set_params(cost="bt", prefilter_type="none")
    with pytest.raises(ValueError):
        m.set_params(prefilter_type="mean")
    assert m.prefilter_params["prefilter_type"] == "none"
    d = HipBlockMatcher()
    assert d.prefilter_params == dict(prefilter_type="none", prefilter_size=9, prefilter_cap=31, texture_threshold=0)
    assert not set(d.params) & {"prefilter_type", "prefilter_size", "texture_threshold"}  # as before the feature
    assert HipBlockMatcher(**d.params).params == d.params
    on = HipBlockMatcher(prefilter_type="xsobel")
    assert on.params["prefilter_type"] == "xsobel" and HipBlockMatcher(**on.params).params == on.params
    for kw in (dict(texture_threshold=5), dict(prefilter_type="mean", prefilter_size=4),
               dict(prefilter_type="xsobel", prefilter_cap=64), dict(prefilter_type="xsobel", cost="bt")):
        with pytest.raises(ValueError):
            HipBlockMatcher(**kw)


def test_stereo_core_keys():
    from depthestimation_amd.stereo_core import StereoCore
    core = StereoCore()
    p = core.get_sgbm_params()
    assert (p["prefilter_type"], p["prefilter_size"], p["texture_threshold"]) == ("none", 9, 0)
    core.configure_sgbm(prefilter_type="mean", prefilter_size=11, texture_threshold=12, prefilter_cap=20)
    p = core.get_sgbm_params()
    assert (p["prefilter_type"], p["prefilter_size"], p["texture_threshold"]) == ("mean", 11, 12)
    mp = core.sgbm.params
    assert (mp["prefilter_type"], mp["prefilter_size"], mp["texture_threshold"], mp["prefilter_cap"]) == \
           ("mean", 11, 12, 20)
    old = core.sgbm
    for kw in (dict(prefilter_type="sobel"), dict(prefilter_size=10), dict(cost="bt")):
        with pytest.raises(ValueError):
            core.configure_sgbm(**kw)
        assert core.sgbm is old
    with pytest.raises(ValueError):
        core.configure_sgbm(prefilter="xsobel")  # unknown keys are still rejected
