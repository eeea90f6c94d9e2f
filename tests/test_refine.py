"""The image-guided weighted median (dsx_refine in include/dsx.h), host side: the vectorised restatement
against a pure-Python loop straight from the definition, the weight table and the argument checks of the
C-ABI (host-only calls: no device is touched), the chain's keywords, and the quality the filter is for."""
from __future__ import annotations

import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from depthestimation_amd import _dsx
from depthestimation_amd import postprocess as pp
from depthestimation_amd.stereo_core import StereoCore
from depthestimation_amd.synthetic import layered_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_wmedian(d, g, r, sigma, fill):
    """The definition, pixel by pixel, with Python numbers only."""
    T = [max(1, int(math.floor(256.0 * math.exp(-k / sigma) + 0.5))) for k in range(256)]
    d = np.asarray(d, np.float32)
    H, W = d.shape
    out = d.copy()
    ob = out.view(np.uint32)

    def valid(v):
        v = float(v)
        return v > 0.0 and v < math.inf  # NaN compares false

    for y in range(H):
        for x in range(W):
            taps = []
            for j in range(-r, r + 1):
                for i in range(-r, r + 1):
                    yy, xx = y + j, x + i
                    if 0 <= yy < H and 0 <= xx < W and valid(d[yy, xx]):
                        taps.append((float(d[yy, xx]), T[abs(int(g[y, x]) - int(g[yy, xx]))], d.view(np.uint32)[yy, xx]))
            if not taps or (not valid(d[y, x]) and not fill):
                continue
            S = sum(w for _, w, _ in taps)
            for v, _, bits in sorted(taps):
                if 2 * sum(w for u, w, _ in taps if u <= v) >= S:
                    ob[y, x] = bits
                    break
    return out


def _inputs(shape, kind, seed):
    rng = np.random.default_rng(seed)
    H, W = shape
    g = rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "quantised":       # k / 16, as the matcher's maps
        d = (rng.integers(0, 40 * 16, shape) / 16.0).astype(np.float32)
    elif kind == "floats":        # arbitrary floats, tiny and huge ones included
        d = np.exp(rng.uniform(-80, 80, shape)).astype(np.float32)
        d.ravel()[rng.integers(0, d.size, max(1, d.size // 8))] = np.float32(1e-42)  # a denormal: valid
    elif kind == "equal":         # many equal values: few distinct keys, ties everywhere
        d = rng.choice(np.array([3.0, 3.0, 3.0, 7.5, 12.25], np.float32), shape)
        g = (g // 64 * 64).astype(np.uint8)
    else:
        raise AssertionError(kind)
    bad = np.array([np.nan, np.inf, 0.0, -0.0, -1.0, -np.inf], np.float32)
    m = rng.random(shape) < 0.3
    d[m] = rng.choice(bad, int(m.sum()))
    return d, g


_SHAPES = [(1, 1), (5, 9), (6, 7), (9, 12)]


@pytest.mark.parametrize("kind", ["quantised", "floats", "equal"])
@pytest.mark.parametrize("shape", _SHAPES)
def test_host_equals_definition(shape, kind):
    d, g = _inputs(shape, kind, seed=shape[0] * 100 + shape[1])
    for r, sigma in ((1, 1), (3, 8), (7, 64)):   # 6 x 7 with r = 7: the window is larger than the image
        for fill in (False, True):
            want = brute_wmedian(d, g, r, sigma, fill)
            got = pp.weighted_median_filter(d, g, radius=r, sigma=sigma, fill=fill)
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"{shape} {kind} r{r} s{sigma}")
            # a selection: every output bit pattern occurs in the input
            assert np.isin(got.view(np.uint32), d.view(np.uint32)).all()
            if not fill:
                inv = ~((d > 0) & (d < np.inf))
                np.testing.assert_array_equal(got.view(np.uint32)[inv], d.view(np.uint32)[inv])


def test_all_invalid_map_passes_unchanged():
    d = np.array([[np.nan, 0.0, -1.0], [np.inf, -0.0, -np.inf]], np.float32)
    g = np.zeros((2, 3), np.uint8)
    got = pp.weighted_median_filter(d, g, radius=2, sigma=8, fill=True)
    np.testing.assert_array_equal(got.view(np.uint32), d.view(np.uint32))


def test_exact_tie_takes_the_lower_value():
    """Two values with equal weights: 2 * w(lower) == S exactly, so the lower one satisfies the rule."""
    d = np.array([[5.0, 9.0]], np.float32)
    g = np.array([[100, 100]], np.uint8)          # equal guide: both taps weigh T[0] at both pixels
    got = pp.weighted_median_filter(d, g, radius=1, sigma=8, fill=True)
    np.testing.assert_array_equal(got, [[5.0, 5.0]])
    np.testing.assert_array_equal(brute_wmedian(d, g, 1, 8, True), [[5.0, 5.0]])
    # a tie through the weights: at x = 1 the far value's weight T[0] equals the two near taps' 2 * T[k]
    T = pp.wmedian_weights(13)
    k = 9
    assert 2 * int(T[k]) == int(T[0]) == 256        # sigma 13: T[9] = 128
    d = np.array([[2.0, 6.0, 2.0]], np.float32)
    g = np.array([[k, 0, k]], np.uint8)
    got = pp.weighted_median_filter(d, g, radius=1, sigma=13, fill=True)
    assert got[0, 1] == 2.0                        # weights 2.0: 2 * T[k], 6.0: T[0] -> tie -> lower
    np.testing.assert_array_equal(got.view(np.uint32), brute_wmedian(d, g, 1, 13, True).view(np.uint32))
    # one grey level further apart and the centre's own value wins
    g2 = np.array([[k + 1, 0, k + 1]], np.uint8)
    assert pp.weighted_median_filter(d, g2, radius=1, sigma=13, fill=True)[0, 1] == 6.0


def test_bad_arguments_host():
    d = np.ones((4, 4), np.float32)
    g = np.zeros((4, 4), np.uint8)
    for kw in (dict(radius=0), dict(radius=8), dict(sigma=0), dict(sigma=65), dict(sigma=2.5)):
        with pytest.raises(ValueError):
            pp.weighted_median_filter(d, g, **kw)
    with pytest.raises(ValueError):
        pp.weighted_median_filter(d, g[:, :3])
    with pytest.raises(ValueError):
        pp.weighted_median_filter(d, g.astype(np.float32))


# --------------------------------------------------------------------------- C-ABI, host-only calls
def test_weight_table_equals_c(dsx_lib_path):
    L = _dsx.lib()
    for sigma in range(1, 65):
        out = (ctypes.c_uint16 * 256)()
        assert L.dsx_wmedian_weights(sigma, out) == _dsx.DSX_OK
        np.testing.assert_array_equal(np.array(out, np.uint16), pp.wmedian_weights(sigma))
    t = pp.wmedian_weights(8)
    assert t[0] == 256 and t.min() == 1 and np.all(np.diff(t.astype(int)) <= 0)
    out = (ctypes.c_uint16 * 256)()
    assert L.dsx_wmedian_weights(0, out) == _dsx.DSX_EINVAL
    assert L.dsx_wmedian_weights(65, out) == _dsx.DSX_EINVAL
    assert L.dsx_wmedian_weights(8, None) == _dsx.DSX_EINVAL


def test_check_refine(dsx_lib_path):
    L = _dsx.lib()
    rf = _dsx.DsxRefine()
    L.dsx_default_refine(ctypes.byref(rf))
    assert (rf.type, rf.radius, rf.sigma, rf.fill) == (_dsx.REFINE["none"], 5, 8, 1)
    assert list(rf.reserved) == [0, 0, 0, 0]
    assert L.dsx_check_refine(ctypes.byref(rf)) == _dsx.DSX_OK
    rf.type = _dsx.REFINE["wmedian"]
    assert L.dsx_check_refine(ctypes.byref(rf)) == _dsx.DSX_OK
    for field, bad in (("radius", 0), ("radius", 8), ("sigma", 0), ("sigma", 65), ("type", 2), ("type", -1), ("fill", 2)):
        q = _dsx.DsxRefine.from_buffer_copy(rf)
        setattr(q, field, bad)
        assert L.dsx_check_refine(ctypes.byref(q)) == _dsx.DSX_EINVAL, (field, bad)
        assert _dsx.last_error()
    for field, ok in (("radius", 1), ("radius", 7), ("sigma", 1), ("sigma", 64), ("fill", 0)):
        q = _dsx.DsxRefine.from_buffer_copy(rf)
        setattr(q, field, ok)
        assert L.dsx_check_refine(ctypes.byref(q)) == _dsx.DSX_OK, (field, ok)
    assert L.dsx_check_refine(None) == _dsx.DSX_EINVAL
    with pytest.raises(ValueError):
        _dsx.make_refine("bilateral")
    with pytest.raises(ValueError):
        _dsx.make_refine("wmedian", refine_radius=8)
    assert _dsx.make_refine("wmedian", 3, 16, False).fill == 0


def test_wmedian_device_argument_errors_need_no_device(dsx_lib_path):
    """Argument errors are reported before any HIP call: these return DSX_EINVAL on a host without a GPU."""
    L = _dsx.lib()
    rf = _dsx.make_refine("wmedian")
    a, b, g = 0x1000, 0x2000, 0x3000    # never dereferenced
    assert L.dsx_wmedian_device(a, 4, 4, 4, g, 4, ctypes.byref(rf), a, None) == _dsx.DSX_EINVAL    # out is in
    assert L.dsx_wmedian_device(a, 4, 4, 4, None, 4, ctypes.byref(rf), b, None) == _dsx.DSX_EINVAL  # no guide
    assert L.dsx_wmedian_device(a, 4, 4, 3, g, 4, ctypes.byref(rf), b, None) == _dsx.DSX_EINVAL    # pitch < W
    assert L.dsx_wmedian_device(a, 4, 4, 4, g, 3, ctypes.byref(rf), b, None) == _dsx.DSX_EINVAL    # stride < W
    assert L.dsx_wmedian_device(a, 4, 4, 4, g, 4, None, b, None) == _dsx.DSX_EINVAL
    off = _dsx.make_refine("none")
    assert L.dsx_wmedian_device(a, 4, 4, 4, g, 4, ctypes.byref(off), b, None) == _dsx.DSX_EINVAL


def test_refine_layout_equals_gcc(tmp_path):
    """dsx_refine as gcc lays it out equals the ctypes mirror (size and every offset)."""
    fields = [f for f, _ in _dsx.DsxRefine._fields_]
    c = tmp_path / "rf.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsx.h"\nint main(void){printf("%zu", sizeof(dsx_refine));'
                 + "".join(f'printf(" %zu", offsetof(dsx_refine, {f}));' for f in fields)
                 + 'printf(" %d %d", DSX_REFINE_NONE, DSX_REFINE_WMEDIAN);return 0;}\n')
    exe = tmp_path / "rf"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_dsx.DsxRefine)] + [getattr(_dsx.DsxRefine, f).offset for f in fields]
    assert got[:-2] == want
    assert got[-2:] == [_dsx.REFINE["none"], _dsx.REFINE["wmedian"]]
    assert ctypes.sizeof(_dsx.DsxRefine) == 32


# --------------------------------------------------------------------------- the chain's keywords
def _chain_map(seed=5):
    rng = np.random.default_rng(seed)
    d = np.full((24, 40), 9.0, np.float32)
    d[:, 20:] = 14.5
    d[rng.random(d.shape) < 0.1] = -1.0
    g = np.where(np.arange(40)[None, :] < 18, 50, 200).astype(np.uint8) + rng.integers(0, 6, d.shape, dtype=np.uint8)
    return d, g


def test_postprocess_disparity_refine_keywords():
    d, g = _chain_map()
    kw = dict(max_speckle_size=20, max_diff=1.0, outlier_threshold=2.5, apply_outlier_removal=True,
              apply_hole_filling=False)
    base = pp.postprocess_disparity(d, **kw)
    # 'none' (and an unused guide) leave the chain exactly as it was
    for extra in (dict(refine="none"), dict(refine="none", left_image=g), dict(left_image=g), dict(refine=None)):
        np.testing.assert_array_equal(pp.postprocess_disparity(d, **kw, **extra).view(np.uint32), base.view(np.uint32))
    with pytest.raises(ValueError):
        pp.postprocess_disparity(d, refine="wmedian", **kw)                         # no left_image
    with pytest.raises(ValueError):
        pp.postprocess_disparity(d, refine="wmedian", left_image=g[:, 1:], **kw)     # wrong shape
    with pytest.raises(ValueError):
        pp.postprocess_disparity(d, refine="wmedian", left_image=g.astype(np.float32), **kw)
    with pytest.raises(ValueError):
        pp.postprocess_disparity(d, refine="bilateral", left_image=g, **kw)
    got = pp.postprocess_disparity(d, refine="wmedian", left_image=g, refine_radius=3, refine_sigma=8, **kw)
    # the stage sits between the outlier removal and the median
    pre = pp.filter_speckles(d, 20, 1.0)
    pre[pp.detect_outliers(pre, threshold=2.5, kernel_size=5)] = 0
    want = pp.median_blur3(pp.weighted_median_filter(pre, g, radius=3, sigma=8, fill=True))
    np.testing.assert_array_equal(got, want)
    assert np.any(got != base) and not np.any(got <= 0)
    nofill = pp.postprocess_disparity(d, refine="wmedian", left_image=g, refine_fill=False, **kw)
    assert np.any(nofill <= 0)


def test_stereo_core_refine_keys():
    core = StereoCore(fast_mode=False)
    p = core.get_sgbm_params()
    assert (p["refine"], p["refine_radius"], p["refine_sigma"], p["refine_fill"]) == ("none", 5, 8, True)
    core.configure_sgbm(refine="wmedian", refine_radius=7, refine_sigma=16, refine_fill=False)
    assert core._refine_kwargs() == dict(refine="wmedian", refine_radius=7, refine_sigma=16, refine_fill=False)
    for bad in (dict(refine="bilateral"), dict(refine_radius=0), dict(refine_radius=8), dict(refine_sigma=0),
                dict(refine_sigma=65), dict(refine_sigma=2.5)):
        with pytest.raises(ValueError):
            StereoCore(fast_mode=False).configure_sgbm(**bad)
    assert "refine" not in core.sgbm.params        # per call: the matcher's own parameters are unchanged

    # host path: _process_pair hands the cropped left image to the chain
    D = 16
    L, R, _ = layered_pair(24, 96, D, seed=3, disparities=(3, 7, 4), levels=(60, 200, 110))
    core = StereoCore(fast_mode=False)
    core.configure_sgbm(num_disp=D, block_size=5, refine="wmedian", refine_radius=5)
    fixed = _oracle_fixed(24, 96, D, 5, 3, (3, 7, 4), (60, 200, 110))
    core.compute_disparity = lambda l, r: fixed.astype(np.float32) / 16.0
    got, _ = core._process_pair(L, R)
    want = pp.postprocess_disparity(fixed.astype(np.float32)[:, D:] / 16.0, left_image=L[:, D:], max_speckle_size=100,
                                    max_diff=1.0, outlier_threshold=2.5, apply_outlier_removal=True,
                                    apply_hole_filling=False, refine="wmedian", refine_radius=5, refine_sigma=8)
    np.testing.assert_array_equal(got, want)
    core.fast_mode = True                           # fast mode ignores the keys, as it ignores hole_filling
    np.testing.assert_array_equal(core._process_pair(L, R)[0], pp.median_blur3(fixed.astype(np.float32)[:, D:] / 16.0))


# --------------------------------------------------------------------------- what the filter is for
@functools.lru_cache(maxsize=None)
def _oracle_fixed(H, W, D, bs, seed, disparities=(6, 12, 7, 13, 8), levels=(60, 200, 100, 240, 140)):
    from oracle.stereo_bm import stereo_bm
    L, R, _ = layered_pair(H, W, D, seed=seed, disparities=disparities, levels=levels)
    return stereo_bm(L, R, min_disp=0, num_disp=D, block_size=bs, cost="sad", uniqueness_ratio=10, disp12_max_diff=1,
                     subpixel=True)["fixed"]


def test_layered_pair_is_occlusion_correct():
    H, W, D = 12, 192, 32
    L, R, gt = layered_pair(H, W, D, seed=1)
    assert L.dtype == np.uint8 and R.dtype == np.uint8 and gt.dtype == np.float32 and gt.shape == (H, W)
    assert sorted(np.unique(gt[:, D:]).tolist()) == [6.0, 7.0, 8.0, 12.0, 13.0]
    xs = np.arange(W)[None, :] - gt.astype(int)
    vis = np.take_along_axis(R, np.clip(xs, 0, W - 1), 1) == L
    # a left pixel shows in the right view unless a nearer layer covers it: the hidden ones are the
    # background just left of a foreground layer's left edge (the disparity rises there), a band as wide
    # as the jump; everything else is visible
    rise = np.nonzero(np.diff(gt[0]) > 0)[0] + 1
    want_hidden = np.zeros((H, W), bool)
    for x in rise:
        jump = int(gt[0, x] - gt[0, x - 1])
        want_hidden[:, x - jump:x] = True
    assert len(rise) == 2 and want_hidden[:, D:].mean() > 0.05
    np.testing.assert_array_equal(~vis[:, D:], want_hidden[:, D:])
    with pytest.raises(ValueError):
        layered_pair(8, 64, 8, disparities=(9,), levels=(10,))


def test_quality_on_the_layered_scene():
    """Share of pixels within 1 px of the truth in the cropped map, 48 x 192, D = 32, SAD 9 x 9: the guided
    median with filling beats 'nearest' by at least 0.02, which beats no filling by at least 0.02
    (measured with seed 1234: none 0.848, nearest 0.886, wmedian 0.913; equal weights - sigma 64 - 0.900)."""
    H, W, D = 48, 192, 32
    L, _, gt = layered_pair(H, W, D, seed=1234)
    d = _oracle_fixed(H, W, D, 9, 1234).astype(np.float32)[:, D:] / 16.0
    g, t = L[:, D:], gt[:, D:]
    kw = dict(left_image=g, max_speckle_size=100, max_diff=1.0, outlier_threshold=2.5, apply_outlier_removal=True)

    def share(o):
        return float(np.mean(np.abs(o - t) <= 1.0))

    none = share(pp.postprocess_disparity(d, apply_hole_filling=False, **kw))
    nearest = share(pp.postprocess_disparity(d, apply_hole_filling=True, fill_method="nearest", **kw))
    wm = share(pp.postprocess_disparity(d, apply_hole_filling=False, refine="wmedian", refine_radius=7, refine_sigma=8,
                                        refine_fill=True, **kw))
    flat = share(pp.postprocess_disparity(d, apply_hole_filling=False, refine="wmedian", refine_radius=7,
                                          refine_sigma=64, refine_fill=True, **kw))
    print(f"correct share: none {none:.3f}  nearest {nearest:.3f}  wmedian {wm:.3f}  wmedian sigma 64 {flat:.3f}")
    assert wm >= nearest + 0.02
    assert nearest + 0.02 >= none + 0.04
    assert wm > flat           # the image, not the median alone, earns the margin
