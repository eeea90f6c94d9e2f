"""Joint bilateral upsampling of a downscaled run's map (dsx_upsample in include/dsx.h), host side: the
restatement (depthestimation_amd/upsample.py) against a plain loop written from the rule, the integer geometry
against the library, the struct, the checks and the argument errors of the C calls, what the rule buys over
nearest-neighbour upsampling on a scene with odd edges, slants and fractional factors, and the StereoCore keys
and host path.  No test here needs a GPU."""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from depthestimation_amd import _dsx
from depthestimation_amd.input import resize_area
from depthestimation_amd.postprocess import wmedian_weights
from depthestimation_amd.stereo_core import StereoCore
from depthestimation_amd.temporal import TemporalFilter
from depthestimation_amd.upsample import (guide_gray, joint_upsample, nearest_upsample, upsample_taps, upsample_x0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
_BAD = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, -7.25], np.float32)
_DEPTH = dict(focal_length=517.3, baseline=0.193, doffs=0.25, eps=0.5, max_depth=90.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# --------------------------------------------------------------------------- the rule as a plain loop
def _loop_upsample(d, x0, g, G, r, sigma, max_diff, depth=None):
    """The rule of include/dsx.h pixel by pixel: Python integers for the geometry and the weights, one numpy
    float32 scalar operation per float step.  Returns (out bits, depth bits or None)."""
    h, w = d.shape
    Wl = g.shape[1]
    H, W = G.shape[:2]
    T = [int(v) for v in wmedian_weights(sigma)]
    md = F32(max_diff)
    sx = F32(W / Wl)
    inf = F32(np.inf)
    X0 = max(0, -((Wl - 2 * W * x0) // (2 * Wl)))
    out = np.zeros((H, W - X0), np.uint32)
    z = np.zeros((H, W - X0), np.uint32) if depth else None

    def near(X, I, O):
        return ((2 * X + 1) * O) // (2 * I)

    def tent(X, t, I, O):
        k = near(X, I, O) + t - r
        n = abs((2 * X + 1) * O - (2 * k + 1) * I)
        return max(0, 64 - ((64 * n + (r + 1) * I) // (2 * (r + 1) * I)))

    def gray(px):
        if np.ndim(px) == 0:
            return int(px)
        return (int(px[0]) * 1868 + int(px[1]) * 9617 + int(px[2]) * 4899 + 8192) >> 14

    def depth_of(v):
        fB = F32(depth["focal_length"] * depth["baseline"])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            adj = F32(v + F32(depth["doffs"]))
            zz = F32(fB / adj) if adj > F32(depth["eps"]) else inf
        if depth.get("max_depth") is not None and zz > F32(depth["max_depth"]):
            zz = F32(depth["max_depth"])
        return zz

    for Y in range(H):
        for X in range(X0, W):
            Gp = gray(G[Y, X])
            taps = []                                               # (value, weight) of the valid taps, window order
            for j in range(2 * r + 1):
                y = near(Y, H, h) + j - r
                for i in range(2 * r + 1):
                    x = near(X, W, Wl) + i - r
                    if not (0 <= y < h and 0 <= x - x0 < w):
                        continue
                    v = d[y, x - x0]
                    if not (v > 0 and v < inf):
                        continue
                    taps.append((v, tent(X, i, W, Wl) * tent(Y, j, H, h) * T[abs(Gp - int(g[y, x]))]))
            if not taps:
                v = d[near(Y, H, h), near(X, W, Wl) - x0]
                out[Y, X - X0] = v.view(np.uint32)
                if depth:
                    z[Y, X - X0] = depth_of(v).view(np.uint32)
                continue
            S = sum(wq for _, wq in taps)
            m = min(v for v, _ in taps if 2 * sum(wq for u, wq in taps if u <= v) >= S)
            num, den = F32(0), 0
            with np.errstate(over="ignore", invalid="ignore"):
                for v, wq in taps:
                    if abs(F32(v - m)) <= md:
                        num = F32(num + F32(F32(wq) * v))
                        den += wq
                assert den >= 1
                a = F32(num / F32(den))
                out[Y, X - X0] = F32(a * sx).view(np.uint32)
            if depth:
                z[Y, X - X0] = depth_of(a).view(np.uint32)
    return out, z


_PAIRS = [(1, 1, 1, 1), (5, 9, 2, 4), (7, 243, 3, 121), (9, 97, 6, 64), (10, 50, 4, 20), (6, 11, 6, 11)]
_KINDS = ("grid", "floats", "equal", "ties", "invalid", "allinvalid")


def _case(H, W, h, Wl, x0, kind, ch, seed):
    """A low-resolution map of one ``kind``, its guide and a full-size guide."""
    rng = np.random.default_rng(seed)
    w = Wl - x0
    g = rng.integers(0, 256, (h, Wl), dtype=np.uint8)
    G = rng.integers(0, 256, (H, W) if ch == 1 else (H, W, 3), dtype=np.uint8)
    if kind == "grid":
        d = rng.integers(1, 40 * 16, (h, w)).astype(np.float32) / 16
    elif kind == "floats":                                          # arbitrary positive floats of every magnitude
        d = np.exp(rng.uniform(-80, 80, (h, w))).astype(np.float32)
        d[rng.random((h, w)) < 0.1] = np.float32(3.0e38)           # sums that overflow
        d[rng.random((h, w)) < 0.1] = np.float32(1e-45)            # the smallest positive value is valid
    elif kind == "equal":
        d = rng.choice(np.array([3.0, 3.0625, 9.5], np.float32), (h, w))
    elif kind == "ties":                                            # flat guides: symmetric weights, exact ties
        d = rng.integers(16, 20, (h, w)).astype(np.float32) / 4
        g[:] = 77
        G[:] = 77
    elif kind == "invalid":
        d = rng.integers(1, 40 * 16, (h, w)).astype(np.float32) / 16
        m = rng.random((h, w)) < 0.5
        d[m] = rng.choice(_BAD, int(m.sum()))
    else:                                                           # whole windows without a valid tap
        d = rng.choice(_BAD, (h, w))
        if w > 8:
            d[:, -2:] = 5.5
    return d, g, G


@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("pair", _PAIRS, ids=lambda p: "%dx%d_from_%dx%d" % p)
def test_loop_form_equals_vectorised_form(pair, r):
    H, W, h, Wl = pair
    x0s = [x for x in (0, 1, 5, Wl - 1) if 0 <= x <= Wl - 1]
    k = 0
    for kind in _KINDS:
        for x0 in (x0s if H * W < 1000 else [x0s[(k + r) % len(x0s)]]):
            md = (2.0 ** -4, 1.0, 1e6)[k % 3]
            ch = (1, 3)[(k // 3 + r) % 2]
            depth = _DEPTH if k % 2 else dict(_DEPTH, max_depth=None)
            d, g, G = _case(H, W, h, Wl, x0, kind, ch, seed=100 * r + k)
            want, wz = _loop_upsample(d, x0, g, G, r, 8 if k % 4 else 3, md, depth)
            got, gz = joint_upsample(d, x0, g, G, r, 8 if k % 4 else 3, md, **depth)
            assert got.shape == want.shape == (H, W - upsample_x0(W, Wl, x0))
            np.testing.assert_array_equal(_bits(got), want, err_msg=f"{kind} x0={x0} md={md} ch={ch}")
            np.testing.assert_array_equal(_bits(gz), wz, err_msg=f"depth {kind} x0={x0} md={md} ch={ch}")
            k += 1


@pytest.mark.parametrize("md", [2.0 ** -4, 1.0, 1e6])
@pytest.mark.parametrize("ch", [1, 3])
def test_every_x0_max_diff_and_channel_count(md, ch):
    for (H, W, h, Wl) in ((5, 9, 2, 4), (10, 50, 4, 20)):
        for x0 in sorted({0, 1, min(5, Wl - 1), Wl - 1}):
            d, g, G = _case(H, W, h, Wl, x0, "invalid", ch, seed=x0)
            want, _ = _loop_upsample(d, x0, g, G, 1, 8, md)
            got, none = joint_upsample(d, x0, g, G, 1, 8, md)
            assert none is None
            np.testing.assert_array_equal(_bits(got), want)


def test_no_valid_tap_keeps_the_centre_bits_unscaled():
    d = np.array([[np.nan, -1.0], [0.0, np.inf]], np.float32)
    d.view(np.uint32)[0, 0] = 0x7FC12345                            # a NaN with a payload
    g = np.zeros((2, 2), np.uint8)
    G = np.zeros((4, 4), np.uint8)
    out, z = joint_upsample(d, 0, g, G, **_DEPTH)
    np.testing.assert_array_equal(_bits(out), np.repeat(np.repeat(_bits(d), 2, 0), 2, 1))
    # the depth rule applied to that value: adj <= eps (or NaN) -> +inf, clamped; d = +inf -> fB / inf = 0
    np.testing.assert_array_equal(z, np.repeat(np.repeat(np.array([[90, 90], [90, 0]], np.float32), 2, 0), 2, 1))
    out, z = joint_upsample(d, 0, g, G, **dict(_DEPTH, max_depth=None))
    assert np.isinf(z[:, :2]).all() and np.isinf(z[:2]).all() and (z[2:, 2:] == 0).all()


def test_identity_shape_with_flat_map_returns_it():
    d = np.full((6, 11), 7.25, np.float32)
    g = np.arange(66, dtype=np.uint8).reshape(6, 11)
    out, _ = joint_upsample(d, 0, g, g)
    np.testing.assert_array_equal(out, d)                           # an average of equal values is that value


def test_inputs_are_checked():
    d = np.ones((2, 3), np.float32)
    g = np.zeros((2, 4), np.uint8)
    G = np.zeros((5, 9), np.uint8)
    joint_upsample(d, 1, g, G)
    for args in ((d.astype(np.float64), 1, g, G), (d, 0, g, G), (d, 1, g.astype(np.int8), G), (d, 1, g[:1], G),
                 (d, 1, g, G[:1]), (d, 1, g, G[:, :3]), (d, 1, g, np.zeros((5, 9, 2), np.uint8)), (d, -1, g, G)):
        with pytest.raises(ValueError):
            joint_upsample(*args)
    for kw in (dict(radius=0), dict(radius=4), dict(radius=1.5), dict(sigma=0), dict(sigma=65), dict(max_diff=0),
               dict(max_diff=float("nan")), dict(max_diff=float("inf")), dict(max_diff="1"), dict(radius=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            joint_upsample(d, 1, g, G, **kw)
    empty, z = joint_upsample(np.ones((2, 0), np.float32), 4, g, G, focal_length=1.0, baseline=1.0)
    assert empty.shape == z.shape == (5, 0)


# --------------------------------------------------------------------------- the C helpers
def test_taps_equal_the_library_for_every_size_pair():
    lib = _dsx.lib()
    for I in range(1, 65):
        near = (ctypes.c_int32 * I)()
        for r in (1, 2, 3):
            tent = (ctypes.c_int32 * (I * (2 * r + 1)))()
            for O in range(1, I + 1):
                assert lib.dsx_upsample_taps(I, O, r, near, tent) == _dsx.DSX_OK
                n, t = upsample_taps(I, O, r)
                assert (np.frombuffer(near, np.int32) == n).all()
                assert (np.frombuffer(tent, np.int32).reshape(I, 2 * r + 1) == t).all()
                assert n.max() <= O - 1 and n.min() >= 0 and (np.diff(n) >= 0).all() and (np.diff(n) <= 1).all()
                assert t[:, r].min() > 0                            # the centre tap always weighs
                assert t.min() >= 1 and t.max() <= 64               # and within radius 3 no tent reaches 0


def test_x0_is_the_smallest_column_whose_near_reaches_x0():
    lib = _dsx.lib()
    for W in range(1, 65):
        for Wl in range(1, W + 1):
            near, _ = upsample_taps(W, Wl, 1)
            for x0 in range(0, Wl + 1):
                want = int(np.searchsorted(near, x0, side="left"))  # near is non-decreasing; W when none reaches
                assert upsample_x0(W, Wl, x0) == want == lib.dsx_upsample_x0(W, Wl, x0), (W, Wl, x0)
    assert upsample_x0(32768, 32768, 32768) == lib.dsx_upsample_x0(32768, 32768, 32768) == 32768
    assert upsample_x0(32768, 16384, 8000) == lib.dsx_upsample_x0(32768, 16384, 8000) == 16000
    for bad in ((0, 0, 0), (4, 5, 0), (4, 2, 3), (4, 2, -1), (32769, 4, 0)):
        assert lib.dsx_upsample_x0(*bad) == _dsx.DSX_EINVAL
        with pytest.raises(ValueError):
            upsample_x0(*bad)
    lib.dsx_upsample_x0(4, 2, 0)                                    # a good call clears the message
    assert _dsx.last_error() == ""


def test_taps_argument_errors():
    lib, E = _dsx.lib(), _dsx.DSX_EINVAL
    a = (ctypes.c_int32 * 64)()
    for args in ((0, 0, 1, a, a), (4, 5, 1, a, a), (4, 0, 1, a, a), (4, 2, 0, a, a), (4, 2, 4, a, a), (4, 2, 1, None, a),
                 (4, 2, 1, a, None), (32769, 2, 1, a, a)):
        assert lib.dsx_upsample_taps(*args) == E, args
    for args in ((0, 0, 1), (4, 5, 1), (4, 2, 0), (4, 2, 4)):
        with pytest.raises(ValueError):
            upsample_taps(*args)


# --------------------------------------------------------------------------- struct, checks, argument errors
def test_struct_layout_matches_c(tmp_path):
    """dsx_upsample as gcc lays it out equals the ctypes mirror; the tile constants and names too."""
    fields = [f for f, _ in _dsx.DsxUpsample._fields_]
    c = tmp_path / "probe.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsx.h"\nint main(void){'
                 'printf("%d %d %d %d %zu", DSX_UPSAMPLE_NONE, DSX_UPSAMPLE_JOINT, DSX_UPSAMPLE_TILE_W, '
                 'DSX_UPSAMPLE_TILE_H, sizeof(dsx_upsample));'
                 + "".join(f'printf(" %zu", offsetof(dsx_upsample, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    U = _dsx.DsxUpsample
    want = [_dsx.UPSAMPLE["none"], _dsx.UPSAMPLE["joint"], *_dsx.UPSAMPLE_TILE, ctypes.sizeof(U)] + \
        [getattr(U, f).offset for f in fields]
    assert got == want
    assert ctypes.sizeof(U) == 8 * 4 and _dsx.lib().dsx_version() == 106


def test_defaults_and_check_upsample():
    lib = _dsx.lib()
    u = _dsx.DsxUpsample()
    lib.dsx_default_upsample(ctypes.byref(u))
    assert (u.type, u.radius, u.sigma, u.max_diff) == (1, 1, 8, 1.0)
    assert list(u.reserved) == [0] * 4
    assert lib.dsx_check_upsample(ctypes.byref(u)) == _dsx.DSX_OK
    assert lib.dsx_check_upsample(None) == _dsx.DSX_EINVAL
    for kw in (dict(radius=0), dict(radius=4), dict(sigma=0), dict(sigma=65), dict(max_diff=0.0), dict(max_diff=-1.0),
               dict(max_diff=float("nan")), dict(max_diff=float("inf")), dict(max_diff=1e39)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            _dsx.make_upsample(**kw)
    with pytest.raises(ValueError):
        _dsx.make_upsample("bilinear")
    for kw in (dict(radius=1, sigma=1, max_diff=1e-6), dict(radius=3, sigma=64, max_diff=1e6)):
        _dsx.make_upsample(**kw)
    bad = _dsx.DsxUpsample()                                        # type NONE passes whatever the rest holds
    assert lib.dsx_check_upsample(ctypes.byref(bad)) == _dsx.DSX_OK
    bad.type = 2
    assert lib.dsx_check_upsample(ctypes.byref(bad)) == _dsx.DSX_EINVAL


def test_argument_errors_come_before_any_hip_call():
    """Every NULL, short or inconsistent argument is DSX_EINVAL with its own message - reported with no device,
    so nothing of HIP has been touched."""
    lib, E = _dsx.lib(), _dsx.DSX_EINVAL
    up = _dsx.make_upsample()

    def run(disp=0x1000, h=4, w=6, pitch=6, x0=2, g=0x2000, Wl=8, gstride=8, G=0x3000, H=8, W=16, ch=1, Gstride=16,
            params=up, out=0x4000, depth=None, has_max=0):
        rc = lib.dsx_upsample_device(disp, h, w, pitch, x0, g, Wl, gstride, G, H, W, ch, Gstride,
                                     None if params is None else ctypes.byref(params), out, depth, 1.0, 1.0, 0.0, 0.0,
                                     0.0, has_max, None)
        return rc, _dsx.last_error()

    none = _dsx.DsxUpsample()
    for kw, msg in ((dict(disp=None), "d_disp"), (dict(g=None), "d_guide_lo"), (dict(G=None), "d_guide is"),
                    (dict(out=None), "d_out_disp"), (dict(params=None), "NULL upsample"), (dict(params=none), "JOINT"),
                    (dict(Wl=17, w=15), "Wl > W"), (dict(h=9), "h > H"), (dict(x0=-1, w=9), "low-resolution shape"),
                    (dict(h=0), "low-resolution shape"), (dict(w=5), "x0 + w == Wl"), (dict(pitch=5), "pitch"),
                    (dict(gstride=7), "low-resolution guide stride"), (dict(Gstride=15), "guide stride"),
                    (dict(ch=3), "guide stride"), (dict(ch=2), "channels"), (dict(ch=0), "channels"),
                    (dict(H=0), "full-size shape"), (dict(W=32769), "full-size shape"),
                    (dict(has_max=2), "has_max_depth"), (dict(out=0x1000), "d_out_disp must not be d_disp"),
                    (dict(depth=0x1000), "d_out_depth"), (dict(depth=0x4000), "d_out_depth")):
        rc, err = run(**kw)
        assert rc == E and msg in err, (kw, err)
    # nothing to do: no column of the map (x0 == Wl) - no launch, no device needed
    assert run(w=0, x0=8, disp=None, out=None)[0] == _dsx.DSX_OK


def test_symbols_are_exported():
    for name in ("dsx_default_upsample", "dsx_check_upsample", "dsx_upsample_taps", "dsx_upsample_x0",
                 "dsx_upsample_device"):
        assert name in _dsx.EXPORTS and hasattr(_dsx.lib(), name)


# --------------------------------------------------------------------------- what the rule buys
_EDGES = (0, 37, 90, 131, 188, 243)
_LEVELS = (60, 200, 100, 240, 140)
_QH, _QW = 48, 243


def _truth(X, Y):
    """The scene's disparity at hi-res position (X, Y), fractional positions included: constant layers 12, 24
    and 26, a ramp 10 -> 20 down the rows of the third layer and a ramp 16 -> 28 across the columns of the
    fifth."""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    X, Y = np.broadcast_arrays(X, Y)
    layer = np.clip(np.searchsorted(_EDGES, X + 0.5, side="right") - 1, 0, 4)  # the layer of the nearest pixel
    rows = 10.0 + 10.0 * np.clip(Y, 0, _QH - 1) / (_QH - 1)
    cols = 16.0 + 12.0 * (np.clip(X, _EDGES[4], _QW - 1) - _EDGES[4]) / (_QW - 1 - _EDGES[4])
    return np.choose(layer, [np.full(X.shape, 12.0), np.full(X.shape, 24.0), rows, np.full(X.shape, 26.0), cols])


@functools.lru_cache(maxsize=None)
def _scene(factor, seed=11):
    """(d low-res map, g, G, truth at the hi-res pixels) of the quality scene at one factor."""
    rng = np.random.default_rng(seed)
    G = np.zeros((_QH, _QW), np.int32)
    for i in range(5):
        G[:, _EDGES[i]:_EDGES[i + 1]] = _LEVELS[i] + rng.integers(-8, 9, (_QH, _EDGES[i + 1] - _EDGES[i]))
    G = G.astype(np.uint8)
    g = resize_area(G, factor)
    h, Wl = g.shape
    xc = (np.arange(Wl) + 0.5) * _QW / Wl - 0.5                     # each cell's centre in hi-res coordinates
    yc = (np.arange(h) + 0.5) * _QH / h - 0.5
    d = _truth(xc[None, :], yc[:, None]) * (Wl / _QW) + rng.normal(0.0, 0.5 * factor, (h, Wl))
    d = (np.rint(d * 16) / 16).astype(np.float32)
    d[rng.random((h, Wl)) < 0.05] = -1.0
    truth = _truth(np.arange(_QW)[None, :], np.arange(_QH)[:, None]).astype(np.float64)
    return d, g, G, truth


def _measures(out, truth):
    """(edge share, ramp RMS, valid share) in hi-res pixels."""
    with np.errstate(invalid="ignore"):
        valid = (out > 0) & (out < np.inf)
    err = np.where(valid, out.astype(np.float64) - truth, np.inf)
    cols = np.arange(_QW)
    band = np.zeros(_QW, bool)
    for e in _EDGES[1:-1]:
        band |= (cols >= e - 3) & (cols < e + 3)                    # within 3 columns of a depth edge
    share = float(np.mean(np.abs(err[:, band]) <= 1.0))             # valid and within 1 px of the truth
    ramp = np.zeros(_QW, bool)
    for a, b in ((_EDGES[2], _EDGES[3]), (_EDGES[4], _EDGES[5])):
        ramp |= (cols >= a + 4) & (cols < b - 4)                    # 4 columns in from the ramps' edges
    e = err[:, ramp]
    rms = float(np.sqrt(np.mean(e[np.isfinite(e)] ** 2)))
    return share, rms, float(valid.mean())


@pytest.mark.parametrize("factor", [0.5, 2 / 3, 0.4], ids=["0.5", "2_3", "0.4"])
def test_quality_against_nearest_neighbour_upsampling(factor):
    d, g, G, truth = _scene(factor)
    joint, _ = joint_upsample(d, 0, g, G, radius=1, sigma=8, max_diff=1.0)
    select, _ = joint_upsample(d, 0, g, G, radius=1, sigma=8, max_diff=1e-6)
    nearest = nearest_upsample(d, 0, g.shape[1], G.shape)
    js, jr, jv = _measures(joint, truth)
    ns, nr, nv = _measures(nearest, truth)
    _, sr, _ = _measures(select, truth)
    print(f"factor {factor:.3f}: edge share joint {js:.4f} nearest {ns:.4f} (+{js - ns:.4f}); ramp RMS joint {jr:.4f} "
          f"nearest {nr:.4f} (x{jr / nr:.3f}) selection {sr:.4f} (joint x{jr / sr:.3f}); valid joint {jv:.4f} "
          f"nearest {nv:.4f}")
    assert js >= ns + 0.10
    assert jr <= 0.6 * nr
    assert jr <= 0.9 * sr
    assert jv >= 0.999


# --------------------------------------------------------------------------- StereoCore
def test_stereo_core_keys_and_their_messages():
    core = StereoCore()
    p = core.get_sgbm_params()
    assert (p["upsample"], p["upsample_radius"], p["upsample_sigma"], p["upsample_max_diff"]) == ("none", 1, 8, 1.0)
    core.configure_sgbm(upsample="joint", upsample_radius=3, upsample_sigma=64, upsample_max_diff=0.5)
    assert core._upsample_kwargs() == dict(radius=3, sigma=64, max_diff=0.5)
    for kw, key in ((dict(upsample="bilinear"), "'upsample'"), (dict(upsample=None), "'upsample'"),
                    (dict(upsample_radius=0), "'upsample_radius'"), (dict(upsample_radius=4), "'upsample_radius'"),
                    (dict(upsample_radius=1.5), "'upsample_radius'"), (dict(upsample_radius=True), "'upsample_radius'"),
                    (dict(upsample_sigma=0), "'upsample_sigma'"), (dict(upsample_sigma=65), "'upsample_sigma'"),
                    (dict(upsample_max_diff=0), "'upsample_max_diff'"),
                    (dict(upsample_max_diff=float("nan")), "'upsample_max_diff'"),
                    (dict(upsample_max_diff="1"), "'upsample_max_diff'")):
        with pytest.raises(ValueError, match=f"Invalid parameter value for {key}"):
            StereoCore().configure_sgbm(**kw)                       # refused whether the stage is on or off
    with pytest.raises(ValueError, match="Invalid parameter 'upsample_type'"):
        StereoCore().configure_sgbm(upsample_type="joint")


def _stub_core(fast, maps, D=8, **kw):
    """A core on the host path whose matcher returns the uncropped low-resolution ``maps`` one after the other."""
    core = StereoCore(fast_mode=fast)
    it = iter(maps)
    core.compute_disparity = lambda l, r: next(it).copy()
    core.configure_sgbm(num_disp=D, **kw)
    return core


def _frames(n, H=40, W=97, bgr=False, seed=3):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, W, 3) if bgr else (H, W)).astype(np.int32)
    return [np.clip(base + rng.integers(-2, 3, base.shape), 0, 255).astype(np.uint8) for _ in range(n)]


def _low_maps(n, h, Wl, seed=4):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        d = 9.0 + rng.integers(-6, 7, (h, Wl)).astype(np.float32) / 16
        d[rng.random((h, Wl)) < 0.1] = -1.0
        out.append(d.astype(np.float32))
    return out


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("fast", [True, False])
def test_host_path_upsamples_behind_the_tail(fast, bgr):
    D, H, W, s = 8, 40, 97, 0.5
    h, Wl = int(H * s), int(W * s)
    maps = _low_maps(2, h, Wl)
    kw = dict(focal_length=400.0, baseline=0.1, doffs=0.5, max_depth=30.0)
    plain = _stub_core(fast, maps, D, **kw)
    up = _stub_core(fast, maps, D, upsample="joint", upsample_radius=2, upsample_sigma=12, upsample_max_diff=0.75, **kw)
    for i, L in enumerate(_frames(2, H, W, bgr)):
        d0, z0 = plain.estimate_depth(L, L, input_scale=s)
        assert d0.shape == (h, Wl - D) and not plain._upsampled
        d1, z1 = up.estimate_depth(L, L, input_scale=s)
        X0 = upsample_x0(W, Wl, D)
        assert d1.shape == z1.shape == (H, W - X0)
        low = resize_area(L, s)
        low = low if low.ndim == 2 else guide_gray(low)             # resize, then gray
        np.testing.assert_array_equal(up.left_rectified, low)       # left_rectified keeps its meaning
        want, wz = joint_upsample(d0, D, low, L, radius=2, sigma=12, max_diff=0.75, focal_length=400.0, baseline=0.1,
                                  doffs=0.5, eps=0, max_depth=30.0)
        np.testing.assert_array_equal(_bits(d1), _bits(want), err_msg=f"frame {i}")
        np.testing.assert_array_equal(_bits(z1), _bits(wz), err_msg=f"frame {i}")
        assert up.disparity_map is d1 and up.depth_map is z1 and up._upsampled
        assert up.confidence_map is None


def test_host_path_with_the_temporal_filter_over_three_frames():
    D, H, W, s = 8, 36, 100, 0.4
    h, Wl = int(H * s), int(W * s)
    maps = _low_maps(3, h, Wl)
    kw = dict(focal_length=400.0, baseline=0.1)
    plain = _stub_core(True, maps, D, **kw)
    up = _stub_core(True, maps, D, upsample="joint", temporal="recursive", **kw)
    ref = TemporalFilter()
    for i, L in enumerate(_frames(3, H, W)):
        d0, _ = plain.estimate_depth(L, L, input_scale=s)
        d1, z1 = up.estimate_depth(L, L, input_scale=s)
        low = resize_area(L, s)
        filt = ref(d0, low[:, D:])                                  # the filter works, and keeps its state, at low resolution
        want, wz = joint_upsample(filt, D, low, L, focal_length=400.0, baseline=0.1, eps=0)
        np.testing.assert_array_equal(_bits(d1), _bits(want), err_msg=f"frame {i}")
        np.testing.assert_array_equal(_bits(z1), _bits(wz), err_msg=f"frame {i}")
        if i:
            assert (filt != d0).any()


def test_none_and_calls_without_input_scale_are_untouched():
    D, H, W = 8, 20, 64
    maps = _low_maps(4, H // 2, W // 2) + _low_maps(2, H, W)
    L = _frames(1, H, W)[0]
    kw = dict(focal_length=400.0, baseline=0.1)
    a = _stub_core(False, maps[:2] + maps[4:5], D, **kw)
    b = _stub_core(False, maps[:2] + maps[4:5], D, upsample="none", upsample_radius=3, **kw)
    c = _stub_core(False, maps[4:], D, upsample="joint", **kw)
    for _ in range(2):
        ra, rb = a.estimate_depth(L, L, input_scale=0.5), b.estimate_depth(L, L, input_scale=0.5)
        for x, y in zip(ra, rb):
            np.testing.assert_array_equal(_bits(x), _bits(y))       # 'none': the present result bit for bit
    ra = a.estimate_depth(L, L)
    for scale in (None, 1.0):                                       # ignored without input_scale: no full-size frame
        rc = c.estimate_depth(L, L, input_scale=scale)
        assert not c._upsampled and rc[0].shape == (H, W - D)
        if scale is None:
            for x, y in zip(ra, rc):
                np.testing.assert_array_equal(_bits(x), _bits(y))


def test_calibration_and_point_cloud_are_refused():
    D, H, W = 8, 20, 64
    L = _frames(1, H, W)[0]
    K = np.array([[100.0, 0, 16], [0, 100.0, 5], [0, 0, 1]])
    core = _stub_core(True, _low_maps(1, H // 2, W // 2), D, upsample="joint", cam_matrix_L=K, cam_matrix_R=K,
                      baseline=0.1, image_width=W // 2, image_height=H // 2, focal_length=100.0)
    with pytest.raises(ValueError, match="full calibration"):
        core.estimate_depth(L, L, input_scale=0.5)
    core = _stub_core(True, _low_maps(2, H // 2, W // 2), D, upsample="joint", focal_length=100.0, baseline=0.1)
    core.estimate_depth(L, L, input_scale=0.5)
    with pytest.raises(ValueError, match="upsampled frame"):
        core.point_cloud()
    core.configure_sgbm(upsample="none")
    core.estimate_depth(L, L, input_scale=0.5)
    pts, _, _ = core.point_cloud()                                  # a low-resolution frame reprojects as before
    assert pts.shape[1] == 3
