"""CPU tests of the point-cloud output: the host restatement (depthestimation_amd/pointcloud.py), the PLY
files, the C-ABI's argument checks and struct layout, and StereoCore's principal point and host path."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from depthestimation_amd import _dsx
from depthestimation_amd import pointcloud as pc
from depthestimation_amd import rectify
from depthestimation_amd.stereo_core import StereoCore
from depthestimation_amd.synthetic import layered_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BAD = np.array([np.nan, np.inf, 0.0, -0.0, -1.0, -np.inf, -np.nan], np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_constant_plane():
    """A constant disparity is a fronto-parallel plane: Z = fB / d everywhere, X steps by exactly s = Z / f."""
    f, B, d = 512.0, 0.25, 8.0
    xyz, valid = pc.reproject_disparity(np.full((5, 9), d, np.float32), f, B, principal_point=(4.0, 2.0))
    assert valid.all()
    Z = np.float32(np.float32(f * B) / np.float32(d))
    s = np.float32(Z / np.float32(f))
    assert (xyz[..., 2] == Z).all()
    assert (np.diff(xyz[..., 0], axis=1) == s).all() and (np.diff(xyz[..., 1], axis=0) == s).all()
    assert (xyz[2, 4] == (0.0, 0.0, Z)).all()                      # the principal point looks down the z axis
    assert xyz[0, 0, 0] < 0 and xyz[0, 0, 1] < 0                  # x right, y down


def test_against_the_homogeneous_q_form():
    """[x, y, d, 1] Q^T in float64, Q from stereo_rectify for a pure-x baseline.  The float32 form has five
    roundings of 2^-24 each (fB, Z, s, the product, and d's own sum with doffs = 0 is exact): about 3e-7,
    so rtol 1e-5 leaves a factor of 30.  cx, cy are float32 numbers and W, H are even, so x - cx is exact
    and never 0."""
    H, W, f, B = 48, 64, 700.0, 0.12
    K = np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1.0]])
    Q = rectify.stereo_rectify(K, np.zeros(5), K, np.zeros(5), (W, H), np.eye(3), np.array([-B, 0.0, 0.0]))[4]
    rng = np.random.default_rng(5)
    d = rng.uniform(0.5, 120.0, (H, W)).astype(np.float32)
    fq, Bq, cx, cy = Q[2, 3], 1.0 / Q[3, 2], -Q[0, 3], -Q[1, 3]
    assert Q[3, 3] == 0 and Bq > 0
    xyz, valid = pc.reproject_disparity(d, fq, Bq, principal_point=(cx, cy), eps=0.0)
    assert valid.all()
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    hom = np.stack([xs, ys, d.astype(np.float64), np.ones((H, W))], -1) @ Q.T
    want = hom[..., :3] / hom[..., 3:]
    np.testing.assert_allclose(xyz.astype(np.float64), want, rtol=1e-5, atol=0)


def test_invalid_values_are_dropped():
    f, B = 400.0, 0.5                                             # fB = 200
    d = np.concatenate([_BAD, np.array([1.0, 2.0, 3.0, 4.0, 100.0], np.float32)])[None, :]
    xyz, valid = pc.reproject_disparity(d, f, B, eps=2.0, max_depth=60.0)
    # adj <= eps drops 1 and 2; Z = 200 / 3 > max_depth drops 3; 4 (Z 50) and 100 (Z 2) stay
    np.testing.assert_array_equal(valid[0], [False] * 7 + [False, False, False, True, True])
    assert np.isnan(xyz[~valid]).all() and (_bits(xyz[~valid]) == 0x7FC00000).all()
    assert np.isfinite(xyz[valid]).all()
    # without a bound everything above eps stays; -1 with doffs 2 is a valid adj of 1
    assert pc.reproject_disparity(d, f, B, eps=2.0)[1].sum() == 3
    assert pc.reproject_disparity(np.array([[-1.0]], np.float32), f, B, doffs=2.0)[1].all()
    # a negative baseline puts everything behind the camera
    assert not pc.reproject_disparity(d, f, -B)[1].any()


def _map(H, W, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(8, 2000, (H, W)).astype(np.float32) / 16.0
    m = rng.random((H, W)) < 0.3
    d[m] = rng.choice(_BAD, int(m.sum()))
    return d


def test_point_cloud_is_the_masked_organized_map():
    H, W, x0 = 13, 37, 5
    d = _map(H, W, 1)
    rng = np.random.default_rng(2)
    bgr = rng.integers(0, 256, (H, x0 + W, 3), dtype=np.uint8)
    kw = dict(focal_length=333.25, baseline=0.193, doffs=0.5, eps=1.0, max_depth=40.0, x0=x0)
    xyz, valid = pc.reproject_disparity(d, **kw)
    pts, col, idx = pc.point_cloud(d, colors=bgr, **kw)
    assert 0 < len(pts) < H * W and pts.dtype == np.float32 and col.dtype == np.uint8 and idx.dtype == np.int32
    np.testing.assert_array_equal(_bits(pts), _bits(xyz[valid]))
    np.testing.assert_array_equal(idx, np.flatnonzero(valid))
    np.testing.assert_array_equal(col, bgr[:, x0:, ::-1][valid])
    gray = bgr[..., 0].copy()
    np.testing.assert_array_equal(pc.point_cloud(d, colors=gray, **kw)[1], np.repeat(gray[:, x0:][valid][:, None], 3, 1))
    assert pc.point_cloud(d, **kw)[1] is None
    with pytest.raises(ValueError):
        pc.point_cloud(d, colors=bgr[:, x0:], **kw)               # the cropped image is not the convention


def test_crop_offset():
    """The cloud of a map cropped at column k with x0 = k is the uncropped map's cloud restricted to x >= k."""
    H, W, k = 9, 40, 16
    d = _map(H, W, 3)
    kw = dict(focal_length=500.0, baseline=0.1, principal_point=(17.25, 3.5), eps=0.0)
    full, vfull = pc.reproject_disparity(d, x0=0, **kw)
    crop, vcrop = pc.reproject_disparity(d[:, k:], x0=k, **kw)
    np.testing.assert_array_equal(vcrop, vfull[:, k:])
    np.testing.assert_array_equal(_bits(crop), _bits(full[:, k:]))
    # the default principal point is the centre of the UNCROPPED image
    a = pc.reproject_disparity(d[:, k:], 500.0, 0.1, x0=k)[0]
    b = pc.reproject_disparity(d[:, k:], 500.0, 0.1, principal_point=((W - 1) / 2, (H - 1) / 2), x0=k)[0]
    np.testing.assert_array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("n", [0, 1, 5])
@pytest.mark.parametrize("with_colors", [False, True])
def test_ply_round_trip(tmp_path, n, with_colors):
    rng = np.random.default_rng(n)
    pts = rng.normal(size=(n, 3)).astype(np.float32)
    col = rng.integers(0, 256, (n, 3), dtype=np.uint8) if with_colors else None
    path = tmp_path / "c.ply"
    pc.write_ply(path, pts, col)
    raw = path.read_bytes()
    head = raw[:raw.index(b"end_header\n")].decode().split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    assert head[3:6] == ["property float x", "property float y", "property float z"]
    assert (head[6:9] == ["property uchar red", "property uchar green", "property uchar blue"]) == with_colors
    assert len(raw) - raw.index(b"end_header\n") - 11 == n * (15 if with_colors else 12)
    got, gcol = pc.read_ply(path)
    assert got.shape == (n, 3) and got.dtype == np.float32
    np.testing.assert_array_equal(_bits(got), _bits(pts))
    if with_colors:
        np.testing.assert_array_equal(gcol, col)
    else:
        assert gcol is None


# --------------------------------------------------------------------------- the C-ABI without a device
def _cloud(**kw):
    c = _dsx.DsxCloud()
    c.focal_length, c.baseline, c.cx, c.cy, c.eps = 500.0, 0.1, 10.0, 5.0, 1e-6
    for k, v in kw.items():
        setattr(c, k, v)
    return c


@pytest.mark.parametrize("kw", [
    dict(focal_length=0.0), dict(focal_length=-1.0), dict(focal_length=float("inf")), dict(focal_length=float("nan")),
    dict(baseline=0.0), dict(baseline=float("nan")), dict(baseline=float("inf")), dict(cx=float("nan")),
    dict(cy=float("inf")), dict(doffs=float("nan")), dict(eps=float("inf")), dict(x0=-1), dict(has_max_depth=2),
    dict(has_max_depth=1, max_depth=0.0), dict(has_max_depth=1, max_depth=float("nan")),
])
def test_check_cloud_rejections(kw):
    lib = _dsx.lib()
    assert lib.dsx_check_cloud(ctypes.byref(_cloud(**kw))) == _dsx.DSX_EINVAL
    assert _dsx.last_error()
    f, B = kw.get("focal_length", 500.0), kw.get("baseline", 0.1)
    if set(kw) <= {"focal_length", "baseline", "cx", "cy", "doffs", "eps", "x0"}:   # the host applies the same rules
        with pytest.raises(ValueError):
            pc.reproject_disparity(np.ones((2, 2), np.float32), f, B, principal_point=(kw.get("cx", 1.0), kw.get("cy", 1.0)),
                                   doffs=kw.get("doffs", 0.0), eps=kw.get("eps", 0.0), x0=kw.get("x0", 0))


def test_check_cloud_accepts():
    lib = _dsx.lib()
    for kw in (dict(), dict(baseline=-0.1), dict(eps=-16.0), dict(has_max_depth=1, max_depth=5.0), dict(x0=512),
               dict(has_max_depth=0, max_depth=float("nan"))):
        assert lib.dsx_check_cloud(ctypes.byref(_cloud(**kw))) == _dsx.DSX_OK, kw
    c = _dsx.make_cloud(721.5, 0.54, 600.0, 180.0, doffs=None, eps=0, max_depth=80.0, x0=128)
    assert (c.has_max_depth, c.x0, c.max_depth, c.doffs) == (1, 128, 80.0, 0.0)
    with pytest.raises(ValueError):
        _dsx.make_cloud(None, 0.54, 1.0, 1.0)


def test_null_and_short_arguments_are_errors_not_crashes():
    lib = _dsx.lib()
    c = ctypes.byref(_cloud())
    E = _dsx.DSX_EINVAL
    assert lib.dsx_check_cloud(None) == E
    assert lib.dsx_reproject_device(None, 4, 4, 4, c, None, None) == E          # NULL map
    assert lib.dsx_reproject_device(0x1000, 4, 4, 4, None, 0x1000, None) == E    # NULL parameters
    assert lib.dsx_reproject_device(0x1000, 4, 4, 3, c, 0x1000, None) == E       # pitch < W
    assert lib.dsx_reproject_device(0x1000, 4, 4, 4, c, None, None) == E         # NULL output
    assert lib.dsx_reproject_device(0x1000, -1, 4, 4, c, 0x1000, None) == E
    assert lib.dsx_reproject_device(0x1000, 65536, 65536, 65536, c, 0x1000, None) == E   # H * W past int32

    def cloud(disp=0x1000, H=4, W=4, pitch=4, cc=c, color=None, cpitch=0, ch=0, pts=0x1000, cols=None, idx=None, cap=16,
              count=0x1000, ws=0x1000, wsb=4):
        return lib.dsx_point_cloud_device(disp, H, W, pitch, cc, color, cpitch, ch, pts, cols, idx, cap, count, ws, wsb, None)
    assert cloud(disp=None) == E and cloud(cc=None) == E and cloud(pitch=3) == E and cloud(count=None) == E
    assert cloud(pts=None) == E and cloud(cap=-1) == E and cloud(ch=2) == E
    assert cloud(ws=None) == E and cloud(wsb=3) == E and cloud(H=-1) == E
    assert cloud(cols=0x1000) == E                                # colours wanted, no image
    assert cloud(cols=0x1000, color=0x1000, ch=3, cpitch=11) == E  # colour pitch below (x0 + W) * channels
    assert cloud(cols=0x1000, color=0x1000, ch=0, cpitch=12) == E
    assert lib.dsx_point_cloud_workspace_bytes(0, 5) == 0 and lib.dsx_point_cloud_workspace_bytes(-1, 5) == 0
    T = _dsx.CLOUD_TILE
    assert lib.dsx_point_cloud_workspace_bytes(1, T) == 4 and lib.dsx_point_cloud_workspace_bytes(1, T + 1) == 8
    assert lib.dsx_point_cloud_workspace_bytes(1080, 1792) == 4 * ((1080 * 1792 + T - 1) // T)


def test_cloud_struct_layout_matches_c(tmp_path):
    """dsx_cloud as gcc lays it out equals the ctypes mirror (size and every offset); the tile constant too."""
    fields = [f for f, _ in _dsx.DsxCloud._fields_]
    c = tmp_path / "probe.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsx.h"\nint main(void){printf("%d %zu", DSX_CLOUD_TILE, sizeof(dsx_cloud));'
                 + "".join(f'printf(" %zu", offsetof(dsx_cloud, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [_dsx.CLOUD_TILE, ctypes.sizeof(_dsx.DsxCloud)] + [getattr(_dsx.DsxCloud, f).offset for f in fields]
    assert got == want


# --------------------------------------------------------------------------- StereoCore
def test_stereo_core_principal_point_key():
    core = StereoCore(downscale_factor=0.5)
    assert core.get_sgbm_params()["principal_point"] is None
    assert core.resolve_principal_point(10, 21) == (10.0, 4.5)     # the image centre
    core.configure_sgbm(principal_point=(640.0, 361.0), focal_length=1000.0)
    p = core.get_sgbm_params()
    assert p["principal_point"] == (320.0, 180.5) and p["focal_length"] == 500.0   # scaled alike
    assert core.resolve_principal_point(10, 21) == (320.0, 180.5)
    core.configure_sgbm(principal_point=None)
    assert core.resolve_principal_point(10, 21) == (10.0, 4.5)
    for bad in ((1.0,), (1.0, 2.0, 3.0), (1.0, float("nan")), (float("inf"), 1.0), "ab", 5.0, (True, 1.0)):
        with pytest.raises(ValueError):
            StereoCore().configure_sgbm(principal_point=bad)


def test_stereo_core_principal_point_from_the_calibration(monkeypatch):
    W, H, B = 64, 48, 0.2
    K = np.array([[300.0, 0, 30.25], [0, 300.0, 25.5], [0, 0, 1.0]])
    core = StereoCore()
    core.configure_sgbm(cam_matrix_L=K, cam_matrix_R=K, baseline=B, image_width=W, image_height=H, num_disp=16)
    P1 = rectify.stereo_rectify(K, np.zeros(5), K, np.zeros(5), (W, H), np.eye(3), np.array([-B, 0.0, 0.0]),
                                zero_disparity=True, alpha=1.0)[2]
    calls = []
    import depthestimation_amd.stereo_core as sc
    real = sc.rectified_principal_point
    monkeypatch.setattr(sc, "rectified_principal_point", lambda *a: calls.append(1) or real(*a))
    assert core.resolve_principal_point(H, W) == (P1[0, 2], P1[1, 2])
    assert core.resolve_principal_point(H, W) == (P1[0, 2], P1[1, 2]) and len(calls) == 1   # once per calibration
    core.configure_sgbm(baseline=0.3)
    core.resolve_principal_point(H, W)
    assert len(calls) == 2
    core.configure_sgbm(principal_point=(1.0, 2.0))                # the key wins
    assert core.resolve_principal_point(H, W) == (1.0, 2.0)
    # the maps' dict is what it was
    maps = rectify.compute_maps(K, K, B, W, H, alpha=1.0)
    assert sorted(maps) == ["map1_L", "map1_R", "map2_L", "map2_R"]


def test_stereo_core_point_cloud_host_path():
    D, H, W = 16, 24, 96
    L, R, gt = layered_pair(H, W, D, seed=3, disparities=(3, 7, 4), levels=(60, 200, 110))
    core = StereoCore(fast_mode=True)
    with pytest.raises(ValueError):
        core.point_cloud()                                         # no frame yet
    stub = np.where(np.arange(W)[None, :] % 7 == 0, -1.0, gt.astype(np.float32) + 0.25).astype(np.float32)
    core.compute_disparity = lambda l, r: stub.copy()              # the host path, no device
    core.configure_sgbm(num_disp=D)
    core.estimate_depth(L, R)
    with pytest.raises(ValueError):
        core.point_cloud()                                         # no focal length / baseline
    core.configure_sgbm(focal_length=333.3, baseline=0.193, max_depth=12.0, doffs=0.125)
    disp, depth = core.estimate_depth(L, R)
    pts, col, idx = core.point_cloud()
    want = pc.point_cloud(disp, 333.3, 0.193, principal_point=((W - 1) / 2, (H - 1) / 2), doffs=0.125, eps=0,
                          max_depth=12.0, x0=D, colors=L)
    assert len(pts) > 100
    for g, w in zip((pts, col, idx), want):
        np.testing.assert_array_equal(g, w)
    # Z carries the depth map's bits wherever that depth is below max_depth, and those are all the points
    below = depth.ravel() < np.float32(12.0)
    assert 0 < below.sum() < below.size and (depth.ravel() == np.float32(12.0)).any()
    np.testing.assert_array_equal(idx, np.flatnonzero(below))
    np.testing.assert_array_equal(_bits(pts[:, 2]), _bits(depth.ravel()[idx]))
    # colours: gray replicated from the left rectified image, cropped
    np.testing.assert_array_equal(col[:, 0], L[:, D:].ravel()[idx])
    bgr = np.stack([L, L // 2, L // 3], -1)
    np.testing.assert_array_equal(core.point_cloud(colors=bgr)[1], bgr[:, D:, ::-1].reshape(-1, 3)[idx])
    core.configure_sgbm(principal_point=(50.0, 10.0))
    np.testing.assert_array_equal(core.point_cloud()[0], pc.point_cloud(
        disp, 333.3, 0.193, principal_point=(50.0, 10.0), doffs=0.125, eps=0, max_depth=12.0, x0=D)[0])


def test_estimator_point_cloud_and_ply(tmp_path):
    from depthestimation_amd.StereoDepthEstimator import StereoDepthEstimator
    D, H, W = 16, 24, 96
    L, R, gt = layered_pair(H, W, D, seed=3, disparities=(3, 7, 4), levels=(60, 200, 110))
    est = StereoDepthEstimator()
    est.left_source, est.right_source = L, R
    est.core.compute_disparity = lambda l, r: gt.astype(np.float32)
    est.configure_sgbm(num_disp=D, focal_length=200.0, baseline=0.1)
    est.estimate_depth()
    pts, col, idx = est.point_cloud()
    n = est.save_point_cloud(tmp_path / "scene.ply")
    got, gcol = pc.read_ply(tmp_path / "scene.ply")
    assert n == len(pts) > 0
    np.testing.assert_array_equal(_bits(got), _bits(pts))
    np.testing.assert_array_equal(gcol, col)
