"""fill_holes(method='nearest') on the device (csrc/dsx_nearest.hip: the fused LDS kernel and the
stepwise one) against the host restatement (depthestimation_amd/postprocess.py fill_holes), bit for
bit, through every layer: dsx_fill_nearest_footprint, fill_holes_device, postprocess_full_device,
StereoCore and DepthPipeline.  The CPU tests pin the footprint rule, the host refactor and the
border equivalence (replicated border == skipping the taps outside the image)."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from depthestimation_amd import _dsx
from depthestimation_amd import postprocess as pp
from depthestimation_amd.stereo_core import StereoCore


# --------------------------------------------------------------------------- inputs and references
def _values(rng, shape):
    return (rng.integers(1, 201, shape) / 16).astype(np.float32)


def _dense(shape, density, seed):
    """integers(1, 200) / 16 with ``density`` of the pixels holes, split between 0.0 and -1.0."""
    rng = np.random.default_rng(seed)
    d = _values(rng, shape)
    m = rng.random(shape) < density
    d[m] = np.where(rng.random(int(m.sum())) < 0.5, 0.0, -1.0).astype(np.float32)
    return d


@functools.lru_cache(maxsize=None)
def _maps(shape):
    """name -> map (read-only): three hole densities, all holes, no hole."""
    H, W = shape
    out = {f"dens{int(q * 100)}": _dense(shape, q, 100 * H + W + i) for i, q in enumerate((0.3, 0.7, 0.95))}
    out["allhole"] = _dense(shape, 2.0, 7 * H + W)
    out["nohole"] = _values(np.random.default_rng(H + W), shape)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _host(shape, name, k):
    ref = pp.fill_holes(_maps(shape)[name], method="nearest", kernel_size=k)
    ref.setflags(write=False)
    return ref


def _brute(d, k):
    """The semantics written out: Jacobi iterations, the mask from the input, per-row half-widths,
    taps outside the image skipped."""
    hw = pp.nearest_halfwidths(k)
    r = k // 2
    H, W = d.shape
    mask = d <= 0
    f = d.copy()
    for _ in range(k):
        g = f.copy()
        for y, x in zip(*np.nonzero(mask)):
            m = -np.inf
            for dy in range(-r, r + 1):
                w = hw[dy + r]
                if w < 0 or not 0 <= y + dy < H:
                    continue
                m = max(m, f[y + dy, max(x - w, 0):min(x + w, W - 1) + 1].max())
            g[y, x] = m
        f = g
    return f


def _corridor():
    """A 1-pixel-wide horizontal corridor of 12 holes between walls of 1.0, a valid 50.0 at one end."""
    d = np.ones((9, 20), np.float32)
    d[4, 3:15] = 0.0
    d[4, 2] = 50.0
    return d


# --------------------------------------------------------------------------- CPU
def _c_halfwidths(k, cap=31):
    buf = (ctypes.c_int32 * max(cap, 1))(*([-7] * max(cap, 1)))
    n = _dsx.lib().dsx_fill_nearest_footprint(k, buf, cap)
    return n, list(buf)


def test_footprint_matches_python_helper(dsx_lib_path):
    """dsx_fill_nearest_footprint against postprocess.nearest_halfwidths for every k in 0..31, the
    float64 rule at r = 13 (k = 27: half-width 11 on rows +-5, where dy^2 + dx^2 <= r^2 gives 12), and
    the error returns."""
    for k in range(32):
        n, got = _c_halfwidths(k)
        want = pp.nearest_halfwidths(k)
        assert n == 2 * (k // 2) + 1 == len(want), k
        assert got[:n] == want.tolist(), k
        assert got[n:] == [-7] * (31 - n), k            # nothing written past the rows
        fp = pp.nearest_footprint(k)                      # every row a centred run: the half-widths say it all
        r = k // 2
        assert fp.shape == (n, n)
        for dy in range(-r, r + 1):
            row = np.abs(np.arange(-r, r + 1)) <= want[dy + r]
            np.testing.assert_array_equal(fp[dy + r], row)
    n, got = _c_halfwidths(27)
    assert n == 27 and got[13 - 5] == 11 and got[13 + 5] == 11
    assert int(np.floor(np.sqrt(13 * 13 - 5 * 5))) == 12  # the integer rule differs there
    assert sum(2 * w + 1 for w in got[:27]) == sum(
        2 * int(np.floor(np.sqrt(169 - dy * dy))) + 1 for dy in range(-13, 14)) - 8
    assert _c_halfwidths(5)[1][:5] == [0, 1, 2, 1, 0]
    assert _c_halfwidths(0)[1][:1] == [0] and _c_halfwidths(1)[0] == 1
    lib = _dsx.lib()
    buf = (ctypes.c_int32 * 31)()
    assert lib.dsx_fill_nearest_footprint(-1, buf, 31) == _dsx.DSX_EINVAL
    assert lib.dsx_fill_nearest_footprint(32, buf, 31) == _dsx.DSX_EINVAL
    assert lib.dsx_fill_nearest_footprint(5, buf, 4) == _dsx.DSX_EINVAL
    assert lib.dsx_fill_nearest_footprint(5, None, 31) == _dsx.DSX_EINVAL
    assert lib.dsx_fill_nearest_footprint(5, buf, 5) == 5


@pytest.mark.parametrize("shape", [(7, 13), (23, 31)])
def test_host_nearest_equals_brute_force(shape):
    """fill_holes(method='nearest') against the brute-force restatement that skips out-of-image
    taps: pins the footprint helper's refactor and the border equivalence."""
    for i, k in enumerate((0, 1, 2, 3, 4, 5, 7)):
        for q in (0.3, 0.7, 1.0):
            d = _dense(shape, q, 31 * i + int(q * 10))
            if q < 1.0:
                d[0, 0] = d[-1, -1] = d[0, -1] = 0.0     # holes in the corners
            got = pp.fill_holes(d, method="nearest", kernel_size=k)
            np.testing.assert_array_equal(got, _brute(d, k), err_msg=f"k={k} q={q}")
    if shape == (7, 13):
        np.testing.assert_array_equal(pp.fill_holes(_corridor(), method="nearest", kernel_size=3),
                                      _brute(_corridor(), 3))


def test_stereo_core_fill_method_host_path():
    core = StereoCore(fast_mode=False)
    assert core.get_sgbm_params()["fill_method"] == "inpaint"
    core.configure_sgbm(num_disp=16, block_size=3, hole_filling=True, fill_method="nearest", focal_length=1000,
                        baseline=0.5)
    assert core.get_sgbm_params()["fill_method"] == "nearest"
    with pytest.raises(ValueError, match="Invalid parameter value for 'fill_method': expected 'inpaint' or 'nearest'"):
        StereoCore().configure_sgbm(fill_method="foo")
    rng = np.random.default_rng(3)
    stub = np.full((60, 96), 7.0, np.float32) + (rng.integers(0, 3, (60, 96)) / 16).astype(np.float32)
    stub[rng.random(stub.shape) < 0.1] = -1.0
    stub[20:32, 40:52] = 0.0                               # a hole k = 3 cannot close
    fake = np.zeros((60, 96), np.uint8)
    core.compute_disparity = lambda l, r: stub.copy()
    disp, depth = core._process_pair(fake, fake)
    kw = dict(max_speckle_size=100, max_diff=1.0, outlier_threshold=2.5, apply_outlier_removal=True,
              apply_hole_filling=True)
    want = pp.postprocess_disparity(stub[:, 16:], fill_method="nearest", **kw)
    np.testing.assert_array_equal(disp, want)
    assert depth.shape == want.shape
    assert np.any(want != pp.postprocess_disparity(stub[:, 16:], fill_method="inpaint", **kw))  # the key is live
    assert np.any(want != pp.postprocess_disparity(stub[:, 16:], **dict(kw, apply_hole_filling=False)))


# --------------------------------------------------------------------------- GPU: the stand-alone fill
SHAPES = [(1, 1), (1, 40), (40, 1), (17, 65), (70, 150), (131, 257)]


def _dev_fill(d, k, path, **kw):
    import torch
    from depthestimation_amd.matcher import fill_holes_device
    got = fill_holes_device(torch.from_numpy(np.array(d)).cuda(), radius=k, method="nearest", path=path, **kw)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5])
def test_device_small_k_both_paths(shape, k):
    for name, d in _maps(shape).items():
        ref = _host(shape, name, k)
        for path in (1, 2):
            np.testing.assert_array_equal(_dev_fill(d, k, path), ref, err_msg=f"{name} path={path}")
        if name == "allhole":
            assert ref.max() <= 0 and np.array_equal(ref[d == 0], d[d == 0])
        if name == "nohole":
            np.testing.assert_array_equal(ref, d)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("k", [7, 9, 27])
def test_device_large_k_stepwise_and_auto(shape, k):
    for name in ("dens70", "dens95") + (("allhole", "nohole", "dens30") if k < 27 else ()):
        d, ref = _maps(shape)[name], _host(shape, name, k)
        for path in (2, 0):
            np.testing.assert_array_equal(_dev_fill(d, k, path), ref, err_msg=f"{name} path={path}")


@pytest.mark.gpu
def test_device_auto_equals_forced_paths_and_argument_errors():
    import torch
    from depthestimation_amd.matcher import fill_holes_device
    shape = (131, 257)
    d, ref = _maps(shape)["dens70"], _host(shape, "dens70", 3)
    for path in (0, 1, 2):
        np.testing.assert_array_equal(_dev_fill(d, 3, path), ref)
    x = torch.from_numpy(d.copy()).cuda()
    with pytest.raises(ValueError):
        fill_holes_device(x, radius=31, method="nearest", path=1)       # past the fused limit
    with pytest.raises(ValueError):
        fill_holes_device(x, radius=3, method="nearest", out=x)         # out aliases disp
    with pytest.raises(ValueError):
        fill_holes_device(x, radius=32, method="nearest")
    with pytest.raises(ValueError):
        fill_holes_device(x, radius=3, method="nearest", path=3)
    with pytest.raises(ValueError):
        fill_holes_device(x, radius=3, method="closest")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(x.cpu().numpy(), d)                   # the refused calls wrote nothing


@pytest.mark.gpu
def test_device_unreached_holes_and_pitched_input():
    import torch
    from depthestimation_amd.matcher import fill_holes_device
    d = _values(np.random.default_rng(9), (40, 40))
    d[5:35, 5:35] = 0.0
    ref = pp.fill_holes(d, method="nearest", kernel_size=3)
    assert int((ref[5:35, 5:35] <= 0).sum()) == 576                     # reach k r = 3: 24 x 24 stay
    for path in (1, 2):
        np.testing.assert_array_equal(_dev_fill(d, 3, path), ref)
    wide = _dense((70, 200), 0.7, 77)
    x = torch.from_numpy(wide).cuda()[:, 23:173]                        # in_pitch 200 > W 150
    assert x.stride(0) == 200
    for k, path in ((3, 1), (5, 1), (3, 2), (7, 0)):
        got = fill_holes_device(x, radius=k, method="nearest", path=path)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), pp.fill_holes(wide[:, 23:173], method="nearest", kernel_size=k))


@pytest.mark.gpu
def test_device_jacobi_and_fixed_mask_corridor():
    """The two traps on one map, k = 3 (the cross footprint): Jacobi iterations carry the 50.0 exactly
    3 pixels into the corridor.  An in-place sweep carries it further; a mask recomputed per iteration
    stops after 1 pixel (the walls' 1.0 fills every corridor pixel in the first iteration - the walls
    are its vertical neighbours - so none would be a hole any more).  The other 9 pixels hold 1.0."""
    d = _corridor()
    ref = pp.fill_holes(d, method="nearest", kernel_size=3)
    assert int((ref[4, 3:15] == 50.0).sum()) == 3 and np.all(ref[4, 3:6] == 50.0)
    assert np.all(ref[4, 6:15] == 1.0)
    for path in (1, 2, 0):
        np.testing.assert_array_equal(_dev_fill(d, 3, path), ref)


# --------------------------------------------------------------------------- GPU: the chain
@functools.lru_cache(maxsize=None)
def _chain_map():
    """96 x 160 after the crop: the ramp round((20 + 0.15 x + 0.05 y) * 16) / 16, 10 % scattered -1, zero
    blocks of side 3, 4, 5, 6, 6 and 12 (three on borders); 16 columns in front for the crop."""
    H, W, crop = 96, 160, 16
    yy, xx = np.mgrid[0:H, 0:W]
    d = (np.round((20 + 0.15 * xx + 0.05 * yy) * 16) / 16).astype(np.float32)
    d[np.random.default_rng(11).random(d.shape) < 0.10] = -1.0
    for y, x, s in ((0, 0, 3), (40, 156, 4), (91, 70, 5), (20, 30, 6), (60, 100, 6), (50, 40, 12)):
        d[y:y + s, x:x + s] = 0.0
    full = np.concatenate([np.full((H, crop), 3.0, np.float32), d], axis=1)
    full.setflags(write=False)
    return full, crop


_CHAIN_KW = dict(max_speckle_size=100, max_diff=1.0, outlier_threshold=2.5, apply_outlier_removal=True)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 5])
def test_postprocess_full_device_nearest(k):
    import torch
    from depthestimation_amd.matcher import postprocess_full_device
    full, crop = _chain_map()
    plain = pp.postprocess_disparity(full[:, crop:], apply_hole_filling=False, **_CHAIN_KW)
    ref = pp.postprocess_disparity(full[:, crop:], apply_hole_filling=True, fill_method="nearest", fill_kernel=k,
                                   **_CHAIN_KW)
    assert (plain <= 0).sum() > 200 and np.count_nonzero(ref != plain) > 1000   # the fill is seen
    assert ((ref <= 0).sum() > 0) == (k == 3)                                   # k = 3 leaves holes, k = 5 none
    zref = StereoCore().disparity_to_depth(ref, 700.0, 0.1, 0.0, eps=0.0)
    got, z = postprocess_full_device(torch.from_numpy(np.array(full)).cuda(), crop, focal_length=700.0, baseline=0.1, eps=0.0,
                                     apply_hole_filling=True, fill_method="nearest", fill_kernel=k, **_CHAIN_KW)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), ref)
    np.testing.assert_array_equal(z.cpu().numpy(), zref)
    with pytest.raises(ValueError):
        postprocess_full_device(torch.from_numpy(np.array(full)).cuda(), crop, apply_hole_filling=True, fill_method="foo")


@pytest.mark.gpu
def test_postprocess_full_device_nearest_past_the_fused_limit():
    """fill_kernel 7 takes the stepwise kernel inside the chain (the workspace's idle Telea area)."""
    import torch
    from depthestimation_amd.matcher import postprocess_full_device
    full, crop = _chain_map()
    ref = pp.postprocess_disparity(full[:, crop:], apply_hole_filling=True, fill_method="nearest", fill_kernel=7,
                                   **_CHAIN_KW)
    got, _ = postprocess_full_device(torch.from_numpy(np.array(full)).cuda(), crop, apply_hole_filling=True,
                                     fill_method="nearest", fill_kernel=7, **_CHAIN_KW)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), ref)


# --------------------------------------------------------------------------- GPU: drop-in, streams
def _dropin_core(method):
    core = StereoCore(fast_mode=False)
    core.configure_sgbm(num_disp=64, block_size=5, hole_filling=True, fill_method=method, focal_length=700.0,
                        baseline=0.1)
    return core


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["nearest", "inpaint"])
def test_stereo_core_device_matches_host(method):
    import torch
    from depthestimation_amd.synthetic import stereo_pair
    L, R, _ = stereo_pair(120, 224, 0, 64, seed=52)
    core = _dropin_core(method)
    hd, hz = core._process_pair(L, R)
    if method == "nearest":
        off = _dropin_core("nearest")
        off.configure_sgbm(hole_filling=False)
        assert np.any(hd != off._process_pair(L, R)[0])                 # the fill acts on this frame
    dd, dz = core.process_pair_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    torch.cuda.synchronize()
    assert (core._fill_check is None) == (method == "nearest")          # nothing to time out
    core.check_fill_status()
    np.testing.assert_array_equal(dd.cpu().numpy(), hd)
    np.testing.assert_array_equal(dz.cpu().numpy(), hz)
    # the two-step device branch (a replaced compute_disparity_device) passes the method too
    core.compute_disparity_device = StereoCore.compute_disparity_device.__get__(core)
    dd, dz = core.process_pair_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    torch.cuda.synchronize()
    core.check_fill_status()
    np.testing.assert_array_equal(dd.cpu().numpy(), hd)
    np.testing.assert_array_equal(dz.cpu().numpy(), hz)


@pytest.mark.gpu
def test_three_streams_fill_concurrently():
    """Three streams, a different map each, four rounds with no synchronisation in between: the fill
    holds no state, so every output is exact."""
    import torch
    from depthestimation_amd.matcher import fill_holes_device
    shape = (131, 257)
    names = ("dens30", "dens70", "dens95")
    xs = [torch.from_numpy(_maps(shape)[n].copy()).cuda() for n in names]
    streams = [torch.cuda.Stream() for _ in names]
    torch.cuda.synchronize()
    outs = []
    for rnd in range(4):
        for x, st, path in zip(xs, streams, (1, 2, 0)):
            with torch.cuda.stream(st):
                outs.append(fill_holes_device(x, radius=5, method="nearest", stream=st, path=path if rnd % 2 else 0))
    torch.cuda.synchronize()
    for i, got in enumerate(outs):
        np.testing.assert_array_equal(got.cpu().numpy(), _host(shape, names[i % 3], 5), err_msg=str(i))


@pytest.mark.gpu
def test_depth_pipeline_three_streams_nearest():
    """DepthPipeline with three streams and hole filling: every depth map equals the host chain's and
    no fill-status error is raised."""
    from depthestimation_amd.multigpu import DepthPipeline
    from depthestimation_amd.synthetic import stereo_pair
    core = _dropin_core("nearest")
    frames = [stereo_pair(120, 224, 0, 64, seed=60 + i)[:2] for i in range(6)]
    want = [core._process_pair(L, R)[1] for L, R in frames]
    pipe = DepthPipeline(core, device=0, depth=3, streams=3)
    try:
        done = []
        for i, pair in enumerate(frames):
            done += pipe.push(i, pair)
        done += pipe.drain_all()
    finally:
        pipe.close()
    assert sorted(i for i, _ in done) == list(range(6))
    for i, z in done:
        np.testing.assert_array_equal(z, want[i], err_msg=f"frame {i}")
