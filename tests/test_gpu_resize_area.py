"""GPU tests of the device area downscale (dsx_resize.hip, input.resize_area_device) and of every layer
that can run it: 0 differing bytes against the host ``resize_area`` (Pillow BOX), on both forms of the
kernel, and bit-equal disparity / depth through StereoCore, DepthPipeline and the video facade."""
from __future__ import annotations

import numpy as np
import pytest

from depthestimation_amd import StereoDepthEstimatorVideo
from depthestimation_amd.input import resize_area, resize_area_device
from depthestimation_amd.rectify import to_grayscale_bgr
from depthestimation_amd.stereo_core import StereoCore
from depthestimation_amd.synthetic import stereo_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# (shape, factor): factors from 0.5 up run the kernel form that loads a window's <= 2 x 2 taps at once,
# smaller ones the looping form.  70 x 700 x 3 is wider and taller than one block's 64 x 4 output tile
# in both (tile seams); then one-row / one-column outputs, 10 x 10 windows, and the identity.
CASES = [
    ((37, 53, 3), 0.6), ((37, 53, 3), 0.33), ((37, 53, 3), 0.9),
    ((48, 64), 0.5),
    ((9, 7, 3), 0.45),
    ((64, 96, 3), 0.75), ((64, 96, 3), 0.1),
    ((70, 700, 3), 0.5), ((70, 700, 3), 0.37),
    ((5, 40, 3), 0.3), ((40, 5), 0.3), ((300, 9), 0.5),
    ((40, 900, 3), 0.1),
    ((33, 47, 3), 1.0),
]
_images = {}


def _image(shape):
    if shape not in _images:
        _images[shape] = np.random.default_rng(sum(shape) * 7 + len(shape)).integers(0, 256, shape, dtype=np.uint8)
    return _images[shape]


def _run(img, factor, gray=False, **kw):
    import torch
    out = resize_area_device(torch.from_numpy(img).cuda() if isinstance(img, np.ndarray) else img, factor,
                             gray=gray, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("shape,factor", CASES)
def test_resize_area_device_equals_host(shape, factor):
    img = _image(shape)
    ref = resize_area(img, factor)
    got = _run(img, factor)
    assert got.shape == ref.shape and got.dtype == np.uint8
    assert int(np.count_nonzero(got != ref)) == 0
    if img.ndim == 3:
        g = _run(img, factor, gray=True)
        assert g.shape == ref.shape[:2]
        assert int(np.count_nonzero(g != to_grayscale_bgr(ref))) == 0


def test_all_255_image():
    img = np.full((37, 53, 3), 255, np.uint8)
    for f in (0.6, 0.33):
        ref = resize_area(img, f)
        assert int(np.count_nonzero(_run(img, f) != ref)) == 0
        assert int(np.count_nonzero(_run(img, f, gray=True) != to_grayscale_bgr(ref))) == 0


def test_strided_view_of_a_wider_tensor():
    """Row stride 210 and a base 225 bytes into the allocation: no row starts on a dword."""
    import torch
    wide = _image((42, 70, 3))
    view = torch.from_numpy(wide).cuda()[1:38, 5:58]
    assert not view.is_contiguous() and view.data_ptr() % 4 == 1
    ref = resize_area(np.ascontiguousarray(wide[1:38, 5:58]), 0.6)
    assert int(np.count_nonzero(_run(view, 0.6) != ref)) == 0
    assert int(np.count_nonzero(_run(view, 0.6, gray=True) != to_grayscale_bgr(ref))) == 0
    ref = resize_area(np.ascontiguousarray(wide[1:38, 5:58]), 0.33)  # the looping form
    assert int(np.count_nonzero(_run(view, 0.33) != ref)) == 0
    gview = torch.from_numpy(np.ascontiguousarray(wide[..., 1])).cuda()[3:40, 2:67]
    gref = resize_area(np.ascontiguousarray(wide[3:40, 2:67, 1]), 0.45)
    assert int(np.count_nonzero(_run(gview, 0.45) != gref)) == 0


def test_tiny_factor_large_windows():
    """70 x 7000 x 3 at 0.015: one output row, windows of 70 rows x 66 or 67 columns."""
    img = _image((70, 7000, 3))
    ref = resize_area(img, 0.015)
    assert ref.shape == (1, 105, 3)
    assert int(np.count_nonzero(_run(img, 0.015) != ref)) == 0
    assert int(np.count_nonzero(_run(img, 0.015, gray=True) != to_grayscale_bgr(ref))) == 0


def test_out_argument_and_errors():
    import torch
    img = torch.from_numpy(_image((37, 53, 3))).cuda()
    out = torch.zeros((22, 31, 3), dtype=torch.uint8, device="cuda")
    assert resize_area_device(img, 0.6, out=out) is out
    torch.cuda.synchronize()
    assert int(np.count_nonzero(out.cpu().numpy() != resize_area(_image((37, 53, 3)), 0.6))) == 0
    with pytest.raises(ValueError):
        resize_area_device(img, 0.6, out=torch.zeros((22, 31), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        resize_area_device(img, 0.01)        # a zero dimension, as Pillow raises
    with pytest.raises(ValueError):
        resize_area_device(img[..., 0], 0.5)  # element stride 3
    with pytest.raises(ValueError):
        resize_area_device(torch.from_numpy(_image((48, 64))).cuda(), 0.5, gray=True)


def test_two_streams_two_shapes_alternately_and_more_shapes_than_the_cache_keeps():
    import torch
    a, b = _image((70, 700, 3)), _image((64, 96, 3))
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ra, rb = resize_area(a, 0.37), to_grayscale_bgr(resize_area(b, 0.75))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for _ in range(4):
        with torch.cuda.stream(s1):
            outs.append((resize_area_device(da, 0.37, stream=s1), ra))
        with torch.cuda.stream(s2):
            outs.append((resize_area_device(db, 0.75, gray=True, stream=s2), rb))
    torch.cuda.synchronize()
    for got, ref in outs:
        assert int(np.count_nonzero(got.cpu().numpy() != ref)) == 0
    # ten more shapes push the first two out of the 8-entry cache; they are rebuilt on the next use
    base = _image((64, 96, 3))
    for i in range(10):
        sub = np.ascontiguousarray(base[: 40 + i, : 60 + 2 * i])
        assert int(np.count_nonzero(_run(sub, 0.5) != resize_area(sub, 0.5))) == 0
    with torch.cuda.stream(s2):
        again = resize_area_device(da, 0.37, stream=s2)
    torch.cuda.synchronize()
    assert int(np.count_nonzero(again.cpu().numpy() != ra)) == 0


# -- the layers above -----------------------------------------------------------------------------

H, W = 128, 192


def _bgr_pair(seed):
    Lg, Rg, _ = stereo_pair(H, W, 0, 64, seed=seed)
    L = np.stack([Lg, np.roll(Lg, 1, 0), Lg // 2], 2).astype(np.uint8)
    R = np.stack([Rg, np.roll(Rg, 1, 0), Rg // 2], 2).astype(np.uint8)
    return L, R


def _calib(w, h):
    from depthestimation_amd.rectify import rodrigues
    K1 = np.array([[0.9 * w, 0, w / 2 + 3.5], [0, 0.9 * w, h / 2 - 2.0], [0, 0, 1]])
    K2 = np.array([[0.92 * w, 0, w / 2 - 4.0], [0, 0.92 * w, h / 2 + 1.5], [0, 0, 1]])
    return dict(cam_matrix_L=K1, cam_matrix_R=K2, dist_coeff_L=np.array([-0.12, 0.05, 0.001, -0.0005, 0.0]),
                dist_coeff_R=np.array([-0.1, 0.03, -0.0008, 0.0004, 0.0]), rotation=rodrigues([0.01, -0.02, 0.005]),
                translation=np.array([-0.12, 0.002, 0.001]), baseline=0.12, image_width=w, image_height=h)


@pytest.mark.parametrize("calibrated", [False, True])
def test_stereo_core_input_scale_equals_host_downscale(calibrated):
    L, R = _bgr_pair(51)
    core = StereoCore(fast_mode=True)
    if calibrated:
        core.configure_sgbm(num_disp=32, block_size=5, focal_length=180.0, **_calib(W // 2, H // 2))
    else:
        core.configure_sgbm(num_disp=32, block_size=5, focal_length=400.0, baseline=0.1)
    hd, hz = core.estimate_depth(resize_area(L, 0.5), resize_area(R, 0.5))
    hl, hr = core.left_rectified.copy(), core.right_rectified.copy()
    dd, dz = core.estimate_depth(L, R, input_scale=0.5)
    assert hd.shape == (H // 2, W // 2 - 32)
    np.testing.assert_array_equal(dd, hd)
    np.testing.assert_array_equal(dz, hz)
    np.testing.assert_array_equal(core.left_rectified, hl)
    np.testing.assert_array_equal(core.right_rectified, hr)
    # gray frames take the one-channel kernel
    gd, gz = core.estimate_depth(resize_area(L[..., 1].copy(), 0.5), resize_area(R[..., 1].copy(), 0.5))
    sd, sz = core.estimate_depth(L[..., 1].copy(), R[..., 1].copy(), input_scale=0.5)
    np.testing.assert_array_equal(sd, gd)
    np.testing.assert_array_equal(sz, gz)


def test_stereo_core_input_scale_host_fallback_on_calibrated_size_mismatch():
    """The calibration names another size than the downscaled frames: the device pipeline does not
    apply, the host resize_area and the host path run - the same result as handing those frames in."""
    L, R = _bgr_pair(52)
    core = StereoCore(fast_mode=True)
    core.configure_sgbm(num_disp=32, block_size=5, focal_length=180.0, **_calib(W // 2 + 8, H // 2 + 4))
    assert not core._device_pipeline_ok(L, R, 0.5)
    hd, hz = core.estimate_depth(resize_area(L, 0.5), resize_area(R, 0.5))
    dd, dz = core.estimate_depth(L, R, input_scale=0.5)
    np.testing.assert_array_equal(dd, hd)
    np.testing.assert_array_equal(dz, hz)


def test_depth_pipeline_input_scale_equals_host_downscaled_pipeline():
    from depthestimation_amd.multigpu import DepthPipeline
    frames = [_bgr_pair(60 + i) for i in range(4)]
    core = StereoCore(fast_mode=True)
    core.configure_sgbm(num_disp=32, block_size=5, focal_length=400.0, baseline=0.1)

    def run(pipe, pairs):
        out = {}
        for i, p in enumerate(pairs):
            out.update(pipe.push(i, p))
        out.update(pipe.drain_all())
        pipe.close()
        return [out[i] for i in range(len(pairs))]

    ref = run(DepthPipeline(core, 0), [(resize_area(l, 0.5), resize_area(r, 0.5)) for l, r in frames])
    got = run(DepthPipeline(core, 0, input_scale=0.5), frames)
    assert len(got) == 4 and got[0].shape == (H // 2, W // 2 - 32)
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g, r)


@pytest.mark.parametrize("use_threading,devices", [(True, None), (False, None), (True, [0])])
def test_video_facade_device_downscale_equals_host_downscale(use_threading, devices):
    frames = [_bgr_pair(70 + i) for i in range(4)]
    lefts, rights = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])

    def run(dd):
        v = StereoDepthEstimatorVideo(lefts, rights, downscale_factor=0.5, fast_mode=True, target_fps=0,
                                      use_threading=use_threading, devices=devices, device_downscale=dd)
        v.configure_sgbm(num_disp=128, block_size=5, focal_length=800.0, baseline=0.1)  # 32 after the two scalings
        return list(v.estimate_depth())

    ref, got = run(False), run(True)
    assert len(ref) == len(got) == 4 and ref[0].shape == (H // 2, W // 2 - 32)
    for g, r in zip(got, ref):
        np.testing.assert_array_equal(g, r)
