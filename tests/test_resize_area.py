"""CPU tests of the device area downscale's host side: the table builder of libdsx
(dsx_resize_area_table) against the numpy restatement (input.resize_area_table), both against Pillow's
BOX resampling (input.resize_area, the contract), argument validation of both entry points, and the
facades' ``device_downscale`` switch.  No test here needs a GPU."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from depthestimation_amd import _dsx
from depthestimation_amd.input import resize_area, resize_area_table

SHAPES = [(37, 53, 3), (48, 64), (31, 100, 3), (9, 7, 3), (64, 96, 3)]
FACTORS = [0.5, 0.25, 0.75, 0.6, 0.33, 0.9, 0.1, 0.45]


def _axis_pairs():
    pairs = {(1920, 960), (1080, 720), (7, 1)}
    for shp in SHAPES:
        for f in FACTORS:
            for n in shp[:2]:
                if int(n * f) >= 1:
                    pairs.add((n, int(n * f)))
    return sorted(pairs)


def _c_table(in_size, out_size):
    arr = [(ctypes.c_int32 * out_size)() for _ in range(3)]
    rc = _dsx.lib().dsx_resize_area_table(in_size, out_size, *arr)
    assert rc == _dsx.DSX_OK, _dsx.last_error()
    return tuple(np.ctypeslib.as_array(a).copy() for a in arr)


def test_c_table_equals_numpy_restatement():
    pairs = _axis_pairs()
    assert len(pairs) > 40
    for i, o in pairs:
        got, ref = _c_table(i, o), resize_area_table(i, o)
        for g, r, name in zip(got, ref, ("start", "count", "coef")):
            np.testing.assert_array_equal(g, r, err_msg=f"{name} of ({i}, {o})")
        start, count, _ = got
        assert count.min() >= 1 and start.min() >= 0 and (start + count).max() <= i
        # windows move forward with the output index and never overlap
        assert np.all(start[1:] >= (start + count)[:-1])


def test_identity_axis_table():
    start, count, coef = _c_table(17, 17)
    np.testing.assert_array_equal(start, np.arange(17))
    assert np.all(count == 1) and np.all(coef == 1 << 22)


def _pass(img, table, axis):
    """One BOX pass along ``axis`` of a u8 array, by the (start, count, coef) table, in integers."""
    start, count, coef = table
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    csum = np.concatenate([np.zeros((1,) + src.shape[1:], np.int64), np.cumsum(src, 0)])
    s = csum[start + count] - csum[start]
    k = coef.astype(np.int64).reshape((-1,) + (1,) * (src.ndim - 1))
    out = np.minimum(255, ((1 << 21) + k * s) >> 22).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def two_pass(img, factor, table=_c_table):
    H, W = img.shape[:2]
    Wo, Ho = int(W * factor), int(H * factor)
    h = _pass(img, table(W, Wo), 1)      # horizontal first, rounded to u8
    return _pass(h, table(H, Ho), 0)     # vertical on the u8 values


@pytest.mark.parametrize("shape", SHAPES)
def test_two_pass_tables_equal_pillow(shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    for f in FACTORS:
        if int(shape[0] * f) < 1 or int(shape[1] * f) < 1:
            continue
        ref = resize_area(img, f)
        np.testing.assert_array_equal(two_pass(img, f), ref, err_msg=f"{shape} x {f} (C tables)")
        np.testing.assert_array_equal(two_pass(img, f, resize_area_table), ref, err_msg=f"{shape} x {f} (numpy tables)")
    white = np.full(shape, 255, np.uint8)
    np.testing.assert_array_equal(two_pass(white, 0.6), resize_area(white, 0.6))


def test_table_argument_errors():
    L = _dsx.lib()
    a = (ctypes.c_int32 * 8)()
    assert L.dsx_resize_area_table(8, 0, a, a, a) == _dsx.DSX_EINVAL
    assert L.dsx_resize_area_table(8, -3, a, a, a) == _dsx.DSX_EINVAL
    assert L.dsx_resize_area_table(4, 8, a, a, a) == _dsx.DSX_EINVAL
    assert L.dsx_resize_area_table(8, 4, None, a, a) == _dsx.DSX_EINVAL
    assert L.dsx_resize_area_table(8, 4, a, None, a) == _dsx.DSX_EINVAL
    assert L.dsx_resize_area_table(8, 4, a, a, None) == _dsx.DSX_EINVAL
    assert _dsx.last_error()
    with pytest.raises(ValueError):
        resize_area_table(4, 8)
    with pytest.raises(ValueError):
        resize_area_table(4, 0)


@pytest.mark.parametrize("args", [
    # (img, Hs, Ws, stride, channels, Ho, Wo, gray_out, out, out_stride)
    (None, 8, 8, 24, 3, 4, 4, 0, 1, 12),        # null image
    (1, 8, 8, 24, 3, 4, 4, 0, None, 12),        # null output
    (1, 8, 8, 24, 2, 4, 4, 0, 1, 12),           # channels not in {1, 3}
    (1, 8, 8, 32, 4, 4, 4, 0, 1, 16),
    (1, 8, 8, 8, 1, 4, 4, 1, 1, 4),             # gray_out with one channel
    (1, 8, 8, 24, 3, 9, 4, 0, 1, 12),           # Ho > Hs
    (1, 8, 8, 24, 3, 4, 9, 0, 1, 27),           # Wo > Ws
    (1, 0, 8, 24, 3, 4, 4, 0, 1, 12),           # sizes < 1
    (1, 8, 0, 24, 3, 4, 4, 0, 1, 12),
    (1, 8, 8, 24, 3, 0, 4, 0, 1, 12),
    (1, 8, 8, 24, 3, 4, 0, 0, 1, 12),
    (1, 8, 8, 23, 3, 4, 4, 0, 1, 12),           # source stride below a row
    (1, 8, 8, 24, 3, 4, 4, 0, 1, 11),           # output stride below a row
])
def test_device_entry_argument_errors_before_any_hip_call(args):
    """Rejected on the arguments alone: the bogus non-null pointers are never touched, and no device is
    needed (this runs on hosts without one)."""
    assert _dsx.lib().dsx_resize_area_device(*args, None) == _dsx.DSX_EINVAL
    assert _dsx.last_error()


def test_resize_area_device_needs_device_tensors():
    from depthestimation_amd.input import resize_area_device
    with pytest.raises(ValueError):
        resize_area_device(np.zeros((8, 8, 3), np.uint8), 0.5)


class _StubCapture:
    seen = []

    def __init__(self, left, right, downscale_factor=1.0, **kw):
        _StubCapture.seen.append(downscale_factor)

    def start(self):
        pass

    def read(self):
        return None

    def stop(self):
        pass


@pytest.mark.parametrize("device_downscale,expect", [(False, 0.5), (True, 1.0)])
def test_video_facade_hands_the_factor_to_capture_or_keeps_frames_full_size(monkeypatch, device_downscale, expect):
    import importlib
    mod = importlib.import_module("depthestimation_amd.StereoDepthEstimatorVideo")
    _StubCapture.seen = []
    streamed = []

    def stub_stream(left, right, downscale_factor=1.0, **kw):
        streamed.append(downscale_factor)
        return iter(())

    monkeypatch.setattr(mod, "ThreadedStereoCapture", _StubCapture)
    monkeypatch.setattr(mod, "stereo_stream", stub_stream)
    src = np.zeros((2, 8, 8, 3), np.uint8)
    kw = dict(device_downscale=True) if device_downscale else {}
    for threaded in (True, False):
        v = mod.StereoDepthEstimatorVideo(src, src, downscale_factor=0.5, use_threading=threaded, target_fps=0, **kw)
        assert v.device_downscale is device_downscale
        assert list(v._frames()) == []
    assert _StubCapture.seen == [expect] and streamed == [expect]


def test_video_facade_passes_input_scale_to_the_core(monkeypatch):
    import importlib
    mod = importlib.import_module("depthestimation_amd.StereoDepthEstimatorVideo")
    frames = np.arange(2 * 8 * 8 * 3, dtype=np.uint8).reshape(2, 8, 8, 3)
    for dd, want_shape, want_kw in ((False, (4, 4, 3), {}), (True, (8, 8, 3), {"input_scale": 0.5})):
        v = mod.StereoDepthEstimatorVideo(frames, frames, downscale_factor=0.5, use_threading=False, target_fps=0,
                                          device_downscale=dd)
        v.configure_sgbm(num_disp=64, focal_length=100.0, baseline=0.1)  # estimate_depth re-applies the parameters
        calls = []
        v.core.estimate_depth = lambda l, r, **kw: (calls.append((l.shape, kw)), (None, None))[1]
        assert list(v.estimate_depth()) == [None, None]
        assert calls == [(want_shape, want_kw)] * 2


def test_still_facade_device_downscale_loads_full_size(tmp_path):
    from PIL import Image

    from depthestimation_amd import StereoDepthEstimator
    img = np.random.default_rng(5).integers(0, 256, (12, 16, 3), dtype=np.uint8)
    p = str(tmp_path / "a.png")
    Image.fromarray(img).save(p)
    host = StereoDepthEstimator(p, p, downscale_factor=0.5)
    dev = StereoDepthEstimator(p, p, downscale_factor=0.5, device_downscale=True)
    assert host.left_source.shape == (6, 8, 3) and dev.left_source.shape == (12, 16, 3)
    calls = []
    dev.core.estimate_depth = lambda l, r, **kw: (calls.append((l.shape, kw)), (None, None))[1]
    host.core.estimate_depth = lambda l, r, **kw: (calls.append((l.shape, kw)), (None, None))[1]
    dev.estimate_depth()
    host.estimate_depth()
    assert calls == [((12, 16, 3), {"input_scale": 0.5}), ((6, 8, 3), {})]
