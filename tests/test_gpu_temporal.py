"""GPU tests of the temporal disparity filter (csrc/dsx_temporal.hip): the device equals the host restatement
(depthestimation_amd/temporal.py) bit for bit on EVERY frame of a sequence - outputs and depth - over the tile
and lane edges, both load paths, every radius, pitched and in-place maps, resets, shape changes and streams; and
StereoCore / DepthPipeline with the filter equal the sequential host path."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from depthestimation_amd import _dsx
from depthestimation_amd.stereo_core import StereoCore
from depthestimation_amd.synthetic import layered_pair
from depthestimation_amd.temporal import TemporalFilter

pytestmark = pytest.mark.gpu

_TW, _TH = _dsx.TEMPORAL_TILE   # pixels of a row and rows per block (csrc/dsx_temporal.hip kTW, kTH)
_KW = dict(focal_length=517.3, baseline=0.193, doffs=0.25, eps=0.5, max_depth=90.0)
_BAD = np.array([np.nan, np.inf, 0.0, -0.0, -1.0, -np.inf], np.float32)
_FRAMES = 6


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _depth(out):
    return StereoCore.disparity_to_depth(None, out, _KW["focal_length"], _KW["baseline"], _KW["doffs"],
                                         eps=_KW["eps"], max_depth=_KW["max_depth"])


@functools.lru_cache(maxsize=None)
def _sequence(H, W, frames=_FRAMES, seed=0, calm=False):
    """Maps on the 1/16 grid around a fixed base (steps within and beyond max_diff, every kind of invalid value)
    and guides of which about 80 % of the pixels keep their level to within 2 from frame to frame (``calm``:
    99 %, and 8 % holes instead of 15 %, so that long runs of agreement and of holds occur)."""
    rng = np.random.default_rng(1000 * H + W + seed)
    base = rng.integers(16, 640, (H, W)).astype(np.float32) / 16
    g = rng.integers(0, 256, (H, W)).astype(np.int32)
    out = []
    for _ in range(frames):
        d = base + rng.integers(-12, 13, (H, W)).astype(np.float32) / 16
        d[rng.random((H, W)) < 0.05] += 3.0
        m = rng.random((H, W)) < (0.08 if calm else 0.15)
        d[m] = rng.choice(_BAD, int(m.sum()))
        move = rng.random((H, W)) > (0.99 if calm else 0.8)
        g = np.clip(np.where(move, rng.integers(0, 256, (H, W)), g + rng.integers(-2, 3, (H, W))), 0, 255)
        out.append((d.astype(np.float32), g.astype(np.uint8)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _reference(H, W, kw=(), frames=_FRAMES, seed=0, calm=False):
    """The host restatement over ``_sequence``: per frame (out, depth).  Computed once, shared, never changed."""
    f = TemporalFilter(**dict(kw))
    res = []
    for d, g in _sequence(H, W, frames, seed, calm):
        o = f(d, g)
        z = _depth(o)
        o.setflags(write=False)
        z.setflags(write=False)
        res.append((o, z))
    return tuple(res)


def _assert_frame(got, want, what):
    (go, gz), (wo, wz) = got, want
    np.testing.assert_array_equal(_bits(go.cpu().numpy()), _bits(wo), err_msg=f"{what}: disparity")
    np.testing.assert_array_equal(_bits(gz.cpu().numpy()), _bits(wz), err_msg=f"{what}: depth")


def _filter(**kw):
    from depthestimation_amd.matcher import TemporalFilterDevice
    return TemporalFilterDevice(device=0, **kw)


def _run_sequence(H, W, kw=(), frames=_FRAMES, seed=0, calm=False):
    import torch
    f = _filter(**dict(kw))
    try:
        for i, ((d, g), want) in enumerate(zip(_sequence(H, W, frames, seed, calm),
                                                  _reference(H, W, kw, frames, seed, calm))):
            got = f.run(torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda(), **_KW)
            torch.cuda.synchronize()
            _assert_frame(got, want, f"{H}x{W} {dict(kw)} frame {i}")
    finally:
        f.close()


_SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (7, 3), (5, 1001),
           (_TH - 1, _TW - 1), (_TH, _TW), (_TH + 1, _TW + 1),          # one short of, equal to, one over the tile
           (_TH + 1, _TW - 4), (_TH - 1, _TW + 4), (2 * _TH + 3, 2 * _TW + 8)]   # 16-byte rows around the tile


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_host_on_every_frame(shape, radius):
    _run_sequence(*shape, kw=(("motion_radius", radius),))


@pytest.mark.parametrize("kw", [
    dict(max_age=1, hold=0), dict(max_age=4, hold=2), dict(max_age=64, hold=255), dict(max_age=64, hold=0, motion_radius=2),
    dict(max_age=1, hold=255, motion_radius=0), dict(motion_threshold=0), dict(motion_threshold=255, motion_radius=2),
    dict(max_diff=0.3125, motion_threshold=40),
], ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_parameters(kw):
    _run_sequence(19, 300, kw=tuple(sorted(kw.items())), frames=8)


def test_long_sequence_reaches_every_age():
    """12 frames with max_age 8 on a mostly static guide: ages up to the cap and holds of several frames."""
    kw = (("hold", 3), ("max_age", 8), ("motion_threshold", 12))
    ref = TemporalFilter(**dict(kw))
    for d, g in _sequence(12, 132, 12, 3, True):
        ref(d, g)
    assert ref.n.max() == 8 and ref.h.max() >= 2
    _run_sequence(12, 132, kw=kw, frames=12, seed=3, calm=True)


@pytest.mark.parametrize("shape", [(9, 260), (6, 129), (11, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pitched_maps_and_guides_at_odd_addresses(shape):
    """The map is a pitched view 12 bytes into its rows, the guide a pitched view at an odd address - what
    ``left[:, num_disp:]`` is for an odd crop; the outputs are views of nothing (contiguous)."""
    import torch
    H, W = shape
    f = _filter()
    try:
        for i, ((d, g), want) in enumerate(zip(_sequence(H, W), _reference(H, W))):
            db = torch.full((H, W + 5), float("nan"), dtype=torch.float32, device="cuda")
            gb = torch.full((H, W + 7), 255, dtype=torch.uint8, device="cuda")
            dv, gv = db[:, 3:3 + W], gb[:, 1 + 2 * (i % 2):1 + 2 * (i % 2) + W]
            dv.copy_(torch.from_numpy(d))
            gv.copy_(torch.from_numpy(g))
            assert gv.data_ptr() % 2 == 1 and dv.data_ptr() % 16 != 0
            got = f.run(dv, gv, **_KW)
            torch.cuda.synchronize()
            _assert_frame(got, want, f"pitched {H}x{W} frame {i}")
    finally:
        f.close()


@pytest.mark.parametrize("shape", [(9, 260), (10, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_in_place(shape):
    import torch
    H, W = shape
    f = _filter(motion_radius=2)
    kw = (("motion_radius", 2),)
    try:
        for i, ((d, g), want) in enumerate(zip(_sequence(H, W), _reference(H, W, kw))):
            t = torch.from_numpy(d).cuda()
            out, z = f.run(t, torch.from_numpy(g).cuda(), out=t, **_KW)
            torch.cuda.synchronize()
            assert out is t
            _assert_frame((out, z), want, f"in place {H}x{W} frame {i}")
    finally:
        f.close()


def test_without_depth_and_state_bytes():
    import torch
    H, W = 9, 260
    f = _filter()
    try:
        for (d, g), (wo, _) in zip(_sequence(H, W), _reference(H, W)):
            out, z = f.run(torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda())
            assert z is None
            np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(wo))
        assert f.state_bytes() == H * 260 * 8 + 65 * 4              # S 4, n 1, h 1, two guides; the gain table
    finally:
        f.close()


def test_reset_in_mid_sequence_and_shape_change_and_back():
    import torch
    H, W = 10, 140
    seq = _sequence(H, W, 8, 1)
    other = _sequence(7, 90, 2, 1)
    f, ref = _filter(), TemporalFilter()

    def step(d, g, what):
        want = ref(d, g)
        got = f.run(torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda(), **_KW)
        torch.cuda.synchronize()
        _assert_frame(got, (want, _depth(want)), what)

    try:
        for i in range(3):
            step(*seq[i], f"frame {i}")
        f.reset()
        ref.reset()
        for i in range(3, 5):
            step(*seq[i], f"after the reset, frame {i}")
        for i in range(2):
            step(*other[i], f"other shape, frame {i}")              # reallocates and resets
        for i in range(5, 8):
            step(*seq[i], f"back, frame {i}")                       # a first frame again, not the old state
        f.set_params(max_age=2, motion_radius=0)                     # new parameters reset the state too
        ref = TemporalFilter(max_age=2, motion_radius=0)
        for i in range(3):
            step(*seq[i], f"new parameters, frame {i}")
    finally:
        f.close()


def test_two_filters_on_two_streams_stay_independent():
    import torch
    A, B = (12, 260), (9, 131)
    fa, fb = _filter(), _filter(motion_radius=2)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ia = [(torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda()) for d, g in _sequence(*A)]
    ib = [(torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda()) for d, g in _sequence(*B)]
    oa = [(torch.empty(A, device="cuda"), torch.empty(A, device="cuda")) for _ in ia]
    ob = [(torch.empty(B, device="cuda"), torch.empty(B, device="cuda")) for _ in ib]
    torch.cuda.synchronize()
    try:
        for i in range(_FRAMES):
            fa.run(*ia[i], out=oa[i][0], out_depth=oa[i][1], stream=sa, **_KW)
            fb.run(*ib[i], out=ob[i][0], out_depth=ob[i][1], stream=sb, **_KW)
        torch.cuda.synchronize()
        for i in range(_FRAMES):
            _assert_frame(oa[i], _reference(*A)[i], f"filter A frame {i}")
            _assert_frame(ob[i], _reference(*B, (("motion_radius", 2),))[i], f"filter B frame {i}")
    finally:
        fa.close()
        fb.close()


def test_one_filter_driven_alternately_from_two_streams():
    """Frame i on stream i mod 2 with no host wait between the calls: the library's event chain orders the
    launches, so the result is the sequential host's."""
    import torch
    H, W, n = 24, 516, 8
    f = _filter()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    inp = [(torch.from_numpy(d).cuda(), torch.from_numpy(g).cuda()) for d, g in _sequence(H, W, n, 2)]
    outs = [(torch.empty((H, W), device="cuda"), torch.empty((H, W), device="cuda")) for _ in inp]
    torch.cuda.synchronize()
    try:
        for i in range(n):
            f.run(*inp[i], out=outs[i][0], out_depth=outs[i][1], stream=streams[i % 2], **_KW)
        torch.cuda.synchronize()
        for i in range(n):
            _assert_frame(outs[i], _reference(H, W, (), n, 2)[i], f"frame {i}")
    finally:
        f.close()


def test_wrapper_refuses_bad_tensors():
    import torch
    f = _filter()
    d = torch.zeros((4, 8), device="cuda")
    g = torch.zeros((4, 8), dtype=torch.uint8, device="cuda")
    try:
        for bad in ((d.double(), g), (d, g.float()), (d, g[:, :7]), (d.cpu(), g.cpu()), (d[:, ::2], g[:, ::2])):
            with pytest.raises(ValueError):
                f.run(*bad)
        with pytest.raises(ValueError):
            f.run(d, g, out=torch.zeros((4, 9), device="cuda"))
        with pytest.raises(ValueError):
            f.run(d[:, :4], g[:, :4], out=d[:, :4])                 # a pitched output
    finally:
        f.close()


# --------------------------------------------------------------------------- StereoCore and the pipeline
_D = 16
_CAL = dict(num_disp=_D, block_size=5, focal_length=420.0, baseline=0.12, max_depth=40.0)


@functools.lru_cache(maxsize=None)
def _video(n=6, H=40, W=96):
    """A static layered scene seen ``n`` times with sensor noise of +-1 grey level."""
    L, R, _ = layered_pair(H, W, _D, seed=9, disparities=(3, 9, 5), levels=(70, 190, 120))
    rng = np.random.default_rng(17)
    frames = []
    for _ in range(n):
        a = np.clip(L.astype(np.int32) + rng.integers(-1, 2, L.shape), 0, 255).astype(np.uint8)
        b = np.clip(R.astype(np.int32) + rng.integers(-1, 2, R.shape), 0, 255).astype(np.uint8)
        frames.append((a, b))
    return tuple(frames)


def _host_sequence(fast, n, **kw):
    """The sequential host path (_process_pair: the host chain and the restatement) over ``_video``."""
    core = StereoCore(fast_mode=fast)
    core.configure_sgbm(temporal="recursive", **_CAL, **kw)
    res = []
    for L, R in _video(n):
        d, z = core._process_pair(L, R)
        res.append((d.copy(), z.copy()))
    core.sgbm.close()
    return res


@pytest.mark.parametrize("fast,kw", [
    (True, {}), (False, {}), (False, dict(refine="wmedian", refine_radius=3)), (True, dict(confidence_threshold=40)),
    (False, dict(confidence=True, hole_filling=True, fill_method="nearest")),
], ids=["fast", "full", "wmedian", "conf-threshold", "conf-map-nearest"])
def test_estimate_depth_device_equals_host_path(fast, kw):
    want = _host_sequence(fast, 6, **kw)
    plain = StereoCore(fast_mode=fast)
    plain.configure_sgbm(**_CAL, **kw)
    core = StereoCore(fast_mode=fast)
    core.configure_sgbm(temporal="recursive", **_CAL, **kw)
    changed = 0
    for i, ((L, R), (wd, wz)) in enumerate(zip(_video(6), want)):
        d, z = core.estimate_depth(L, R)                             # host arrays in, the device pipeline inside
        np.testing.assert_array_equal(_bits(d), _bits(wd), err_msg=f"frame {i}: disparity")
        np.testing.assert_array_equal(_bits(z), _bits(wz), err_msg=f"frame {i}: depth")
        np.testing.assert_array_equal(_bits(z), _bits(core.disparity_to_depth(d, 420.0, 0.12, 0.0, eps=0, max_depth=40.0)))
        assert core.disparity_map is d and core.depth_map is z
        changed += int((d != plain.estimate_depth(L, R)[0]).sum())
    assert changed > 0                                               # the filter did something
    idx = core.point_cloud()[2]                                      # the cloud is the filtered map's
    np.testing.assert_array_equal(idx, np.flatnonzero(z.ravel() < np.float32(40.0)))
    core.reset_temporal()
    d, _ = core.estimate_depth(*_video(6)[0])
    np.testing.assert_array_equal(_bits(d), _bits(want[0][0]))      # a first frame again
    core.sgbm.close()
    plain.sgbm.close()


def test_depth_pipeline_equals_sequential_host_path():
    from depthestimation_amd.multigpu import DepthPipeline
    n = 8
    want = _host_sequence(True, n)
    core = StereoCore(fast_mode=True)
    core.configure_sgbm(temporal="recursive", **_CAL)
    pipe = DepthPipeline(core, 0, depth=3, streams=2)
    assert len({id(c._temporal) for c in pipe.cores}) == 1 and len(pipe.cores) == 3
    done = []
    for i, pair in enumerate(_video(n)):
        done += pipe.push(i, pair)
    done += pipe.drain_all()
    pipe.close()
    assert [i for i, _ in done] == list(range(n))
    for i, z in done:
        np.testing.assert_array_equal(_bits(z), _bits(want[i][1]), err_msg=f"frame {i}")
    core.sgbm.close()


@pytest.mark.parametrize("fast", [True, False])
def test_filter_off_runs_exactly_the_parents_kernels(fast):
    """With 'temporal': 'none' a frame runs the launches of the matcher's drop-in call and nothing else: the
    handle names the same kernels, the same number of times, as a direct call of that function; and the
    filter, when on, adds no kernel of the handle's either (its one launch belongs to the filter object)."""
    import torch
    from depthestimation_amd.matcher import HipBlockMatcher
    L, R = _video(6)[0]
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()

    def names(core):
        core.sgbm = HipBlockMatcher(**dict(core.sgbm.params, timing=True))
        for _ in range(2):
            core.process_pair_device(tl, tr)
        torch.cuda.synchronize()
        kt = {k: v[1] for k, v in core.sgbm.kernel_times().items() if v[1]}
        core.sgbm.close()
        return kt

    m = HipBlockMatcher(num_disp=_D, block_size=5, timing=True)
    for _ in range(2):
        m.process_pair_device(tl, tr, fast_mode=fast, max_speckle_size=100, max_diff=1.0, apply_outlier_removal=True,
                              outlier_threshold=2.5, outlier_kernel=5, focal_length=420.0, baseline=0.12, eps=0,
                              max_depth=40.0)
    torch.cuda.synchronize()
    parent = {k: v[1] for k, v in m.kernel_times().items() if v[1]}
    m.close()
    off = StereoCore(fast_mode=fast)
    off.configure_sgbm(**_CAL)
    assert off.get_sgbm_params()["temporal"] == "none" and off._temporal is None
    assert names(off) == parent and parent
    on = StereoCore(fast_mode=fast)
    on.configure_sgbm(temporal="recursive", **_CAL)
    assert names(on) == parent
