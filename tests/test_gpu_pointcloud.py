"""GPU tests of the point-cloud output (csrc/dsx_cloud.hip): the device equals the host restatement
(depthestimation_amd/pointcloud.py) bit for bit - the organized map, and the compact cloud with its count,
order, colours and indices - over the tile and wave edges, pitched views, capacities and streams."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from depthestimation_amd import _dsx
from depthestimation_amd import pointcloud as pc
from depthestimation_amd.stereo_core import StereoCore
from depthestimation_amd.synthetic import layered_pair

pytestmark = pytest.mark.gpu

_T = 2048           # pixels per block of the compaction (csrc/dsx_cloud.hip kCT = DSX_CLOUD_TILE)
_SCAN = 1024        # threads of the scan block (kScanThreads): more tiles than this and its loop runs
_KW = dict(focal_length=517.3, baseline=0.193, doffs=0.25, eps=0.5, max_depth=90.0)
_BAD = np.array([np.nan, np.inf, 0.0, -0.0, -1.0, -np.inf, -np.nan], np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _inputs(H, W, seed, density="mixed", x0=0):
    """A k / 16 map with arbitrary normal-range floats and every kind of invalid value (magnitudes e^+-40: with
    fB near 100 neither Z nor X leaves the normal range), and an uncropped BGR image."""
    rng = np.random.default_rng(seed)
    d = rng.integers(16, 4000, (H, W)).astype(np.float32) / 16.0
    m = rng.random((H, W)) < 0.1
    # "mixed" reaches below eps and beyond max_depth; the other densities keep every such value valid
    d[m] = np.exp(rng.uniform(-40 if density == "mixed" else 1, 40, int(m.sum()))).astype(np.float32)
    if density == "mixed":                                         # about 75 % valid
        m = rng.random((H, W)) < 0.22
        d[m] = rng.choice(_BAD, int(m.sum()))
    elif density != "all":
        keep = d.copy()
        d[...] = rng.choice(_BAD, (H, W))
        if density == "last":
            d[-1, -1] = keep[-1, -1]
        elif density == "first":
            d[0, 0] = keep[0, 0]
        else:
            assert density == "none"
    bgr = rng.integers(0, 256, (H, x0 + W, 3), dtype=np.uint8)
    return d, bgr


def _assert_cloud(got, want, what=""):
    (gp, gc, gi), (wp, wc, wi) = got, want
    assert len(gp) == len(wp), f"{what}: {len(gp)} points, the host has {len(wp)}"
    np.testing.assert_array_equal(_bits(gp.cpu().numpy()), _bits(wp), err_msg=what)
    np.testing.assert_array_equal(gi.cpu().numpy(), wi, err_msg=what)
    if wc is None:
        assert gc is None
    else:
        np.testing.assert_array_equal(gc.cpu().numpy(), wc, err_msg=what)


def test_tile_constant():
    assert _T == _dsx.CLOUD_TILE


_SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (7, 3),           # below a wave, a wave, one over
           (1, _T - 1), (1, _T), (1, _T + 1),                    # one short of the tile, exact, one over
           (5, 1001),                                            # W % 4 = 1, the tile boundary in mid-row
           (3, 256 + 64 + 1)]                                    # a round, a wave and one pixel per row


@pytest.mark.parametrize("shape", _SHAPES)
@pytest.mark.parametrize("density", ["mixed", "all", "none", "last", "first"])
def test_device_equals_host(shape, density):
    import torch
    from depthestimation_amd.matcher import point_cloud_device, reproject_device
    H, W = shape
    x0 = 5
    d, bgr = _inputs(H, W, seed=H * 10000 + W, density=density, x0=x0)
    dd, dc = torch.from_numpy(d).cuda(), torch.from_numpy(bgr).cuda()
    kw = dict(_KW, x0=x0)
    want = pc.point_cloud(d, colors=bgr, **kw)
    n = {"all": H * W, "none": 0, "last": 1, "first": 1}.get(density)
    assert n is None or len(want[0]) == n
    _assert_cloud(point_cloud_device(dd, colors=dc, **kw), want, f"{shape} {density} bgr")
    gray = np.ascontiguousarray(bgr[..., 1])
    _assert_cloud(point_cloud_device(dd, colors=torch.from_numpy(gray).cuda(), **kw),
                  pc.point_cloud(d, colors=gray, **kw), f"{shape} {density} gray")
    _assert_cloud(point_cloud_device(dd, **kw), (want[0], None, want[2]), f"{shape} {density} no colours")
    xyz = reproject_device(dd, **kw).cpu().numpy()
    np.testing.assert_array_equal(_bits(xyz), _bits(pc.reproject_disparity(d, **kw)[0]))   # the NaN pattern included


def test_more_tiles_than_scan_threads():
    """1025 x 2049 pixels are 1026 tiles: the scan's second chunk carries the first's total."""
    import torch
    from depthestimation_amd.matcher import point_cloud_device
    H, W = 1025, 2049
    assert (H * W + _T - 1) // _T > _SCAN
    d, _ = _inputs(H, W, seed=9, x0=0)
    gray = np.random.default_rng(1).integers(0, 256, (H, W), dtype=np.uint8)
    kw = dict(_KW, principal_point=(1000.5, 500.25))
    got = point_cloud_device(torch.from_numpy(d).cuda(), colors=torch.from_numpy(gray).cuda(), **kw)
    _assert_cloud(got, pc.point_cloud(d, colors=gray, **kw))


def test_pitched_views_and_odd_colour_address():
    import torch
    from depthestimation_amd.matcher import point_cloud_device, reproject_device
    H, W, x0 = 21, 131, 7
    d, bgr = _inputs(H, W, seed=4, x0=x0)
    big = torch.full((H, W + 5), 3.0, dtype=torch.float32, device="cuda")       # the pad is valid: it must not be read
    big[:, :W] = torch.from_numpy(d).cuda()
    dview = big[:, :W]
    Wf = x0 + W
    raw = torch.full((H * (Wf + 3) * 3 + 1,), 255, dtype=torch.uint8, device="cuda")
    cview = raw[1:].view(H, Wf + 3, 3)[:, :Wf]                                   # BGR rows 3 (Wf + 3) apart, odd address
    cview.copy_(torch.from_numpy(bgr).cuda())
    graw = torch.full((H * (Wf + 2) + 1,), 255, dtype=torch.uint8, device="cuda")
    gview = graw[1:].view(H, Wf + 2)[:, :Wf]
    gview.copy_(torch.from_numpy(np.ascontiguousarray(bgr[..., 0])).cuda())
    assert dview.stride(0) == W + 5 and cview.data_ptr() % 2 == 1 and gview.data_ptr() % 2 == 1
    kw = dict(_KW, x0=x0)
    _assert_cloud(point_cloud_device(dview, colors=cview, **kw), pc.point_cloud(d, colors=bgr, **kw), "bgr")
    _assert_cloud(point_cloud_device(dview, colors=gview, **kw), pc.point_cloud(d, colors=bgr[..., 0], **kw), "gray")
    np.testing.assert_array_equal(_bits(reproject_device(dview, **kw).cpu().numpy()),
                                  _bits(pc.reproject_disparity(d, **kw)[0]))


@pytest.mark.parametrize("cap_of", ["N-1", "1", "0"])
def test_capacity(cap_of):
    """The first cap points are written, the count is the true N, nothing at or past cap is touched."""
    import torch
    from depthestimation_amd.matcher import point_cloud_device
    H, W = 3, _T + 77                                             # four tiles; the cut falls inside one
    d, bgr = _inputs(H, W, seed=11)
    dd, dc = torch.from_numpy(d).cuda(), torch.from_numpy(bgr).cuda()
    wp, wc, wi = pc.point_cloud(d, colors=bgr, **_KW)
    N = len(wp)
    cap = {"N-1": N - 1, "1": 1, "0": 0}[cap_of]
    assert N > _T
    room = N + 64
    P = torch.full((room, 3), -7.0, dtype=torch.float32, device="cuda")
    C = torch.full((room, 3), 0xA5, dtype=torch.uint8, device="cuda")
    I = torch.full((room,), -7, dtype=torch.int32, device="cuda")
    pts, col, idx, count = point_cloud_device(dd, colors=dc, capacity=cap, out_points=P[:cap], out_colors=C[:cap],
                                              out_index=I[:cap], sync=False, **_KW)
    assert pts.shape == (cap, 3) and col.shape == (cap, 3) and idx.shape == (cap,) and count.dtype == torch.int32
    torch.cuda.synchronize()
    assert int(count.item()) == N
    np.testing.assert_array_equal(_bits(P[:cap].cpu().numpy()), _bits(wp[:cap]))
    np.testing.assert_array_equal(C[:cap].cpu().numpy(), wc[:cap])
    np.testing.assert_array_equal(I[:cap].cpu().numpy(), wi[:cap])
    assert bool((P[cap:] == -7.0).all()) and bool((C[cap:] == 0xA5).all()) and bool((I[cap:] == -7).all())
    with pytest.raises(ValueError, match="capacity"):
        point_cloud_device(dd, colors=dc, capacity=cap, **_KW)     # sync=True reads the count and refuses
    # without colours (the wrapper still writes its own index tensor) the same cut holds
    P.fill_(-7.0)
    pts, col, idx, count = point_cloud_device(dd, capacity=cap, out_points=P[:cap], sync=False, **_KW)
    torch.cuda.synchronize()
    assert col is None and int(count.item()) == N
    np.testing.assert_array_equal(_bits(P[:cap].cpu().numpy()), _bits(wp[:cap]))
    np.testing.assert_array_equal(idx.cpu().numpy(), wi[:cap])
    assert bool((P[cap:] == -7.0).all())
    # without an index (d_index NULL), with colours: the same cut in points and colours
    P.fill_(-7.0)
    C.fill_(0xA5)
    pts, col, idx, count = point_cloud_device(dd, colors=dc, capacity=cap, out_points=P[:cap], out_colors=C[:cap],
                                              out_index=False, sync=False, **_KW)
    torch.cuda.synchronize()
    assert idx is None and int(count.item()) == N
    np.testing.assert_array_equal(_bits(P[:cap].cpu().numpy()), _bits(wp[:cap]))
    np.testing.assert_array_equal(C[:cap].cpu().numpy(), wc[:cap])
    assert bool((P[cap:] == -7.0).all()) and bool((C[cap:] == 0xA5).all())


@pytest.mark.parametrize("colours", ["bgr", "gray", "none"])
@pytest.mark.parametrize("shape", [(7, 3), (1, _T + 1), (5, 1001)])
def test_c_abi_without_index(shape, colours):
    """dsx_point_cloud_device with d_index NULL and room for every point: points and colours equal the host's bit
    for bit, the count is N; then the same through the wrapper (out_index=False)."""
    import torch
    from depthestimation_amd.matcher import point_cloud_device
    H, W = shape
    x0 = 3
    d, bgr = _inputs(H, W, seed=H * 77 + W, x0=x0)
    img = {"bgr": bgr, "gray": np.ascontiguousarray(bgr[..., 2]), "none": None}[colours]
    kw = dict(_KW, x0=x0)
    wp, wc, _ = pc.point_cloud(d, colors=img, **kw)
    N = len(wp)
    assert 0 < N < H * W
    dd = torch.from_numpy(d).cuda()
    dc = None if img is None else torch.from_numpy(img).cuda()
    ch = 0 if img is None else (3 if img.ndim == 3 else 1)
    L = _dsx.lib()
    c = _dsx.make_cloud(kw["focal_length"], kw["baseline"], (x0 + W - 1) / 2, (H - 1) / 2, kw["doffs"], kw["eps"],
                        kw["max_depth"], x0)
    nbytes = L.dsx_point_cloud_workspace_bytes(H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    P = torch.full((H * W + 8, 3), -7.0, dtype=torch.float32, device="cuda")
    C = torch.full((H * W + 8, 3), 0xA5, dtype=torch.uint8, device="cuda")
    n = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    rc = L.dsx_point_cloud_device(dd.data_ptr(), H, W, W, ctypes.byref(c), dc.data_ptr() if ch else None,
                                  dc.stride(0) if ch else 0, ch, P.data_ptr(), C.data_ptr() if ch else None, None,
                                  H * W, n.data_ptr(), ws.data_ptr(), nbytes, None)
    assert rc == _dsx.DSX_OK, _dsx.last_error()
    torch.cuda.synchronize()
    assert int(n.item()) == N
    np.testing.assert_array_equal(_bits(P[:N].cpu().numpy()), _bits(wp))
    assert bool((P[N:] == -7.0).all())
    if ch:
        np.testing.assert_array_equal(C[:N].cpu().numpy(), wc)
    assert bool((C[N if ch else 0:] == 0xA5).all())
    pts, col, idx = point_cloud_device(dd, colors=dc, out_index=False, **kw)
    assert idx is None and len(pts) == N
    np.testing.assert_array_equal(_bits(pts.cpu().numpy()), _bits(wp))
    if ch:
        np.testing.assert_array_equal(col.cpu().numpy(), wc)
    else:
        assert col is None


def test_stream_and_shared_workspace():
    """A non-default stream; two C-ABI calls back to back on one workspace and one count word each."""
    import torch
    from depthestimation_amd.matcher import point_cloud_device
    H, W = 9, 1000
    d1, bgr = _inputs(H, W, seed=21)
    d2, _ = _inputs(H, W, seed=22)
    t1, t2, tc = torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda(), torch.from_numpy(bgr).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    _assert_cloud(point_cloud_device(t1, colors=tc, stream=st, **_KW), pc.point_cloud(d1, colors=bgr, **_KW), "stream")

    L = _dsx.lib()
    c = _dsx.make_cloud(_KW["focal_length"], _KW["baseline"], (W - 1) / 2, (H - 1) / 2, _KW["doffs"], _KW["eps"],
                        _KW["max_depth"], 0)
    nbytes = L.dsx_point_cloud_workspace_bytes(H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    outs = []
    with torch.cuda.stream(st):
        for t in (t1, t2):
            P = torch.empty((H * W, 3), dtype=torch.float32, device="cuda")
            I = torch.empty((H * W,), dtype=torch.int32, device="cuda")
            n = torch.empty(1, dtype=torch.int32, device="cuda")
            rc = L.dsx_point_cloud_device(t.data_ptr(), H, W, W, ctypes.byref(c), None, 0, 0, P.data_ptr(), None,
                                          I.data_ptr(), H * W, n.data_ptr(), ws.data_ptr(), nbytes, st.cuda_stream)
            assert rc == _dsx.DSX_OK, _dsx.last_error()
            outs.append((P, I, n))
    st.synchronize()
    for (P, I, n), d in zip(outs, (d1, d2)):
        wp, _, wi = pc.point_cloud(d, **_KW)
        k = int(n.item())
        _assert_cloud((P[:k], None, I[:k]), (wp, None, wi), "shared workspace")


def test_empty_map_and_argument_errors():
    import torch
    from depthestimation_amd.matcher import point_cloud_device, reproject_device
    e = torch.empty((0, 17), dtype=torch.float32, device="cuda")
    pts, col, idx = point_cloud_device(e, **_KW)
    assert pts.shape == (0, 3) and col is None and idx.shape == (0,)
    assert reproject_device(e, **_KW).shape == (0, 17, 3)
    d = torch.ones((4, 8), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        point_cloud_device(d, **dict(_KW, focal_length=0.0))
    with pytest.raises(ValueError):
        point_cloud_device(d.double(), **_KW)
    with pytest.raises(ValueError):
        point_cloud_device(d, colors=torch.zeros((4, 8, 3), dtype=torch.uint8, device="cuda"), **dict(_KW, x0=2))
    with pytest.raises(ValueError):
        point_cloud_device(d, out_points=torch.empty((31, 3), dtype=torch.float32, device="cuda"), **_KW)
    with pytest.raises(ValueError):
        point_cloud_device(d, capacity=-1, **_KW)
    with pytest.raises(ValueError):
        reproject_device(d, out=torch.empty((4, 8), dtype=torch.float32, device="cuda"), **_KW)


# --------------------------------------------------------------------------- StereoCore
_H, _W, _D = 48, 192, 32
_F, _B, _ZMAX = 431.7, 0.193, 11.0                               # neither f nor B is a float32 number


@functools.lru_cache(maxsize=None)
def _core_frame():
    L, R, _ = layered_pair(_H, _W, _D, seed=1234)
    core = StereoCore(fast_mode=False)
    core.configure_sgbm(num_disp=_D, block_size=9, focal_length=_F, baseline=_B, max_depth=_ZMAX)
    disp, depth = core.estimate_depth(L, R)
    return core, L, R, disp, depth


def test_stereo_core_point_cloud(monkeypatch):
    import depthestimation_amd.stereo_core as sc
    core, L, R, disp, depth = _core_frame()

    def no_host(*a, **k):
        raise AssertionError("the host restatement ran where the device pipeline applies")
    monkeypatch.setattr(sc, "host_point_cloud", no_host)
    pts, col, idx = core.point_cloud()
    want = pc.point_cloud(disp, _F, _B, principal_point=((_W - 1) / 2, (_H - 1) / 2), eps=0, max_depth=_ZMAX, x0=_D,
                          colors=L)
    np.testing.assert_array_equal(_bits(pts), _bits(want[0]))
    np.testing.assert_array_equal(col, want[1])
    np.testing.assert_array_equal(idx, want[2])
    # every point's Z has the depth map's bits wherever that depth is below max_depth; those are all the points
    below = depth.ravel() < np.float32(_ZMAX)
    print(f"{len(pts)} points of {below.size} pixels, {int((depth.ravel() == np.float32(_ZMAX)).sum())} at max_depth")
    assert 0.2 * below.size < below.sum() < below.size
    assert len(pts) == int(below.sum())
    np.testing.assert_array_equal(idx, np.flatnonzero(below))
    np.testing.assert_array_equal(_bits(pts[:, 2]), _bits(depth.ravel()[idx]))


def test_stereo_core_point_cloud_device():
    import torch
    core, L, R, disp, depth = _core_frame()
    d, z = core.estimate_depth_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    want = pc.point_cloud(disp, _F, _B, eps=0, max_depth=_ZMAX, x0=_D, colors=L)
    _assert_cloud(core.point_cloud_device(d), want, "sync")
    pts, col, idx, count = core.point_cloud_device(d, sync=False)
    torch.cuda.synchronize()
    n = int(count.item())
    assert pts.shape == (d.numel(), 3) and n == len(want[0])
    _assert_cloud((pts[:n], col[:n], idx[:n]), want, "sync=False")
