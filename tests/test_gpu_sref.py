"""Reference row of the rotated row loop (csrc/dsx_bm.hip; pair layout, one-wave left pass, block sizes up to
11, the strips that load unaligned dwords - "FAST" below).  The cases were written for a form that took the row
through the scalar unit (rejected and removed from the source): a step read the aligned dwords that
hold the bytes [x0 - R, x0 - R + 4 NC4) of the entering and the leaving reference row and shifted the
misalignment out.  The shipped loop reads the row from its staged LDS copy, and the cases guard what any form of
that read can get wrong: the alignment of the row pointer (base pointer, byte offset of a view, row stride), the
last dword of a row, the rows taken before a segment's first step and behind its last one, and the byte of a
column.

Every comparison is bit for bit over all pixels against the C oracle (oracle/cref.py): the int16 x16 map and
the float map - float mode 'fixed' against x16 / 16 (exact in f32), 'parabola' by bit pattern.  Every case
asserts from the launch geometry restated in tests/fused_geometry.py (the plan functions of
csrc/dsx_partition.h) that a strip with the unaligned-dword loads runs, and where the column update matters
that one of its segments has two rows or more (a segment's first row has no column update).

Base: D = 128, block 9, W = 256: strips 3..7 run, x0 = 160 and 192 with the unaligned-dword loads.
"""
from __future__ import annotations

import numpy as np
import pytest

from depthestimation_amd.synthetic import binary_pair, stereo_pair

import fused_geometry as fg

pytestmark = pytest.mark.gpu

M, D, BS, W0 = 0, 128, 9, 256
BASE = dict(min_disp=M, num_disp=D, block_size=BS, cost="sad", disp12_max_diff=-1)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _segments(H, gb, W=W0, m=M, nf=1, bs=BS, d=D):
    """Every segment (fused_geometry.Seg; FAST = its fast flag) of a left-pass launch."""
    return [s for b in fg.blocks(H, gb, W, m, nf, bs // 2, d) for s in b]


def _covered(H, gb, rows=1, **kw):
    """The coverage assertion: a FAST segment of at least ``rows`` rows runs.  Returns the FAST segments."""
    segs = [s for s in _segments(H, gb, **kw) if s.fast]
    assert segs and max(s.rows for s in segs) >= rows, (H, gb, kw, segs)
    return segs


def _run(torch, dL, dR, shape, want, what, grids, fmode="fixed", stride=None, **kw):
    """dL / dR: device tensors (any view) or (ptr, H, W) tuples with ``stride``."""
    from depthestimation_amd.matcher import HipBlockMatcher
    for g in grids:
        mt = HipBlockMatcher(grid_blocks=g, float_mode=fmode, **kw)
        try:
            fx = torch.empty(shape, dtype=torch.int16, device="cuda")
            fl = torch.empty(shape, dtype=torch.float32, device="cuda")
            mt.compute_device(dL, dR, out_fixed=fx, out_float=fl, stride=stride)
            torch.cuda.synchronize()
            fg.check_maps(fx, fl, want, f"{what} grid_blocks={g}", fmode)
        finally:
            mt.close()


def _pair(H, W=W0, m=M, d=D, seed=0):
    L, R, _ = stereo_pair(H, W, m, d, seed=7300 + 13 * H + seed)
    return L, R


def _all_modes(torch, key, L, R, grids, what, m=M, d=D, bs=BS, modes=(("fixed", True), ("parabola", True)), us=(0, 10)):
    kw = dict(BASE, min_disp=m, num_disp=d, block_size=bs)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    for u in us:
        for fmode, sp in modes:
            want = fg.want(key, L, R, m, d, bs, u, sp)
            _run(torch, dL, dR, L.shape, want, f"{what} u={u} {fmode} subpixel={sp}", grids, fmode=fmode,
                 uniqueness_ratio=u, subpixel=sp, **kw)


# ---- base shape: segment lengths ---------------------------------------------------------------------

def test_base_geometry():
    """x0 = 160 and 192 are the FAST strips of the base shape, and the (H, grid_blocks) set of the base test holds
    FAST segments of 1, 2, 3 and 20 or more rows and blocks that run on from a FAST strip into the next one."""
    assert sorted({s.x0 for s in _segments(24, 0) if s.fast}) == [160, 192]
    assert sorted({s.x0 for s in _segments(24, 0) if not s.fast}) == [96, 128, 224]
    lens = set()
    for H in (1, 2, 7, 24):
        for gb in (0, 1, 4):
            lens |= {s.rows for s in _covered(H, gb)}
    assert {1, 2, 3} <= lens and max(lens) >= 20, lens
    # one block: strips in a row, the rows taken ahead at the end of x0 = 160 are dropped at the start of x0 = 192
    assert [(s.x0, s.rows) for s in _segments(24, 1)] == [(96, 24), (128, 24), (160, 24), (192, 24), (224, 24)]


@pytest.mark.parametrize("H", [1, 2, 7, 24])
@pytest.mark.parametrize("gb", [0, 1, 4])
def test_base_shape(torch_dev, H, gb):
    _covered(H, gb, rows=min(H, 2) if gb == 1 else 1)
    L, R = _pair(H)
    _all_modes(torch_dev, ("random", H), L, R, (gb,), f"H={H} random")


# ---- alignment ---------------------------------------------------------------------------------------

def _views(torch, L, R, off, stride):
    """L and R as views at byte offset ``off`` (R: 3 - off) of larger uint8 tensors, rows ``stride`` bytes apart.
    The bytes around the images are noise, so a byte taken from beside a row shows."""
    H, W = L.shape
    rng = np.random.default_rng(40 + 4 * off + stride)
    out = []
    for img, o in ((L, off), (R, 3 - off)):
        host = rng.integers(0, 256, 8 + H * stride, dtype=np.uint8)
        rows = np.lib.stride_tricks.as_strided(host[o:], (H, W), (stride, 1))
        rows[...] = img
        buf = torch.from_numpy(host).cuda()
        out.append((buf, torch.as_strided(buf, (H, W), (stride, 1), o)))
    return out


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("pad", [0, 1, 2, 3])
def test_alignment_of_views(torch_dev, off, pad):
    """Base pointer at byte offset 0..3 and row strides W .. W + 3: every residue of the row pointer, changing from
    row to row when the stride is no multiple of 4.  As tensors and as (ptr, H, W) with stride."""
    torch = torch_dev
    H = 7
    _covered(H, 4, rows=2)
    _covered(H, 1, rows=2)
    L, R = _pair(H)
    want = fg.want(("random", H), L, R, M, D, BS, 10, True)
    (bl, vl), (br, vr) = _views(torch, L, R, off, W0 + pad)
    assert vl.data_ptr() % 4 == (bl.data_ptr() + off) % 4 and vl.stride(0) == W0 + pad
    _run(torch, vl, vr, L.shape, want, f"views off={off} stride=W+{pad}", (4,), uniqueness_ratio=10, **BASE)
    _run(torch, (vl.data_ptr(), H, W0), (vr.data_ptr(), H, W0), L.shape, want, f"pointers off={off} stride=W+{pad}",
         (1,), stride=W0 + pad, uniqueness_ratio=10, **BASE)


@pytest.mark.parametrize("W", [288, 292])
def test_left_image_ends_its_allocation(torch_dev, W):
    """The left image is a tensor of exactly H * W bytes.  W = 288 (a multiple of 32): the last FAST strip is x0 = 224
    and its rows end at byte 259 of the row.  W = 292 = 256 + 36: the last FAST strip is x0 = 256, whose reference bytes
    [252, 292) end with the row, so in the last row its final dword ends at the tensor's last byte (and, the tensor
    being aligned and W a multiple of 4, no further dword is read)."""
    torch = torch_dev
    H = 7
    fast = sorted({s.x0 for s in _covered(H, 4, rows=2, W=W)})
    assert fast[-1] == (224 if W == 288 else 256)
    assert (fast[-1] - BS // 2 + 40 == W) == (W == 292)
    L, R = _pair(H, W=W, seed=W)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    assert dL.numel() == H * W and dL.is_contiguous()
    for u in (0, 10):
        want = fg.want(("random", H, W), L, R, M, D, BS, u, True)
        _run(torch, dL, dR, L.shape, want, f"W={W} u={u}", (0, 1, 4), uniqueness_ratio=u, **BASE)


# ---- radii -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bs", [1, 5, 7, 11])
def test_block_sizes(torch_dev, bs):
    """R = 0, 2, 3, 5: 8, 9, 10 and 11 reference dwords per row (+ 1 when misaligned); at R = 5 the last chunk has two
    columns and the last dword two needed bytes.  Odd stride and offset, so the shift is live at every radius."""
    torch = torch_dev
    for H, gb in ((7, 4), (24, 1)):
        _covered(H, gb, rows=2, bs=bs)
        L, R = _pair(H)
        _all_modes(torch, ("random", H), L, R, (gb,), f"block {bs} H={H}", bs=bs)
    H = 7
    L, R = _pair(H)
    want = fg.want(("random", H), L, R, M, D, bs, 10, True)
    (_, vl), (_, vr) = _views(torch, L, R, 1, W0 + 3)
    _run(torch, vl, vr, L.shape, want, f"block {bs} view off=1 stride=W+3", (4,), uniqueness_ratio=10,
         **dict(BASE, block_size=bs))


# ---- values ------------------------------------------------------------------------------------------

def test_extreme_and_constant_values(torch_dev):
    """Images of 0 and 255 only (every byte difference 0 or 255: a wrong byte moves a cost by 255) and a constant
    image (winner 0 everywhere)."""
    H = 7
    _covered(H, 4, rows=2)
    Lb, Rb = binary_pair(H, W0, M, D, seed=191 + H)[:2]
    assert set(np.unique(Lb)) <= {0, 255} and set(np.unique(Rb)) <= {0, 255}
    _all_modes(torch_dev, ("binary", H), Lb, Rb, (0, 1, 4), "binary")
    C = np.full((H, W0), 93, np.uint8)
    want = fg.want(("const", H), C, C, M, D, BS, 0, True)
    assert np.all(want["fixed"][:, D - 1:] == 0)
    _all_modes(torch_dev, ("const", H), C, C.copy(), (0, 1, 4), "constant")


# ---- other modes -------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [96, 127])
def test_num_disparities(torch_dev, d):
    for H, gb in ((7, 4), (24, 1)):
        _covered(H, gb, rows=2, d=d)
        L, R = _pair(H, d=d, seed=d)
        _all_modes(torch_dev, ("random", H, d), L, R, (gb,), f"D={d} H={H}", d=d)


def test_min_disp(torch_dev):
    H, m = 24, 3
    _covered(H, 4, rows=2, m=m)
    L, R = _pair(H, m=m, seed=3)
    _all_modes(torch_dev, ("random", H, "m3"), L, R, (0, 1, 4), f"min_disp={m}", m=m)


def test_batch_of_two_frames(torch_dev):
    """Two frames per launch: the frame offset enters the row pointer (frame stride H * W + 5, odd)."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    H = 7
    L0, R0 = _pair(H)
    L1, R1 = _pair(H, seed=1)
    fr = [(L0, R0), (L1, R1)]
    for g in (0, 1, 3):
        assert {s.frame for s in _covered(H, g, nf=2)} == {0, 1}
    fs = H * W0 + 5
    bufs = []
    for k in range(2):
        b = torch.zeros(2 * fs, dtype=torch.uint8, device="cuda")
        v = torch.as_strided(b, (2, H, W0), (fs, W0, 1), 0)
        v.copy_(torch.from_numpy(np.stack([f[k] for f in fr])).cuda())
        bufs.append((b, v))
    for u in (0, 10):
        wants = [fg.want(("random", H) if i == 0 else ("random1", H), L, R, M, D, BS, u, True) for i, (L, R) in enumerate(fr)]
        for g in (0, 1, 3):
            mt = HipBlockMatcher(grid_blocks=g, uniqueness_ratio=u, **BASE)
            try:
                fx = torch.empty((2, H, W0), dtype=torch.int16, device="cuda")
                fl = torch.empty((2, H, W0), dtype=torch.float32, device="cuda")
                mt.compute_batch_device(bufs[0][1], bufs[1][1], out_fixed=fx, out_float=fl)
                torch.cuda.synchronize()
                for i in range(2):
                    fg.check_maps(fx[i], fl[i], wants[i], f"batch u={u} grid_blocks={g} frame={i}")
            finally:
                mt.close()


def test_in_flight_handles(torch_dev):
    """Two in_flight handles on two streams, two rounds, each with its own frame and oracle."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    H = 24
    _covered(H, 0, rows=1)
    fr = [_pair(H), binary_pair(H, W0, M, D, seed=191 + H)[:2]]
    wants = [fg.want(("random", H), *fr[0], M, D, BS, 0, True), fg.want(("binary", H), *fr[1], M, D, BS, 0, True)]
    dev = [(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in fr]
    handles = [HipBlockMatcher(in_flight=True, uniqueness_ratio=0, **BASE) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    fx = [torch.empty((H, W0), dtype=torch.int16, device="cuda") for _ in range(4)]
    fl = [torch.empty((H, W0), dtype=torch.float32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    try:
        for i in range(4):
            handles[i % 2].compute_device(*dev[i % 2], out_fixed=fx[i], out_float=fl[i], stream=streams[i % 2])
        torch.cuda.synchronize()
        for i in range(4):
            fg.check_maps(fx[i], fl[i], wants[i % 2], f"in_flight handle {i % 2} call {i // 2}")
    finally:
        for h in handles:
            h.close()


def test_in_flight_grid_below_the_row_count(torch_dev):
    """An in_flight handle launches one-wave blocks on two thirds of the resident capacity (launch_bm2_side).  With
    H = 480 the launch has 5 * 480 = 2400 strip rows, more than that grid on a device of 256 CUs (2048 blocks; a
    lone-frame handle launches a block per row), so blocks own one or two rows and some run on into the next strip.
    Whatever the device's capacity, the maps equal the oracle's and a lone-frame handle's."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    H = 480
    assert {s.rows for s in _covered(H, 2048, rows=2)} == {1, 2}
    L, R = _pair(H)
    want = fg.want(("random", H), L, R, M, D, BS, 10, True)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    for fl in (True, False):
        mt = HipBlockMatcher(in_flight=fl, uniqueness_ratio=10, **BASE)
        try:
            fx = torch.empty(L.shape, dtype=torch.int16, device="cuda")
            fo = torch.empty(L.shape, dtype=torch.float32, device="cuda")
            mt.compute_device(dL, dR, out_fixed=fx, out_float=fo)
            torch.cuda.synchronize()
            fg.check_maps(fx, fo, want, f"H={H} in_flight={fl}")
        finally:
            mt.close()


# ---- prefilter ---------------------------------------------------------------------------------------

def test_rows_written_by_the_prefilter(torch_dev):
    """x-Sobel prefilter on the device: the matcher's scalar loads read rows that a kernel wrote just before it on
    the same stream.  Two calls with different frames through one handle, so the second call's rows replace the
    first call's at the same addresses."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    from depthestimation_amd.prefilter import prefilter_xsobel
    H = 24
    _covered(H, 4, rows=2)
    frames = [_pair(H), _pair(H, seed=5)]
    mt = HipBlockMatcher(grid_blocks=4, uniqueness_ratio=10, prefilter_type="xsobel", prefilter_cap=31, **BASE)
    try:
        for i, (L, R) in enumerate(frames):
            want = fg.want(("xsobel", H, i), prefilter_xsobel(L, 31), prefilter_xsobel(R, 31), M, D, BS, 10, True)
            fx = torch.empty(L.shape, dtype=torch.int16, device="cuda")
            fl = torch.empty(L.shape, dtype=torch.float32, device="cuda")
            mt.compute_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), out_fixed=fx, out_float=fl)
            torch.cuda.synchronize()
            fg.check_maps(fx, fl, want, f"xsobel frame {i}")
    finally:
        mt.close()
