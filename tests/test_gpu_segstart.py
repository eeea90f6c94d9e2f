"""Segment start of the fused pass (csrc/dsx_bm.hip): the code between kernel entry and a segment's first row step -
the block's partition words, the loads of the 2R+1 init rows in one batch (-DDSX_SEGSTART_BATCH) and the init SAD
loop's LDS reads one chunk ahead (-DDSX_SEGSTART_AHEAD).  The cases hold for both settings of either switch; they
were run on the default build and, with the radius-4 unit (block 9) rebuilt, on AHEAD / BATCH = 1 0 and 0 1, and also
on builds that took the partition words through scalar loads at kernel entry, a form that was rejected and removed
from the source.

What these forms can get wrong is a row of the init (clamped into the frame at both ends, rows past 2R zero), the
column chunk a read belongs to (the last one partial at odd radii), and the block's first and last unit.  So the
cases are chosen by where segments start and how long they are, from the launch geometry restated in
tests/fused_geometry.py (the host partition and the kernel's test for the unaligned-dword copy, "fast" below; the
others take clamped bytes), and every case asserts from that restatement that the classes it is there for occur.

Every comparison is bit for bit over all pixels against the C oracle (oracle/cref.py): the int16 x16 map and the
float map - float mode 'fixed' against x16 / 16 (exact in f32), 'parabola' by bit pattern.

Base: D = 128, block 9, W = 256: the valid band starts at x = 127, strips 3..7 run, x0 = 160 and 192 with the
unaligned-dword loads and 96, 128, 224 with clamped bytes, so both copies of the segment start run.
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


def _blocks(H, gb, W=W0, m=M, nf=1, R=BS // 2, d=D):
    """Per block of a left-pass launch its segments (fused_geometry.Seg), in order."""
    return fg.blocks(H, gb, W, m, nf, R, d)


def _kinds(blocks, H, R=BS // 2):
    """Segment classes of a launch; 'f:' marks the unaligned-dword copy, 'c:' the clamped one."""
    k = set()
    for b in blocks:
        for s in b:
            p = "f:" if s.fast else "c:"
            for name, hit in (("row0", s.y0 == 0), ("last", s.y0 == H - 1), ("last-R", s.y0 == H - 1 - R and s.y0 > 0),
                              ("inside", 0 < s.y0 < H - 1), ("one", s.rows == 1), ("long", s.rows >= 2 * R + 2)):
                if hit:
                    k.add(p + name)
        if len(b) > 1 and any(p.strip != q.strip and p.frame == q.frame for p, q in zip(b, b[1:])):
            k.add("next_strip")
        if len(b) > 1 and any(p.frame != q.frame for p, q in zip(b, b[1:])):
            k.add("next_frame")
    return k


def _run(torch, dL, dR, shape, want, what, grids, fmode="fixed", **kw):
    from depthestimation_amd.matcher import HipBlockMatcher
    for g in grids:
        mt = HipBlockMatcher(grid_blocks=g, float_mode=fmode, **kw)
        try:
            fx = torch.empty(shape, dtype=torch.int16, device="cuda")
            fl = torch.empty(shape, dtype=torch.float32, device="cuda")
            mt.compute_device(dL, dR, out_fixed=fx, out_float=fl)
            torch.cuda.synchronize()
            fg.check_maps(fx, fl, want, f"{what} grid_blocks={g}", fmode)
        finally:
            mt.close()


def _pair(H, W=W0, m=M, d=D, seed=0):
    L, R, _ = stereo_pair(H, W, m, d, seed=7300 + 13 * H + seed)
    return L, R


def _both_modes(torch, key, L, R, grids, what, d=D, bs=BS, u=10, lr=-1, **kw):
    """Both float modes (the int16 map with each)."""
    want = fg.want(key, L, R, M, d, bs, u, True, lr)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    par = dict(BASE, num_disp=d, block_size=bs, uniqueness_ratio=u, disp12_max_diff=lr)
    par.update(kw)
    for fmode in ("fixed", "parabola"):
        _run(torch, dL, dR, L.shape, want, f"{what} {fmode}", grids, fmode=fmode, **par)


# ---- frame heights around 2R+1 -----------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 2, 8, 9, 10])
def test_short_frames(torch_dev, H):
    """Frames shorter than, equal to and just above 2R+1 = 9 rows: the init clamps at both ends.  One block per
    strip (every segment starts at row 0 and takes the whole frame) and one per row."""
    whole, rows = _kinds(_blocks(H, 5), H), _kinds(_blocks(H, 0), H)
    assert {"f:row0", "c:row0"} <= whole and all(len(b) == 1 and b[0].rows == H for b in _blocks(H, 5))
    # the strips with clamped bytes weigh more and get a block per row; those with unaligned dwords get one per row
    # only in frames of one or two rows (above that their last segment has two rows or more at every grid)
    assert {"f:one", "c:one", "c:last"} <= rows and (H > 2 or "f:last" in rows)
    L, R = _pair(H)
    _both_modes(torch_dev, ("random", H), L, R, (5, 0), f"H={H} random")
    Lb, Rb = binary_pair(H, W0, M, D, seed=31 + H)[:2]  # differences of 0 and 255: a wrong row moves a cost by 255
    _both_modes(torch_dev, ("binary", H), Lb, Rb, (5, 0), f"H={H} binary", u=0)


# ---- where segments start ----------------------------------------------------------------------------

# (H, grid_blocks) -> classes the launch must contain.  H = 20, R = 4: H - 1 - R = 15.  A block per row gives every
# start row as one-row segments in the clamped copy and all but the last in the other (see test_short_frames); 4 blocks per strip (20 blocks) cut at rows 5, 10 and 15, so the
# segment of rows 15..19 starts at H - 1 - R and the first step's entering row is the frame's last; fewer blocks than
# strips make blocks that go on into the next strip.
CLAIMS = {(20, 0): {"f:row0", "f:last-R", "f:one", "c:row0", "c:last", "c:last-R", "c:one"},
          (20, 20): {"f:row0", "f:last-R", "f:inside"},
          (20, 3): {"next_strip", "f:inside", "f:row0"},
          (20, 1): {"next_strip", "f:long", "c:long"},
          (41, 7): {"f:long", "f:row0"}}


@pytest.mark.parametrize("H,gb", sorted(CLAIMS))
def test_segment_starts(torch_dev, H, gb):
    blocks = _blocks(H, gb)
    assert CLAIMS[(H, gb)] <= _kinds(blocks, H), (H, gb, blocks)
    if (H, gb) == (20, 20):  # rows 15..19 of a strip with the unaligned-dword loads are one segment
        assert any(s.y0 == 15 and s.rows == 5 and s.fast for b in blocks for s in b)
    L, R = _pair(H)
    _both_modes(torch_dev, ("random", H), L, R, (gb,), f"H={H} random")
    _both_modes(torch_dev, ("random", H), L, R, (gb,), f"H={H} random u=0", u=0)


# ---- radii, disparity ranges ---------------------------------------------------------------------------

@pytest.mark.parametrize("bs,d", [(1, 128), (5, 128), (7, 128), (9, 128), (11, 128), (15, 192)])
def test_block_sizes(torch_dev, bs, d):
    """R = 0 .. 7: one to four row groups (the last with 1, 1, 3, 1, 3 and 3 rows), 8 to 12 column chunks, the last
    one partial at odd R.  Block 15 with D = 192 runs two waves per block."""
    R = bs // 2
    W = 256 if d == 128 else 352
    for H, gb in ((2 * R + 2, 0), (20, 3)):
        blocks = _blocks(H, gb, W=W, R=R, d=d)
        kinds = _kinds(blocks, H, R)
        assert "f:row0" in kinds and ("f:one" in kinds if gb == 0 else {"f:long", "next_strip"} <= kinds), (bs, H, gb, blocks)
        L, Rr = _pair(H, W=W, d=d, seed=bs)
        _both_modes(torch_dev, ("random", H, W, d), L, Rr, (gb,), f"block {bs} D={d} H={H}", d=d, bs=bs)


def test_sad1(torch_dev):
    """D = 64: one disparity per lane (SAD1), the transposed init with one SAD per column and group."""
    d, W = 64, 192
    for H, gb in ((10, 0), (20, 3)):
        kinds = _kinds(_blocks(H, gb, W=W, d=d), H)
        assert "f:row0" in kinds and ("f:one" in kinds if gb == 0 else "f:inside" in kinds)
        L, R = _pair(H, W=W, d=d, seed=64)
        _both_modes(torch_dev, ("random", H, W, d), L, R, (gb,), f"D=64 H={H}", d=d)


# ---- frames, views, handles ----------------------------------------------------------------------------

def test_batch_of_two_frames(torch_dev):
    """Two frames per launch: blocks go on into the next frame, whose init rows clamp at its own first row."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    H = 10
    L0, R0 = _pair(H)
    L1, R1 = _pair(H, seed=1)
    fr = [(L0, R0), (L1, R1)]
    kinds = set()
    for g in (0, 3, 7):
        kinds |= _kinds(_blocks(H, g, nf=2), H)
    assert {"next_frame", "next_strip", "f:row0", "c:last", "f:inside"} <= kinds
    dL = torch.from_numpy(np.stack([f[0] for f in fr])).cuda()
    dR = torch.from_numpy(np.stack([f[1] for f in fr])).cuda()
    wants = [fg.want(("random", H) if i == 0 else ("random1", H), L, R, M, D, BS, 10, True) for i, (L, R) in enumerate(fr)]
    for g in (0, 3, 7):
        mt = HipBlockMatcher(grid_blocks=g, uniqueness_ratio=10, **BASE)
        try:
            fx = torch.empty((2, H, W0), dtype=torch.int16, device="cuda")
            fl = torch.empty((2, H, W0), dtype=torch.float32, device="cuda")
            mt.compute_batch_device(dL, dR, out_fixed=fx, out_float=fl)
            torch.cuda.synchronize()
            for i in range(2):
                fg.check_maps(fx[i], fl[i], wants[i], f"batch grid_blocks={g} frame={i}")
        finally:
            mt.close()


@pytest.mark.parametrize("off", [1, 2, 3])
def test_strided_views(torch_dev, off):
    """Rows W + 5 bytes apart, base pointers at byte offset ``off`` (left) and 4 - off (right) of noise buffers:
    a byte taken from beside a row shows."""
    torch = torch_dev
    H, stride = 10, W0 + 5
    assert {"f:row0", "f:inside", "c:inside"} <= _kinds(_blocks(H, 10), H)
    L, R = _pair(H)
    rng = np.random.default_rng(70 + off)
    views = []
    for img, o in ((L, off), (R, 4 - off)):
        host = rng.integers(0, 256, 8 + H * stride, dtype=np.uint8)
        np.lib.stride_tricks.as_strided(host[o:], (H, W0), (stride, 1))[...] = img
        buf = torch.from_numpy(host).cuda()
        views.append(torch.as_strided(buf, (H, W0), (stride, 1), o))
    assert views[0].data_ptr() % 4 == off and views[0].stride(0) == stride
    want = fg.want(("random", H), L, R, M, D, BS, 10, True)
    _run(torch, views[0], views[1], L.shape, want, f"views off={off}", (10, 0), uniqueness_ratio=10, **BASE)


def test_in_flight_handle(torch_dev):
    """An in_flight handle (its own grid rule) on a side stream, two calls."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    H = 20
    L, R = _pair(H)
    want = fg.want(("random", H), L, R, M, D, BS, 10, True)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    assert "f:one" in _kinds(_blocks(H, 0), H)  # the resident capacity exceeds the 100 rows: a block per row
    mt = HipBlockMatcher(in_flight=True, uniqueness_ratio=10, **BASE)
    st = torch.cuda.Stream()
    fx = [torch.empty((H, W0), dtype=torch.int16, device="cuda") for _ in range(2)]
    fl = [torch.empty((H, W0), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    try:
        for i in range(2):
            mt.compute_device(dL, dR, out_fixed=fx[i], out_float=fl[i], stream=st)
        torch.cuda.synchronize()
        for i in range(2):
            fg.check_maps(fx[i], fl[i], want, f"in_flight call {i}")
    finally:
        mt.close()


# ---- the other passes ----------------------------------------------------------------------------------

@pytest.mark.parametrize("bs", [5, 9])
def test_lr_pass(torch_dev, bs):
    """Side 3 (left pass + right-view winners, LR check): block 5 takes the transposed init, block 9 the row-by-row one."""
    for H, gb in ((10, 0), (20, 3)):
        blocks = _blocks(H, gb, R=bs // 2)
        assert "f:row0" in _kinds(blocks, H, bs // 2)
        L, R = _pair(H)
        _both_modes(torch_dev, ("random", H), L, R, (gb,), f"lr bm block {bs} H={H}", bs=bs, lr=1, lr_form="bm")


def test_volume_path(torch_dev):
    """Side 2: the cost volume written by the same segment start, winners taken from it afterwards."""
    for H, gb in ((10, 0), (20, 3)):
        assert "f:row0" in _kinds(_blocks(H, gb), H)
        L, R = _pair(H)
        _both_modes(torch_dev, ("random", H), L, R, (gb,), f"volume H={H}", lr=1, path="volume")
