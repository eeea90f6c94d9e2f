"""Rotated row loop of the fused pass (csrc/dsx_bm.hip, pair layout, one-wave left pass, block sizes up to 11):
step y of a segment runs the epilogue of row y - 1 between the chunks of row y's column update, and the column
update reads its staged words one chunk ahead.  Both are the only form in the source (their A/B switches were
folded once settled); the cases guard the segment shapes below, at which the rotation can go wrong.

A segment's first step has no epilogue and one epilogue drains the segment behind its last step, so what decides
the code path is the segment length: 1 row is init + drain only, 2 rows have one overlapped step.  The cases are
chosen by it from the launch geometry restated in tests/fused_geometry.py, and every
case asserts from that restatement that the classes it is there for occur: segments of 1, 2, 3 and 20 or more
rows, blocks that own several segments in a row (they go on into the next strip or frame), strips cut inside
(a segment that starts below row 0).

Every comparison is bit for bit over all pixels against the C oracle (oracle/cref.py): the int16 x16 map and
the float map - float mode 'fixed' against x16 / 16 (exact in f32), 'parabola' by bit pattern.

Base: D = 128, block 9, W = 256: the valid band starts at x = 127, strips 3..7 run, x0 = 160 and 192 with
the unaligned-dword loads and 96, 128, 224 with clamped bytes, so both copies of the row loop run.
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


def _kinds(blocks):
    segs = [s for b in blocks for s in b]
    k = {name for name, f in (("one", lambda n: n == 1), ("two", lambda n: n == 2), ("three", lambda n: n == 3),
                              ("long", lambda n: n >= 20)) if any(f(s.rows) for s in segs)}
    if any(len(b) > 1 and any(p.strip != q.strip and p.frame == q.frame for p, q in zip(b, b[1:])) for b in blocks):
        k.add("next_strip")  # a block goes on into the next strip: two segments in a row
    if any(len(b) > 1 and any(p.frame != q.frame for p, q in zip(b, b[1:])) for b in blocks):
        k.add("next_frame")
    if any(s.y0 > 0 for s in segs):
        k.add("cut")  # a strip cut inside: the segment starts below row 0
    return k


def _run(torch, L, R, want, what, grids, fmode="fixed", **kw):
    from depthestimation_amd.matcher import HipBlockMatcher
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    for g in grids:
        mt = HipBlockMatcher(grid_blocks=g, float_mode=fmode, **kw)
        try:
            fx = torch.empty(L.shape, dtype=torch.int16, device="cuda")
            fl = torch.empty(L.shape, dtype=torch.float32, device="cuda")
            mt.compute_device(dL, dR, out_fixed=fx, out_float=fl)
            torch.cuda.synchronize()
            fg.check_maps(fx, fl, want, f"{what} grid_blocks={g}", fmode)
        finally:
            mt.close()


def _pair(H, W=W0, m=M, d=D, seed=0):
    L, R, _ = stereo_pair(H, W, m, d, seed=5200 + 13 * H + seed)
    return L, R


def _all_modes(torch, key, L, R, grids, what, m=M, d=D, bs=BS, modes=(("fixed", True), ("parabola", True)), us=(0, 10)):
    kw = dict(BASE, min_disp=m, num_disp=d, block_size=bs)
    for u in us:
        for fmode, sp in modes:
            want = fg.want(key, L, R, m, d, bs, u, sp)
            _run(torch, L, R, want, f"{what} u={u} {fmode} subpixel={sp}", grids, fmode=fmode, uniqueness_ratio=u, subpixel=sp, **kw)


# ---- segment lengths ---------------------------------------------------------------------------------

# (H, grid_blocks) -> what the launch must contain.  With fewer blocks than strips (5) the blocks take an even
# split of the linearised rows and go on into the next strip: H = 7 in 4 blocks is 7 1 | 6 3 | 4 5 | 2 7, in 3
# blocks 7 4 | 3 7 2 | 5 7; H = 41 in 3 blocks 41 27 | 14 41 13 | 28 41, in 4 blocks 41 10 | 31 20 | 21 30 | 11 41.
# From 5 blocks on a block stays inside a strip: 7 blocks cut two strips (H = 24: 12 + 12).  With a block per row
# (0 = the resident capacity, clipped to the row count) the clamped strips get more blocks than rows and the
# others fewer: single rows and pairs.
CLAIMS = {(7, 4): {"one", "two", "three", "next_strip", "cut"}, (7, 3): {"two", "three", "next_strip", "cut"},
          (7, 0): {"one", "two"}, (7, 1): {"next_strip"}, (24, 1): {"long", "next_strip"}, (24, 7): {"long", "cut"},
          (41, 3): {"long", "next_strip", "cut"}, (41, 4): {"long", "next_strip", "cut"}, (41, 0): {"one", "two"}}


@pytest.mark.parametrize("H,gb", sorted(CLAIMS))
def test_segment_lengths(torch_dev, H, gb):
    blocks = _blocks(H, gb)
    assert CLAIMS[(H, gb)] <= _kinds(blocks), (H, gb, blocks)
    if (H, gb) == (7, 4):
        assert [[s.rows for s in b] for b in blocks] == [[7, 1], [6, 3], [4, 5], [2, 7]]
    if (H, gb) == (41, 4):
        assert [[s.rows for s in b] for b in blocks] == [[41, 10], [31, 20], [21, 30], [11, 41]]
    L, R = _pair(H)
    _all_modes(torch_dev, ("random", H), L, R, (gb,), f"H={H} random")
    Lb, Rb = binary_pair(H, W0, M, D, seed=91 + H)[:2]  # ties between neighbouring disparities: quotient 8
    _all_modes(torch_dev, ("binary", H), Lb, Rb, (gb,), f"H={H} binary")


def test_every_class_is_covered():
    kinds = set()
    for (H, gb) in CLAIMS:
        kinds |= _kinds(_blocks(H, gb))
    assert {"one", "two", "three", "long", "next_strip", "cut"} <= kinds


def test_no_subpixel(torch_dev):
    L, R = _pair(7)
    _all_modes(torch_dev, ("random", 7), L, R, (0, 1, 4), "H=7 random", modes=(("fixed", False),))


def test_constant_images(torch_dev):
    """Flat cost rows: winner 0 everywhere, no sub-pixel step (the neighbour costs read at d = -1 are dropped)."""
    H = 7
    L = np.full((H, W0), 93, np.uint8)
    R = np.full((H, W0), 93, np.uint8)
    want = fg.want(("const", H), L, R, M, D, BS, 0, True)
    band = want["fixed"][:, D - 1:]
    assert np.all(band == 0)
    _all_modes(torch_dev, ("const", H), L, R, (0, 1, 4), "constant")


# ---- frames ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [7, 24])
def test_batch_of_two_frames(torch_dev, H):
    """Two frames per launch, frame 1 = frame 0 with the left image moved by one column: an epilogue that drains
    into the wrong frame or is lost at a frame boundary changes the result."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    L0, R0 = _pair(H)
    L1 = np.roll(L0, 1, axis=1)
    L1[:, 0] = L0[:, 0]
    fr = [(L0, R0), (L1, R0.copy())]
    dL = torch.from_numpy(np.stack([f[0] for f in fr])).cuda()
    dR = torch.from_numpy(np.stack([f[1] for f in fr])).cuda()
    kinds = set()
    for g in (0, 1, 3, 7):
        kinds |= _kinds(_blocks(H, g, nf=2))
    assert "next_frame" in kinds and "next_strip" in kinds
    for u in (0, 10):
        wants = [fg.want(("random", H) if i == 0 else ("rolled", H), L, R, M, D, BS, u, True) for i, (L, R) in enumerate(fr)]
        assert np.any(wants[0]["fixed"] != wants[1]["fixed"])
        for g in (0, 1, 3, 7):
            mt = HipBlockMatcher(grid_blocks=g, uniqueness_ratio=u, **BASE)
            try:
                fx = torch.empty((2, H, W0), dtype=torch.int16, device="cuda")
                fl = torch.empty((2, H, W0), dtype=torch.float32, device="cuda")
                mt.compute_batch_device(dL, dR, out_fixed=fx, out_float=fl)
                torch.cuda.synchronize()
                for i in range(2):
                    fg.check_maps(fx[i], fl[i], wants[i], f"batch H={H} u={u} grid_blocks={g} frame={i}")
            finally:
                mt.close()


def test_in_flight_handles(torch_dev):
    """Two in_flight handles on two streams, two rounds, each with its own frame and oracle."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    H = 24
    fr = [_pair(H), binary_pair(H, W0, M, D, seed=91 + H)[:2]]
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


# ---- other radii, disparity ranges, bands ----------------------------------------------------------------

@pytest.mark.parametrize("bs", [5, 11])
def test_block_sizes(torch_dev, bs):
    """R = 2 and R = 5 of the same code: 9 and 11 column chunks, the last one partial at R = 5."""
    for H in (7, 24):
        L, R = _pair(H)
        _all_modes(torch_dev, ("random", H), L, R, (0, 1, 4), f"block {bs} H={H}", bs=bs)


@pytest.mark.parametrize("d", [127, 96])
def test_masked_tile_stores(torch_dev, d):
    """D = 127: the odd-D overwrite of the last pair's high half follows the lane-indexed stores; D = 96 < Dp:
    lanes 48..63 store nothing and the padding keeps the value the segment start wrote.  The moved tile reads
    must see both."""
    for H in (7, 24):
        L, R = _pair(H, d=d, seed=d)
        Lb, Rb = binary_pair(H, W0, M, d, seed=17 + d + H)[:2]
        for name, (l, r) in (("random", (L, R)), ("binary", (Lb, Rb))):
            _all_modes(torch_dev, (name, H, d), l, r, (0, 1, 4), f"D={d} H={H} {name}", d=d)


def test_min_disp(torch_dev):
    H, m = 24, 3
    L, R = _pair(H, m=m, seed=3)
    _all_modes(torch_dev, ("random", H, "m3"), L, R, (0, 1, 4), f"min_disp={m}", m=m)
