"""Row staging and output stores of the rotated row loop of the fused pass (csrc/dsx_bm.hip, bm2_segment).  In the
shipped form row y - 1's two output stores, formed behind step y's last column chunk, are issued at the end of step
y, behind the staging of step y + 1's rows, which stands behind the box phase.  Two other orders were measured and
rejected and are no longer in the source: the staging directly behind the last column chunk, in front of
those stores, and a segment's first step's two rows loaded in front of the init SAD loop and staged in front of the row
loop.  The cases were run on builds of all three forms and of their combinations; they hold for the shipped one and
guard the shapes at which any such order can go wrong.

What it can get wrong is which slot pair a step writes (it alternates on y & 1 and the carried staging address
flips once per step), a slot written while its last reader still needs it, an output stored for the wrong
row or held across a step that has none, and the places the staging stands in: a one-step segment stages nothing
that is used, a two-step segment uses the first staged slots exactly once, and from three steps on a step reads what
the step before staged.  So the cases are chosen by segment length, first-row parity and position
in the frame, from the launch geometry restated in tests/fused_geometry.py (the host partition and the kernel's
test for the unaligned-dword copy, "f:" below; the others, "c:", take clamped bytes), and every case asserts from
that restatement that the classes it is there for occur.

Every comparison is bit for bit over all pixels against the C oracle (oracle/cref.py): the int16 x16 map and the
float map - float mode 'fixed' against x16 / 16 (exact in f32), 'parabola' by bit pattern.

Base: D = 128, block 9, W = 256: the valid band starts at x = 127, strips 3..7 run, x0 = 160 and 192 on the
unaligned-dword copy and 96, 128, 224 on the clamped one.  H is between 12 and 40.
"""
from __future__ import annotations

import numpy as np
import pytest

from depthestimation_amd.synthetic import stereo_pair

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


def _kinds(blocks, H):
    """Segment classes of a launch; 'f:' marks the unaligned-dword copy, 'c:' the clamped one.

    n1 / n2 / n3 / n4+: segments of one, two, three, four or more steps.  even / odd: parity of the first row of a
    segment of two steps or more (one that reads a staged slot pair).  row0 / last: a segment of two steps or more that
    starts at row 0 / ends at row H - 1.  next_strip: a block that goes from a strip's last row to the next strip's
    row 0; frame_cut: a segment that ends a frame's last strip while the next block starts the next frame's first."""
    k = set()
    for b in blocks:
        for s in b:
            p = "f:" if s.fast else "c:"
            n = s.rows
            k.add(p + ("n4+" if n >= 4 else f"n{n}"))
            if n >= 2:
                k.add(p + ("odd" if s.y0 & 1 else "even"))
                if s.y0 == 0:
                    k.add(p + "row0")
                if s.y0 + n == H:
                    k.add(p + "last")
        for p, q in zip(b, b[1:]):
            if p.frame == q.frame and q.strip == p.strip + 1 and p.y0 + p.rows == H and q.y0 == 0:
                k.add("next_strip")
    for b, c in zip(blocks, blocks[1:]):
        if b and c and c[0].frame == b[-1].frame + 1 and c[0].strip == 0 and c[0].y0 == 0 and b[-1].y0 + b[-1].rows == H:
            k.add("frame_cut")
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
    L, R, _ = stereo_pair(H, W, m, d, seed=9100 + 13 * H + seed)
    return L, R


def _both_modes(torch, key, L, R, grids, what, d=D, bs=BS, u=10, lr=-1, **kw):
    """Both float modes (the int16 map with each)."""
    want = fg.want(key, L, R, M, d, bs, u, True, lr)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    par = dict(BASE, num_disp=d, block_size=bs, uniqueness_ratio=u, disp12_max_diff=lr)
    par.update(kw)
    for fmode in ("fixed", "parabola"):
        _run(torch, dL, dR, L.shape, want, f"{what} {fmode}", grids, fmode=fmode, **par)


# ---- segment lengths, first-row parity, frame edges ----------------------------------------------------

# (H, grid_blocks) -> classes the launch must contain, in both copies of the loop where it names both.
# The strips of the clamped copy weigh 11/8 of the others, so at one grid they get shorter segments.
#  (12, 0)   a block per unit of weight: one step per segment in the clamped strips (nothing staged is used), one
#            or two in the others.
#  (12, 30)  one and two steps (clamped), two and three (unaligned): the early-staged slots used exactly once; even
#            and odd first rows; segments at the frame's first and last rows.
#  (12, 20)  two and three steps (clamped), three and four (unaligned), both parities, both frame edges.
#  (15, 25)  as (12, 20) with other cut rows.
#  (13, 30)  an odd height: two and three steps in both copies.
#  (20, 3)   fewer blocks than strips: long segments, blocks that cross from a strip's last row to the next strip's row 0.
#  (40, 7)   long segments with cuts inside the strips.
CLAIMS = {(12, 0): {"f:n1", "c:n1", "f:n2"},
          (12, 30): {"f:n2", "c:n2", "f:n3", "f:even", "f:odd", "c:even", "c:odd", "f:row0", "c:row0", "f:last", "c:last"},
          (12, 20): {"f:n3", "c:n3", "f:even", "f:odd", "c:even", "c:odd", "f:row0", "c:row0", "f:last", "c:last"},
          (15, 25): {"f:n3", "c:n3", "f:odd", "c:odd"},
          (13, 30): {"f:n2", "f:n3", "c:n2", "c:n3", "f:odd", "c:odd"},
          (20, 3): {"next_strip", "f:n4+", "c:n4+", "f:row0", "f:last", "c:last"},
          (40, 7): {"f:n4+", "c:n4+", "f:row0", "c:row0", "f:last", "c:last"}}


@pytest.mark.parametrize("H,gb", sorted(CLAIMS))
def test_segment_lengths(torch_dev, H, gb):
    blocks = _blocks(H, gb)
    assert CLAIMS[(H, gb)] <= _kinds(blocks, H), (H, gb, sorted(_kinds(blocks, H)), blocks)
    if (H, gb) == (12, 0):  # no segment of the clamped strips has a second step
        assert all(s.rows == 1 for b in blocks for s in b if not s.fast)
    L, R = _pair(H)
    _both_modes(torch_dev, ("random", H), L, R, (gb,), f"H={H} random")
    _both_modes(torch_dev, ("random", H), L, R, (gb,), f"H={H} random u=0", u=0)


# ---- radii, disparity ranges ---------------------------------------------------------------------------

@pytest.mark.parametrize("bs,d", [(1, 128), (5, 128), (7, 128), (9, 128), (11, 128), (15, 128), (9, 256)])
def test_block_sizes(torch_dev, bs, d):
    """R = 0, 2, 3, 4, 5: every build of the rotated loop (8 to 11 column chunks, the last one partial at odd R).
    R = 7 (key-tree argmin, sequential loop) and D = 256 (two waves per block) are outside it: untouched guards."""
    R = bs // 2
    W = 256 if d == 128 else 384
    for H, gb in ((12, 0), (13, 0), (20, 3)):
        if gb == 0:  # two and three steps per segment: a block per two rows of the five strips
            gb = 5 * H // 2 - (H == 13)
        blocks = _blocks(H, gb, W=W, R=R, d=d)
        kinds = _kinds(blocks, H)
        if gb > 3:
            assert "f:n2" in kinds and (H != 13 or {"f:n3", "f:odd"} <= kinds), (bs, H, gb, sorted(kinds))
        else:
            assert {"f:n4+", "next_strip"} <= kinds, (bs, H, gb, sorted(kinds))
        L, Rr = _pair(H, W=W, d=d, seed=bs)
        _both_modes(torch_dev, ("random", H, W, d, bs), L, Rr, (gb,), f"block {bs} D={d} H={H}", d=d, bs=bs)


# ---- branches behind the chunks ------------------------------------------------------------------------

def test_odd_disparity_count(torch_dev):
    """D = 127: the high half of the last pair is overwritten through an exec-masked store between the box phase and
    the staging's old place; uniqueness on (the block minima are read again behind the chunks) and off."""
    d = 127
    for H, gb in ((12, 30), (13, 20)):
        kinds = _kinds(_blocks(H, gb, d=d), H)
        assert {"f:n2", "c:n2"} <= kinds if H == 12 else {"f:n3", "f:odd"} <= kinds, sorted(kinds)
        L, R = _pair(H, d=d, seed=127)
        _both_modes(torch_dev, ("random127", H), L, R, (gb,), f"D=127 H={H}", d=d)
        _both_modes(torch_dev, ("random127", H), L, R, (gb,), f"D=127 H={H} u=0", d=d, u=0)


def test_no_subpixel(torch_dev):
    """subpixel off: the sub-pixel stage's quotient is dropped for every pixel."""
    H, gb = 13, 20
    assert {"f:n3", "c:n3", "f:odd"} <= _kinds(_blocks(H, gb), H)
    L, R = _pair(H)
    want = fg.want(("random", H), L, R, M, D, BS, 10, False)
    dL, dR = torch_dev.from_numpy(L).cuda(), torch_dev.from_numpy(R).cuda()
    _run(torch_dev, dL, dR, L.shape, want, "subpixel off", (gb,), uniqueness_ratio=10, subpixel=False, **BASE)


# ---- extreme images ------------------------------------------------------------------------------------

@pytest.mark.parametrize("lv,rv", [(0, 255), (255, 0)])
def test_extreme_images(torch_dev, lv, rv):
    """All-0 against all-255: every column sum is at its bound, 9 * 255, every window sum at 81 * 255 = 20655, and a row
    taken from the wrong slot (0 or 255 apart in every byte) cannot hide.  Then the same with the last rows swapped
    between the views, so that entering and leaving rows differ by the full range."""
    H = 13
    for gb in (30, 20, 3):
        kinds = _kinds(_blocks(H, gb), H)
        assert ({"f:n2", "c:n2"} <= kinds) if gb == 30 else (("f:n3" in kinds) if gb == 20 else ("next_strip" in kinds))
    L = np.full((H, W0), lv, np.uint8)
    R = np.full((H, W0), rv, np.uint8)
    _both_modes(torch_dev, ("flat", lv, rv), L, R, (30, 20, 3), f"flat {lv}/{rv}")
    L2, R2 = L.copy(), R.copy()
    L2[H // 2:], R2[H // 2:] = rv, lv
    L2[::3, 5::7] = 128  # some texture: the minimum is not the same everywhere
    _both_modes(torch_dev, ("step", lv, rv), L2, R2, (30, 20, 3), f"step {lv}/{rv}", u=0)


# ---- batches and handles -------------------------------------------------------------------------------

def test_batch_of_two_frames(torch_dev):
    """Two frames per launch: ten and twenty blocks per frame put a segment boundary on the frame boundary; of three
    blocks the middle one goes on from one frame into the next."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    H = 12
    fr = [_pair(H), _pair(H, seed=1)]
    grids = (20, 40, 3)
    k20, k40, k3 = (_kinds(_blocks(H, g, nf=2), H) for g in grids)
    assert "frame_cut" in k20 and "f:n4+" in k20 and {"frame_cut", "f:n3", "c:n3"} <= k40 and "next_strip" in k3
    assert any(len({s.frame for s in b}) == 2 for b in _blocks(H, 3, nf=2))  # a block with rows of both frames
    dL = torch.from_numpy(np.stack([f[0] for f in fr])).cuda()
    dR = torch.from_numpy(np.stack([f[1] for f in fr])).cuda()
    wants = [fg.want(("random", H) if i == 0 else ("random1", H), L, R, M, D, BS, 10, True) for i, (L, R) in enumerate(fr)]
    for g in grids:
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


def test_three_handles_in_flight(torch_dev):
    """Three in_flight handles on three streams, four frames each, every output checked.  The grids are forced (the
    handles' own rule gives a block per row at this size): segments of two, three and many steps."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    H, NF = 12, 4
    grids = (30, 20, 3)
    assert "f:n2" in _kinds(_blocks(H, 30), H) and "f:n3" in _kinds(_blocks(H, 20), H) and "next_strip" in _kinds(_blocks(H, 3), H)
    fr = [_pair(H, seed=s) for s in range(NF)]
    keys = [("random", H), ("random1", H), ("random2", H), ("random3", H)]
    wants = [fg.want(k, L, R, M, D, BS, 10, True) for k, (L, R) in zip(keys, fr)]
    dev = [(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in fr]
    mts = [HipBlockMatcher(in_flight=True, grid_blocks=g, uniqueness_ratio=10, **BASE) for g in grids]
    sts = [torch.cuda.Stream() for _ in grids]
    fx = [[torch.empty((H, W0), dtype=torch.int16, device="cuda") for _ in range(NF)] for _ in grids]
    fl = [[torch.empty((H, W0), dtype=torch.float32, device="cuda") for _ in range(NF)] for _ in grids]
    torch.cuda.synchronize()
    try:
        for i in range(NF):
            for h, (mt, st) in enumerate(zip(mts, sts)):
                mt.compute_device(dev[i][0], dev[i][1], out_fixed=fx[h][i], out_float=fl[h][i], stream=st)
        torch.cuda.synchronize()
        for h in range(len(grids)):
            for i in range(NF):
                fg.check_maps(fx[h][i], fl[h][i], wants[i], f"handle {h} (grid_blocks={grids[h]}) frame {i}")
    finally:
        for mt in mts:
            mt.close()
