"""Left tail of the fused pass (csrc/dsx_bm.hip, pair layout): its branch-free sub-pixel quotient
(csrc/dsx_subpix.h), and segments of every short length.  The length cases were written for a tail that ran once
per two rows, a form that was rejected and removed from the source; they were run on that build and
on the shipped one, and hold for the shipped tail, which runs once per row.

The paired tail left a row step's scan results (winner, its cost, valid bit, the two neighbour costs) in both
lanes of a pixel; the first row of a pair kept them across the next step, the second row's tail finished both
rows at once (lane h = 0 the kept row, h = 1 its own), and a segment's unpaired last row ran the tail on the
h = 0 lanes alone.  Rows were paired by their offset in the segment, so what decided the form was the segment
length: the cases below are chosen by it, from the launch geometry restated in tests/fused_geometry.py, and guard
a tail that holds anything across row steps.  The quotient's cases are the tail classes (quotients 8, 0 and
below 0, rows that take no step) and disparity ranges of one, two and four waves per block.

Every comparison is bit for bit over all pixels against the C oracle (oracle/cref.py): the int16 x16 map and
the float map - float mode 'fixed' against x16 / 16 (exact in f32), 'parabola' by bit pattern.

Base: D = 128, block 9, W = 256: the valid band starts at x = 127, strips 3..7 run, x0 = 160 and 192 with
the unaligned-dword loads and 96, 128, 224 with clamped bytes, so both copies of the row loop run.

An interior winner is the LOWEST disparity of minimal cost, so cm > cb always: of the quotient's extremes
only cm - cp = +den (cp == cb, a tie with the next disparity, q = 8) can occur, and den >= 1 without the
clamp; 'cm == cp == cb' exists only as a flat cost row, whose winner is d = 0 and takes no step (the tail
then drops neighbour costs read at d = -1).  The class test asserts what can occur.
"""
from __future__ import annotations

import numpy as np
import pytest

from depthestimation_amd.synthetic import binary_pair, stereo_pair
from oracle.cref import CRef
from oracle.stereo_bm import cost_volume

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


@pytest.fixture(scope="module")
def cref():
    return CRef()


def _segments(H, gb, W=W0, m=M, nf=1, R=BS // 2):
    """Lengths of the segments (runs of rows of one strip in one block) of a left-pass launch."""
    return [s.rows for b in fg.blocks(H, gb, W, m, nf, R, D) for s in b]


def _kinds(segs):
    return {k for k, f in (("one", lambda n: n == 1), ("even", lambda n: n % 2 == 0), ("odd3", lambda n: n % 2 == 1 and n >= 3))
            if any(f(n) for n in segs)}


def _run(torch, L, R, want, what, grids, fmode="fixed", outs="both", **kw):
    from depthestimation_amd.matcher import HipBlockMatcher
    for g in grids:
        mt = HipBlockMatcher(grid_blocks=g, float_mode=fmode, **kw)
        try:
            fx = torch.empty(L.shape, dtype=torch.int16, device="cuda") if outs in ("both", "fixed") else None
            fl = torch.empty(L.shape, dtype=torch.float32, device="cuda") if outs in ("both", "float") else None
            mt.compute_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), out_fixed=fx, out_float=fl)
            torch.cuda.synchronize()
            fg.check_maps(fx, fl, want, f"{what} grid_blocks={g}", fmode)
        finally:
            mt.close()


def _pair(H, W=W0, m=M, seed=0):
    L, R, _ = stereo_pair(H, W, m, D, seed=4100 + 13 * H + seed)
    return L, R


# ---- segment parities --------------------------------------------------------------------------------

# What each (H, grid_blocks) must contain.  Whole strips at 1 and 5 blocks.  With fewer blocks than strips (3)
# the blocks take an even split of the linearised rows and cross strip boundaries: H = 7 gives 7, 4 | 3, 7, 2
# | 5, 7.  From 5 blocks on every block stays inside one strip, so 7 blocks split two of the strips, as 3 + 4
# at H = 7 and 4 + 4 at H = 8 (not the 5-row blocks an even split would give).  With a block per row
# (35, and 0 = the resident capacity, which the launcher clips to the row count) the clamped strips get more
# blocks than rows and the others fewer: single rows, where every tail is the unpaired form, and pairs.
CLAIMS = {(7, 1): {"odd3"}, (8, 1): {"even"}, (7, 3): {"even", "odd3"}, (8, 3): {"even", "odd3"},
          (7, 5): {"odd3"}, (8, 5): {"even"}, (7, 7): {"even", "odd3"}, (8, 7): {"even"},
          (7, 35): {"one", "even"}, (8, 35): {"one", "even"}, (7, 0): {"one", "even"}, (8, 0): {"one", "even"}}


@pytest.mark.parametrize("gb", [0, 1, 3, 5, 7, 35])
@pytest.mark.parametrize("H", [7, 8])
def test_segment_parities(torch_dev, cref, H, gb):
    segs = _segments(H, gb)
    assert CLAIMS[(H, gb)] <= _kinds(segs), (H, gb, segs)
    if gb in (1, 5):
        assert set(segs) == {H}
    if (H, gb) == (7, 3):
        assert segs == [7, 4, 3, 7, 2, 5, 7]
    if (H, gb) == (7, 7):
        assert sorted(segs) == [3, 3, 4, 4, 7, 7, 7]
    for name, (L, R) in (("random", _pair(H)), ("binary", binary_pair(H, W0, M, D, seed=77 + H)[:2])):
        for u in (0, 10):
            want = cref(L, R, M, D, BS, "sad", u, -1, True)
            for fmode in ("fixed", "parabola"):
                _run(torch_dev, L, R, want, f"H={H} u={u} {fmode} input={name}", (gb,), fmode=fmode, uniqueness_ratio=u, **BASE)


def test_every_segment_kind_is_covered():
    kinds = set()
    for (H, gb) in CLAIMS:
        kinds |= _kinds(_segments(H, gb))
    assert kinds == {"one", "even", "odd3"}


# ---- nothing kept across segments, strips or frames ------------------------------------------------------

@pytest.mark.parametrize("H", [7, 8])
def test_no_leak_across_frames(torch_dev, cref, H):
    """Two frames per launch, frame 1 = frame 0 with the left image moved by one column (every disparity + 1):
    a kept row finished in the wrong segment or frame changes the result.  The same frames singly as well."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    L0, R0 = _pair(H)
    L1 = np.roll(L0, 1, axis=1)
    L1[:, 0] = L0[:, 0]
    fr = [(L0, R0), (L1, R0.copy())]
    dL = torch.from_numpy(np.stack([f[0] for f in fr])).cuda()
    dR = torch.from_numpy(np.stack([f[1] for f in fr])).cuda()
    for u in (0, 10):
        wants = [cref(L, R, M, D, BS, "sad", u, -1, True) for L, R in fr]
        assert np.any(wants[0]["fixed"] != wants[1]["fixed"])
        for g in (0, 1, 3, 7, 10):
            segs = _segments(H, g, nf=2)
            assert sum(segs) == 2 * 5 * H
            mt = HipBlockMatcher(grid_blocks=g, uniqueness_ratio=u, **BASE)
            try:
                fx = torch.empty((2, H, W0), dtype=torch.int16, device="cuda")
                fl = torch.empty((2, H, W0), dtype=torch.float32, device="cuda")
                mt.compute_batch_device(dL, dR, out_fixed=fx, out_float=fl)
                torch.cuda.synchronize()
                for i in range(2):
                    fg.check_maps(fx[i], fl[i], wants[i], f"batch H={H} u={u} grid_blocks={g} frame={i}")
                for i in range(2):
                    f1 = torch.empty((H, W0), dtype=torch.int16, device="cuda")
                    mt.compute_device(dL[i], dR[i], out_fixed=f1)
                    torch.cuda.synchronize()
                    fg.check_maps(f1, None, wants[i], f"single H={H} u={u} grid_blocks={g} frame={i}")
            finally:
                mt.close()


# ---- tail inputs that differ between the rows of a pair --------------------------------------------------

def _class_frame(H=44, W=W0):
    """Bands of rows, each taller than the 9-row window: two unrelated binary textures (interior winners, costs
    in steps of 255 with ties between neighbouring disparities), constant rows (flat costs), identical images
    (winner d = 0), a grey texture displaced by 127 = D - 1 (the last disparity wins)."""
    rng = np.random.default_rng(5)
    Rr = rng.integers(0, 256, (H, W + 160), dtype=np.uint8)
    R = Rr[:, 160:].copy()
    L = R.copy()

    def shifted(rows, d):
        L[rows] = Rr[rows, 160 - d:160 - d + W]

    b0, b1, b2, b3 = slice(0, 11), slice(11, 22), slice(22, 33), slice(33, 44)
    R[b0] = np.where(Rr[b0, 160:] > 127, 255, 0)
    L[b0] = rng.integers(0, 2, (11, W), dtype=np.uint8) * 255
    R[b1] = 93
    L[b1] = 93
    # b2: identical images
    shifted(b3, D - 1)
    return L, R


def _classes(L, R):
    """Per pixel of the valid band: (row parity, class) from the block costs."""
    vol = cost_volume(L, R, M, D, BS, "sad").astype(np.int64)  # [H, W, D]
    H, W = L.shape
    b = vol.argmin(axis=2)
    yy, xx = np.mgrid[0:H, 0:W]
    cb = vol[yy, xx, b]
    cm = vol[yy, xx, np.maximum(b - 1, 0)]
    cp = vol[yy, xx, np.minimum(b + 1, D - 1)]
    band = (xx >= M + D - 1) & (xx <= W - 1 + M)
    inner = (b > 0) & (b < D - 1)
    den = np.maximum(cm + cp - 2 * cb, 1)
    assert not np.any(inner & band & (cm <= cb)), "an interior winner is the lowest minimum: cm > cb"
    cls = {
        "first": band & (b == 0),
        "last": band & (b == D - 1),
        "interior": band & inner,
        "flat": band & (vol.max(axis=2) == vol.min(axis=2)),
        "q8": band & inner & (cm - cp == den),
        "q0": band & inner & (cm == cp),
        "qneg": band & inner & (cm < cp),
    }
    return {k: {int(p) for p in np.unique(yy[v] & 1)} for k, v in cls.items()}


@pytest.fixture(scope="module")
def class_case(cref):
    L, R = _class_frame()
    got = _classes(L, R)
    for k, par in got.items():
        assert par == {0, 1}, f"class {k} must occur on even and on odd rows, got {par}"
    return L, R, {(u, sp): cref(L, R, M, D, BS, "sad", u, -1, sp) for u in (0, 10) for sp in (True, False)}


@pytest.mark.parametrize("u", [0, 10])
@pytest.mark.parametrize("fmode", ["fixed", "parabola"])
def test_tail_classes(torch_dev, class_case, fmode, u):
    """Rows whose tails differ (no step at d = 0 and d = D - 1, flat costs, interior winners with quotients 8,
    0 and below 0), in both positions of a pair: 44 rows in one block, in 3 blocks (segments of 29 and 15 rows,
    which start at odd rows too), in 7 and in single rows and pairs."""
    L, R, wants = class_case
    assert _segments(44, 3) == [44, 29, 15, 44, 14, 30, 44] and {"one", "even"} <= _kinds(_segments(44, 0))
    _run(torch_dev, L, R, wants[(u, True)], f"classes u={u} {fmode}", (1, 3, 7, 0), fmode=fmode, uniqueness_ratio=u, **BASE)


# ---- store forms -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("outs", ["fixed", "float", "both"])
@pytest.mark.parametrize("fmode", ["fixed", "parabola"])
def test_store_forms(torch_dev, class_case, outs, fmode):
    L, R, wants = class_case
    for u in (0, 10):
        _run(torch_dev, L[:15], R[:15], _crop(wants, L, R, u, True, 15), f"outs={outs} {fmode} u={u}", (1, 3, 7), fmode=fmode, outs=outs,
             uniqueness_ratio=u, **BASE)


_CROPS = {}


def _crop(wants, L, R, u, sp, H):
    """Oracle of the first H rows (its own frame: the window clamps at row H - 1), computed once."""
    key = (u, sp, H)
    if key not in _CROPS:
        _CROPS[key] = CRef()(L[:H], R[:H], M, D, BS, "sad", u, -1, sp)
    return _CROPS[key]


@pytest.mark.parametrize("u", [0, 10])
def test_no_subpixel(torch_dev, class_case, u):
    L, R, wants = class_case
    _run(torch_dev, L, R, wants[(u, False)], f"subpixel off u={u}", (1, 7, 0), uniqueness_ratio=u, subpixel=False, **BASE)


# ---- edges -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 2, 7])
@pytest.mark.parametrize("W,m", [(250, 0), (256, 3), (250, 3)])
def test_edges(torch_dev, cref, H, W, m):
    """A partial last strip, a band moved by min_disp, frames of one and two rows."""
    L, R, _ = stereo_pair(H, W, m, D, seed=900 + H + W + m)
    kw = dict(BASE, min_disp=m)
    for u in (0, 10):
        want = cref(L, R, m, D, BS, "sad", u, -1, True)
        for fmode in ("fixed", "parabola"):
            _run(torch_dev, L, R, want, f"H={H} W={W} m={m} u={u} {fmode}", (0, 1, 3), fmode=fmode, uniqueness_ratio=u, **kw)


# ---- other builds ----------------------------------------------------------------------------------------

def test_clamped_copy(torch_dev, cref):
    """W = 160: strips 3 and 4 only, both on the clamped-byte copy of the row loop (no strip passes the
    unaligned-load test x0 in [133, 124])."""
    H, W = 9, 160
    L, R, _ = stereo_pair(H, W, M, D, seed=31)
    for u in (0, 10):
        want = cref(L, R, M, D, BS, "sad", u, -1, True)
        _run(torch_dev, L, R, want, f"clamped u={u}", (0, 1, 3), fmode="parabola", uniqueness_ratio=u, **BASE)


@pytest.mark.parametrize("H", [7, 8])
@pytest.mark.parametrize("Dw", [192, 131, 300])
def test_multiwave_blocks(torch_dev, cref, H, Dw):
    """Two and four waves per block at W = 320 (the left pass of every pair layout takes the branch-free
    quotient): whole strips, blocks that cross strips, single rows."""
    W = 320 + (Dw > 256) * 128
    L, R, _ = stereo_pair(H, W, M, Dw, seed=600 + Dw + H)
    Lb, Rb, _ = binary_pair(H, W, M, Dw, seed=700 + Dw + H)
    kw = dict(BASE, num_disp=Dw)
    for name, (l, r) in (("random", (L, R)), ("binary", (Lb, Rb))):
        for u in (0, 10):
            want = cref(l, r, M, Dw, BS, "sad", u, -1, True)
            for fmode in ("fixed", "parabola"):
                _run(torch_dev, l, r, want, f"D={Dw} H={H} u={u} {fmode} input={name}", (0, 1, 2, 3), fmode=fmode,
                     uniqueness_ratio=u, **kw)


def test_three_in_flight(torch_dev, cref):
    """Three in_flight handles on three streams, two rounds, each with its own frame and oracle."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    H = 15
    fr = [_pair(H, seed=s) for s in (0, 1)] + [binary_pair(H, W0, M, D, seed=3)[:2]]
    wants = [cref(L, R, M, D, BS, "sad", 0, -1, True) for L, R in fr]
    dev = [(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in fr]
    handles = [HipBlockMatcher(in_flight=True, uniqueness_ratio=0, **BASE) for _ in range(3)]
    streams = [torch.cuda.Stream() for _ in range(3)]
    fx = [torch.empty((H, W0), dtype=torch.int16, device="cuda") for _ in range(6)]
    fl = [torch.empty((H, W0), dtype=torch.float32, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    try:
        for i in range(6):
            handles[i % 3].compute_device(*dev[i % 3], out_fixed=fx[i], out_float=fl[i], stream=streams[i % 3])
        torch.cuda.synchronize()
        for i in range(6):
            fg.check_maps(fx[i], fl[i], wants[i % 3], f"in_flight handle {i % 3} call {i // 3}")
    finally:
        for h in handles:
            h.close()
