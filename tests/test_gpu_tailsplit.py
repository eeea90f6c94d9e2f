"""Tail of the rotated row loop of the fused SAD pass (csrc/dsx_bm.hip, bm2<R, SAD, 1, 0> with R <= 5):
-DDSX_ROWSTEP_TAILSPLIT, default 1 - both lanes of a pixel key half of the winning 8-disparity block, four elements
each - and the two output stores behind it (estore and the drain's own stores), which this change leaves as they were
and which the cases below cover as well.

What this form can get wrong, and the cases for it:
  * the element order inside the winning block: lane 0 of a pixel keys elements 0 .. 3 and lane 1 elements 4 .. 7, whichever
    lane's slice holds the block, and the pair's minimum must keep "lowest cost, then lowest disparity".  Ties are built
    where each boundary lies: between blocks of one lane's slice (a periodic right view), between the two slices
    (d = 63 against 64), between elements 3 and 4 of one block (the new lane boundary), all costs equal (constant views),
    and winners at d = 0 and d = D - 1, where no sub-pixel step applies.  Every tie is first shown on the CPU in the
    oracle's cost rows;
  * the drain behind a segment, which forms and stores its outputs at once: forced grids cut the strips into segments of
    one and two rows, where the drain is every or every second row;
  * the stages at every radius that runs this loop (R = 0, 2, 3, 4, 5), on frames that hold a strip of the unaligned-dword
    copy ("f:") and clamped strips ("c:") at both edges of the band;
  * D < Dp with an odd D (100 - even, for the padding alone - and 127): the padding costs and the u16 overwrite of the
    last pair's high half stay ordered with the block reads;
  * uniqueness_ratio = 15: that branch reads the blocks again and must not see the new stage's registers;
  * the stores: out_fixed alone, out_float alone, both; outputs that start 2 and 4 bytes into a larger allocation (row
    bases at every alignment a map allows; the elements around the map must stay as they were); input rows further
    apart than W; a batch of three frames (the frame's part of the row base); three in_flight handles on three streams.

Every comparison is bit for bit over all pixels against the C oracle (oracle/cref.py): the int16 x16 map and the float
map - float mode 'fixed' against x16 / 16 (exact in f32), 'parabola' by bit pattern.  The cases hold for both settings
of the switch; the file was run on the default build and on the build with the switch off.
"""
from __future__ import annotations

import numpy as np
import pytest

from depthestimation_amd.synthetic import stereo_pair

import fused_geometry as fg

pytestmark = pytest.mark.gpu

M, D = 0, 128
BASE = dict(cost="sad", disp12_max_diff=-1)
SHAPES = [(24, 224), (40, 330)]
BLOCKS = [1, 5, 7, 9, 11]  # R = 0, 2, 3, 4, 5
# grid_blocks: 0 - a block per strip row (every row is a drain); the others - see test_geometry
GRIDS = {(24, 224): (0, 48, 5), (40, 330): (0, 160, 7)}


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _blocks(H, W, gb, bs, nf=1, d=D):
    return fg.blocks(H, gb, W, M, nf, bs // 2, d)


def _kinds(blocks):
    """'f:' the unaligned-dword copy, 'c:' the clamped one; n1 / n2 / n3+: segments of one, two, three or more rows."""
    return {("f:" if s.fast else "c:") + ("n3+" if s.rows >= 3 else f"n{s.rows}") for b in blocks for s in b}


def _strips(blocks):
    """(x0 of the unaligned strips, of the clamped strips left of them, of the clamped strips right of them)"""
    f = sorted({s.x0 for b in blocks for s in b if s.fast})
    c = sorted({s.x0 for b in blocks for s in b if not s.fast})
    return f, [x for x in c if f and x < f[0]], [x for x in c if f and x > f[-1]]


def _pair(H, W, d=D, seed=0):
    L, R, _ = stereo_pair(H, W, M, d, seed=7100 + 17 * H + W + seed)
    return L, R


def _run(torch, dL, dR, shape, want, what, grids, fmode="fixed", outs="both", **kw):
    from depthestimation_amd.matcher import HipBlockMatcher
    for g in grids:
        mt = HipBlockMatcher(grid_blocks=g, float_mode=fmode, **kw)
        try:
            fx = torch.empty(shape, dtype=torch.int16, device="cuda") if outs in ("both", "fixed") else None
            fl = torch.empty(shape, dtype=torch.float32, device="cuda") if outs in ("both", "float") else None
            mt.compute_device(dL, dR, out_fixed=fx, out_float=fl)
            torch.cuda.synchronize()
            fg.check_maps(fx, fl, want, f"{what} grid_blocks={g} outs={outs}", fmode)
        finally:
            mt.close()


def _case(torch, key, L, R, grids, what, bs=9, d=D, u=0, fmodes=("fixed", "parabola"), sp=True, **run_kw):
    kw = dict(BASE, min_disp=M, num_disp=d, block_size=bs, uniqueness_ratio=u, subpixel=sp)
    want = fg.want(key, L, R, M, d, bs, u, sp)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    for fmode in fmodes:
        _run(torch, dL, dR, L.shape, want, f"{what} {fmode}", grids, fmode=fmode, **run_kw, **kw)
    return want


# ---- geometry ------------------------------------------------------------------------------------------

def test_geometry():
    """Every frame holds an unaligned strip and clamped strips left of it (the band starts inside a strip that reaches
    back over the row's start); 330 columns end in a ragged clamped strip at every radius, 224 columns in a clamped one
    for R >= 2 (at R = 0 its last strip, x0 = 192, still loads whole dwords).  The forced grids hold one-row and two-row
    segments of the unaligned copy, and segments of many rows."""
    for (H, W) in SHAPES:
        for bs in BLOCKS:
            f, left, right = _strips(_blocks(H, W, 0, bs))
            assert f and left, (H, W, bs, f, left)
            assert right or (W == 224 and bs == 1), (H, W, bs, f, right)
            g1, g2, g3 = GRIDS[H, W]
            assert {"f:n1", "c:n1"} <= _kinds(_blocks(H, W, g1, bs)), (H, W, bs)
            assert {"f:n2", "c:n2", "c:n1"} <= _kinds(_blocks(H, W, g2, bs)), (H, W, bs)
            assert {"f:n3+", "c:n3+"} <= _kinds(_blocks(H, W, g3, bs)), (H, W, bs)


# ---- every radius of the rotated loop ------------------------------------------------------------------

@pytest.mark.parametrize("bs", BLOCKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_frames(torch_dev, shape, bs):
    H, W = shape
    L, R = _pair(H, W)
    _case(torch_dev, ("random", H, W), L, R, GRIDS[shape], f"{H}x{W} block {bs}", bs=bs)


# ---- tie order -----------------------------------------------------------------------------------------

TH, TW = SHAPES[0]
TX0 = 160  # the unaligned strip of the 224-column frame, R <= 5


def _noise(seed):
    return np.random.default_rng(seed).integers(0, 256, (TH, TW), dtype=np.uint8)


def _periodic(seed, period):
    """Noise that repeats every `period` columns."""
    return np.ascontiguousarray(np.tile(_noise(seed)[:, :period], (1, TW // period + 1))[:, :TW])


def _shift(R, s):
    """L with L(x) = R(x - s) (columns left of s: R's first column, as the clamped search reads it)"""
    return np.ascontiguousarray(R[:, np.clip(np.arange(R.shape[1]) - s, 0, R.shape[1] - 1)])


def _ties(name):
    """(L, R, d_lo, d_hi): views whose cost rows hold equal minima at d_lo and d_hi (and nowhere below d_lo)."""
    if name == "constant":  # every cost is 0
        return np.full((TH, TW), 77, np.uint8), np.full((TH, TW), 77, np.uint8), 0, D - 1
    if name == "blocks":  # right view of period 24, left view 2 columns on: zero cost at d = 2, 26, 50 (blocks 0, 3, 6
        # of lane 0's slice) and 74, 98, 122 (blocks 9, 12, 15, lane 1's)
        R = _periodic(1, 24)
        return _shift(R, 2), R, 2, 26
    if name == "blocks_hi":  # period 24 again, 18 columns on: d = 18, 42 in blocks 2, 5; 66, 90, 114 in lane 1's slice
        R = _periodic(2, 24)
        return _shift(R, 18), R, 18, 42
    if name in ("63/64", "35/36", "99/100"):
        # right view: an even triangle wave of period 160 (> D: one pair of minima in range) whose phase moves with
        # the row; the left pixel lies midway between the right pixels it meets at d and d + 1, so every term of the two
        # costs is the same, and on the wave's slopes a term is |2 (d' - d) - 1| at disparity d'
        d = int(name.split("/")[0])
        x, y = np.meshgrid(np.arange(TW), np.arange(TH))
        R = (40 + 2 * np.abs((x + 13 * y) % 160 - 80)).astype(np.uint8)
        L = ((_shift(R, d).astype(np.int64) + _shift(R, d + 1)) // 2).astype(np.uint8)
        return L, R, d, d + 1
    if name in ("first", "last"):  # one zero-cost winner at d = 0 / D - 1: no sub-pixel step
        d = 0 if name == "first" else D - 1
        R = _periodic(9, 160)
        return _shift(R, d), R, d, d
    raise KeyError(name)


@pytest.mark.parametrize("bs", [9, 5])
@pytest.mark.parametrize("name", ["constant", "blocks", "blocks_hi", "63/64", "35/36", "99/100", "first", "last"])
def test_tie_order(torch_dev, name, bs):
    from oracle.stereo_bm import cost_volume
    L, R, dlo, dhi = _ties(name)
    # the oracle's cost rows in the band's part of the unaligned strip hold the tie: both disparities at the row's
    # minimum, none below d_lo
    C = cost_volume(L, R, M, D, bs, "sad")[:, TX0:TX0 + fg.TX]
    cmin = C.min(axis=2)
    assert np.all(C[:, :, dlo] == cmin) and np.all(C[:, :, dhi] == cmin), name
    assert np.all(C[:, :, :dlo] > cmin[..., None]), name
    if name == "constant":
        assert np.all(C == 0)
    if name in ("blocks", "blocks_hi"):  # the same minimum in three blocks of lane 0's slice and three of lane 1's
        for d in range(dlo, D, 24):
            assert np.all(C[:, :, d] == cmin), (name, d)
        assert dlo // 8 != dhi // 8 and dhi < 64
    if "/" in name:  # two winners only
        assert np.all((C == cmin[..., None]).sum(axis=2) == 2), name
    assert TX0 in _strips(_blocks(TH, TW, 0, bs))[0]
    want = _case(torch_dev, ("tie", name), L, R, GRIDS[TH, TW], f"tie {name} block {bs}", bs=bs)
    # the oracle takes the lowest disparity of the tie: no sub-pixel step at d = 0 and D - 1; a step of at most half
    # a disparity between tied blocks; C(d + 1) = C(d) < C(d - 1) puts the parabola's vertex at d + 1/2, 8 in x16
    w = want["fixed"][:, TX0:TX0 + fg.TX].astype(np.int64)
    if name in ("constant", "first", "last"):
        assert np.all(w == 16 * dlo), name
    elif "/" in name:
        assert np.all(w == 16 * dlo + 8), name
    else:
        assert np.all(np.abs(w - 16 * dlo) <= 8), name


# ---- disparity range -----------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [100, 127])
@pytest.mark.parametrize("bs", [9, 5, 1])
def test_padded_and_odd_range(torch_dev, d, bs):
    """D = 100: 28 padding disparities behind the tile stores.  D = 127: the last pair's high half is overwritten with
    the padding cost behind them.  Constant views put every real cost at 0, below the padding, up to d = D - 1."""
    H, W = SHAPES[0]
    f, left, _ = _strips(fg.blocks(H, 0, W, M, 1, bs // 2, d))
    assert f and left, (d, bs)
    L, R = _pair(H, W, d=d, seed=d)
    _case(torch_dev, ("random", H, W, d), L, R, GRIDS[H, W], f"D={d} block {bs}", bs=bs, d=d)
    Rr = _periodic(d, 160)
    want = _case(torch_dev, ("last", d), _shift(Rr, d - 1), Rr, (0, 5), f"D={d} winner D-1 block {bs}", bs=bs, d=d,
                 fmodes=("fixed",))
    if bs > 1:  # (a one-pixel block meets its value at lower disparities too)
        assert np.all(want["fixed"][:, f[0]:f[0] + fg.TX] == 16 * (d - 1))


# ---- uniqueness ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("bs", [9, 7])
def test_uniqueness_15(torch_dev, bs):
    H, W = SHAPES[1]
    L, R = _pair(H, W, seed=15)
    want = _case(torch_dev, ("random", H, W, "u"), L, R, GRIDS[H, W], f"u=15 block {bs}", bs=bs, u=15)
    band = want["fixed"][:, D - 1:]
    assert (band == -16).any() and (band != -16).any()  # the branch decides both ways
    # tied winners: the second minimum is the first (zero against zero passes the ratio test; next to d it is left out)
    for name in ("blocks", "99/100"):
        Lt, Rt, _, _ = _ties(name)
        _case(torch_dev, ("tie", name), Lt, Rt, GRIDS[TH, TW], f"u=15 tie {name} block {bs}", bs=bs, u=15)


# ---- outputs -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("outs", ["fixed", "float", "both"])
@pytest.mark.parametrize("fmode", ["fixed", "parabola"])
def test_one_output_or_both(torch_dev, outs, fmode):
    H, W = SHAPES[0]
    L, R = _pair(H, W)
    for bs in (9, 5):
        _case(torch_dev, ("random", H, W), L, R, GRIDS[H, W], f"block {bs}", bs=bs, fmodes=(fmode,), outs=outs)


@pytest.mark.parametrize("pad", [1, 3, 32])
def test_input_row_stride(torch_dev, pad):
    """Input rows W + pad bytes apart, noise between them."""
    torch = torch_dev
    H, W = SHAPES[0]
    L, R = _pair(H, W)
    rng = np.random.default_rng(pad)
    views = []
    for img in (L, R):
        host = rng.integers(0, 256, (H, W + pad), dtype=np.uint8)
        host[:, :W] = img
        buf = torch.from_numpy(host).cuda()
        views.append(buf[:, :W])
    assert views[0].stride(0) == W + pad and not views[0].is_contiguous()
    for bs in (9, 1):
        want = fg.want(("random", H, W), L, R, M, D, bs, 0)
        _run(torch, views[0], views[1], (H, W), want, f"stride W+{pad} block {bs}", GRIDS[H, W], uniqueness_ratio=0,
             min_disp=M, num_disp=D, block_size=bs, **BASE)


@pytest.mark.parametrize("off", [2, 4])
def test_outputs_inside_a_larger_allocation(torch_dev, off):
    """The maps start `off` bytes (the float map: 4 and 8) into larger buffers, so the row bases take every
    alignment a map allows; the elements in front of and behind the maps keep their values."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    H, W = SHAPES[0]
    L, R = _pair(H, W)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    e16, e32 = off // 2, off // 2  # elements: 2 / 4 bytes of int16, 4 / 8 bytes of float
    for bs in (9, 5):
        want = fg.want(("random", H, W), L, R, M, D, bs, 0)
        for g in GRIDS[H, W]:
            b16 = torch.full((H * W + 8,), 12345, dtype=torch.int16, device="cuda")
            b32 = torch.full((H * W + 8,), -7.5, dtype=torch.float32, device="cuda")
            fx, fl = b16[e16:e16 + H * W].view(H, W), b32[e32:e32 + H * W].view(H, W)
            assert fx.data_ptr() == b16.data_ptr() + off and fl.data_ptr() == b32.data_ptr() + 2 * off
            mt = HipBlockMatcher(grid_blocks=g, uniqueness_ratio=0, min_disp=M, num_disp=D, block_size=bs, **BASE)
            try:
                mt.compute_device(dL, dR, out_fixed=fx, out_float=fl)
                torch.cuda.synchronize()
            finally:
                mt.close()
            fg.check_maps(fx, fl, want, f"offset {off} block {bs} grid_blocks={g}")
            h16, h32 = b16.cpu().numpy(), b32.cpu().numpy()
            assert np.all(h16[:e16] == 12345) and np.all(h16[e16 + H * W:] == 12345)
            assert np.all(h32[:e32] == -7.5) and np.all(h32[e32 + H * W:] == -7.5)


def test_batch_of_three_frames(torch_dev):
    """Three frames per launch: the frame's part of the row base; blocks that go on from one frame into the next."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    (H, W), NF = SHAPES[0], 3
    grids = (0, 144, 5)
    assert any(len({s.frame for s in b}) == 2 for b in _blocks(H, W, 5, 9, nf=NF))
    assert "f:n2" in _kinds(_blocks(H, W, 144, 9, nf=NF))
    fr = [_pair(H, W, seed=s) for s in range(NF)]
    dL = torch.from_numpy(np.stack([f[0] for f in fr])).cuda()
    dR = torch.from_numpy(np.stack([f[1] for f in fr])).cuda()
    for bs in (9, 5):
        wants = [fg.want(("random", H, W, i), L, R, M, D, bs, 0) for i, (L, R) in enumerate(fr)]
        for g in grids:
            mt = HipBlockMatcher(grid_blocks=g, uniqueness_ratio=0, min_disp=M, num_disp=D, block_size=bs, **BASE)
            try:
                fx = torch.empty((NF, H, W), dtype=torch.int16, device="cuda")
                fl = torch.empty((NF, H, W), dtype=torch.float32, device="cuda")
                mt.compute_batch_device(dL, dR, out_fixed=fx, out_float=fl)
                torch.cuda.synchronize()
                for i in range(NF):
                    fg.check_maps(fx[i], fl[i], wants[i], f"batch block {bs} grid_blocks={g} frame={i}")
            finally:
                mt.close()


def test_three_handles_in_flight(torch_dev):
    """Three in_flight handles on three streams, four frames each, every output checked; the grids are forced."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    (H, W), NF = SHAPES[0], 4
    grids = GRIDS[H, W]
    fr = [_pair(H, W, seed=s) for s in range(NF)]
    wants = [fg.want(("random", H, W, i), L, R, M, D, 9, 0) for i, (L, R) in enumerate(fr)]
    dev = [(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in fr]
    mts = [HipBlockMatcher(in_flight=True, grid_blocks=g, uniqueness_ratio=0, min_disp=M, num_disp=D, block_size=9, **BASE)
           for g in grids]
    sts = [torch.cuda.Stream() for _ in grids]
    fx = [[torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(NF)] for _ in grids]
    fl = [[torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(NF)] for _ in grids]
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
