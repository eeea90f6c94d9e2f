"""Three-column group sums of the rotated 9x9 and 3x3 row loops of the fused pass (csrc/dsx_bm.hip, CG in bm2_segment;
-DDSX_ROWSTEP_COLGROUP, default 1).  The strips that load unaligned dwords ("f:" below) of bm2<4, SAD, 1, 0> and
bm2<1, SAD, 1, 0> keep, per column c, the sum of columns c, c + 1, c + 2 over the live rows: the staged words are
3-byte windows built from a lane's dword and its neighbour's, one v_sad_u8 adds a 3-column term, the single-column sums
of the segment init are summed into groups once per segment, and a 9-column box is one v_add3_u32.  The other strips
("c:", clamped bytes) keep the single-column form.

What this form can get wrong, and the cases for it:
  * the window bytes that come from the neighbour lane's dword, for searched entries and reference columns, at every
    alignment of the row pointer (views at byte offsets 0 - 3 with strides W .. W + 3, rows that end their allocation)
    and for values that change with a period that is no multiple of 4;
  * the hand-over from the init's column sums to the group sums: it runs once per segment, so forced grids cut the
    strips into segments of one, two, three and many rows that start at several rows, the frame's first and last ones
    (clamped rows) included;
  * a carry between the two u16 halves: all-0 against all-255 puts every half of a group sum at 3 * 9 * 255 = 6,885
    and every half of a box sum at 20,655;
  * the boundary between the two forms (a block goes on from a clamped strip into an unaligned one and back), a ragged
    clamped strip behind the last unaligned one (W = 288), the odd-D overwrite (D = 127) and the padding lanes (D = 96)
    behind the tile stores, min_disp != 0, the uniqueness re-read of the block minima, both float modes, a batch of
    three frames and three handles in flight on three streams;
  * block 3 (R = 1), where a group sum is the box sum.

Every comparison is bit for bit over all pixels against the C oracle (oracle/cref.py): the int16 x16 map and the
float map - float mode 'fixed' against x16 / 16 (exact in f32), 'parabola' by bit pattern.  The cases hold for both
settings of the switch; the file was run on both builds.

Base: D = 128, block 9, W = 256, H = 48: the valid band starts at x = 127, strips 3 .. 7 run, x0 = 160 and 192 on the
unaligned-dword copy and 96, 128, 224 on the clamped one.
"""
from __future__ import annotations

import numpy as np
import pytest

from depthestimation_amd.synthetic import stereo_pair

import fused_geometry as fg

pytestmark = pytest.mark.gpu

M, D, BS, W0, H0 = 0, 128, 9, 256, 48
BASE = dict(cost="sad", disp12_max_diff=-1)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _blocks(H, gb, W=W0, m=M, nf=1, bs=BS, d=D):
    """Per block of a left-pass launch of the pair layout (64 < d <= 128) its segments (fused_geometry.Seg), in
    order."""
    return fg.blocks(H, gb, W, m, nf, bs // 2, d)


def _kinds(blocks, H):
    """Segment classes of a launch; 'f:' marks the unaligned-dword copy, 'c:' the clamped one.

    n1 / n2 / n3 / n4+: segments of one, two, three, four or more rows.  row0 / last: a segment that starts at row 0 /
    ends at row H - 1 (its init, or its last steps, take clamped rows).  mid: a segment that starts at a row >= 5
    (every init row is a row of its own).  even / odd: the parity of a first row.  c>f / f>c: a block that goes on
    from a clamped strip into an unaligned one / back."""
    k = set()
    for b in blocks:
        for s in b:
            p = "f:" if s.fast else "c:"
            n = s.rows
            k.add(p + ("n4+" if n >= 4 else f"n{n}"))
            k.add(p + ("odd" if s.y0 & 1 else "even"))
            if s.y0 == 0:
                k.add(p + "row0")
            if s.y0 >= 5:
                k.add(p + "mid")
            if s.y0 + n == H:
                k.add(p + "last")
        for p, q in zip(b, b[1:]):
            if p.fast != q.fast:
                k.add("f>c" if p.fast else "c>f")
    return k


def _fast_x0(blocks):
    return sorted({s.x0 for b in blocks for s in b if s.fast})


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


def _pair(H=H0, W=W0, m=M, d=D, seed=0):
    L, R, _ = stereo_pair(H, W, m, d, seed=4400 + 13 * H + seed)
    return L, R


def _all_modes(torch, key, L, R, grids, what, m=M, d=D, bs=BS, us=(0, 10), fmodes=("fixed", "parabola")):
    """Uniqueness off and 10 (no LR check: the block minima are read again behind the chunks), both float modes."""
    kw = dict(BASE, min_disp=m, num_disp=d, block_size=bs)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    for u in us:
        want = fg.want(key, L, R, m, d, bs, u)
        for fmode in fmodes:
            _run(torch, dL, dR, L.shape, want, f"{what} u={u} {fmode}", grids, fmode=fmode, uniqueness_ratio=u, **kw)


# ---- base shape and forced grids -----------------------------------------------------------------------

# grid_blocks -> classes the launch must contain (H = 48, five strips, 240 strip rows)
#   0    a block per row: every segment is its init and one box phase - the hand-over alone, at every row of the frame
#   120  two rows per block in the unaligned strips: the staged windows are used exactly once per segment
#   77   three and four rows, odd and even first rows
#   31   segments of several rows that start inside the strips
#   7    long segments
#   3    fewer blocks than strips: blocks that cross between the two forms
CLAIMS = {0: {"f:n1", "c:n1", "f:row0", "f:last", "f:mid", "f:odd", "f:even"},
          120: {"f:n2", "f:row0", "f:last", "f:mid"},
          77: {"f:n3", "f:n4+", "f:odd", "f:even", "f:mid"},
          31: {"f:n4+", "c:n4+", "f:mid", "f:row0", "f:last"},
          7: {"f:n4+", "c:n4+", "f:mid"},
          3: {"f:n4+", "c:n4+", "c>f", "f>c", "f:row0", "f:last"}}


def test_base_geometry():
    """Strips 3, 4 and 7 (x0 = 96, 128, 224) take the clamped copy, strips 5 and 6 (x0 = 160, 192) the unaligned one,
    and every forced grid holds the segment classes it is there for."""
    blocks = _blocks(H0, 0)
    assert _fast_x0(blocks) == [160, 192]
    assert sorted({s.x0 for b in blocks for s in b if not s.fast}) == [96, 128, 224]
    for gb, claim in CLAIMS.items():
        kinds = _kinds(_blocks(H0, gb), H0)
        assert claim <= kinds, (gb, sorted(claim - kinds), sorted(kinds))
    # block 3: the same strips
    assert _fast_x0(_blocks(H0, 0, bs=3)) == [160, 192]


@pytest.mark.parametrize("gb", sorted(CLAIMS))
def test_base_shape(torch_dev, gb):
    L, R = _pair()
    _all_modes(torch_dev, "random", L, R, (gb,), "base")


@pytest.mark.parametrize("gb", sorted(CLAIMS))
def test_block_3(torch_dev, gb):
    """R = 1: 32 groups for 34 columns, the group sum is the box sum (no add in the box phase)."""
    assert CLAIMS[gb] - {"c>f", "f>c"} <= _kinds(_blocks(H0, gb, bs=3), H0) | ({"c:n1"} if gb == 0 else set())
    L, R = _pair()
    _all_modes(torch_dev, "random", L, R, (gb,), "block 3", bs=3)


def test_one_and_two_row_frames(torch_dev):
    """H = 1 and 2: every init row and every staged row is a clamped copy of row 0 or H - 1."""
    for H in (1, 2):
        L, R = _pair(H)
        for bs in (9, 3):
            _all_modes(torch_dev, ("random", H), L, R, (0, 1), f"H={H} block {bs}", bs=bs)


# ---- extreme images ------------------------------------------------------------------------------------

GRIDS = (0, 77, 3)  # at H = 24: one-row segments, one and two rows, blocks that run through several strips


def _extreme(name):
    H, W = 24, W0
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    if name == "0/255":
        return np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)
    if name == "255/0":
        return np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8)
    if name == "swap":  # the views swap their values half way down: entering and leaving rows differ by the full range
        L, R = np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)
        L[H // 2:], R[H // 2:] = 255, 0
        L[::3, 5::7] = 128  # some texture: the minimum is not the same everywhere
        return L, R
    if name == "checker":  # 0 / 255 by column, the right view a column out of phase in every third row
        L = ((x & 1) * 255).astype(np.uint8)
        R = (((x + (y % 3 == 0)) & 1) * 255).astype(np.uint8)
        return L, R
    if name == "ramp7":  # periods 7 and 11: the bytes of a window cross staged dwords and lanes at every phase
        L = (((x + 3 * y) % 7) * 40).astype(np.uint8)
        R = (((x + 5 + 2 * y) % 11) * 25).astype(np.uint8)
        return L, R
    raise KeyError(name)


@pytest.mark.parametrize("name", ["0/255", "255/0", "swap", "checker", "ramp7"])
def test_extreme_images(torch_dev, name):
    L, R = _extreme(name)
    H = L.shape[0]
    for gb in GRIDS:
        kinds = _kinds(_blocks(H, gb), H)
        assert {0: {"f:n1"}, 77: {"f:n2"}, 3: {"f:n4+", "c>f", "f>c"}}[gb] <= kinds, (gb, sorted(kinds))
    if name in ("0/255", "255/0"):  # every half of every window sum at its bound
        want = fg.want(name, L, R, M, D, BS, 0)
        assert np.all(want["fixed"][:, D - 1:] == 0)
    _all_modes(torch_dev, name, L, R, GRIDS, name)
    _all_modes(torch_dev, name, L, R, GRIDS, name + " block 3", bs=3, fmodes=("fixed",))


# ---- alignment -----------------------------------------------------------------------------------------

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
    """Base pointer at byte offset 0 .. 3 and row strides W .. W + 3: every residue of the row pointer, changing from
    row to row when the stride is no multiple of 4."""
    torch = torch_dev
    H = 12
    assert {"f:n2", "f:n3"} <= _kinds(_blocks(H, 30), H) and "f:n4+" in _kinds(_blocks(H, 3), H)
    L, R = _pair(H)
    (bl, vl), (br, vr) = _views(torch, L, R, off, W0 + pad)
    assert vl.data_ptr() % 4 == (bl.data_ptr() + off) % 4 and vl.stride(0) == W0 + pad
    for bs in (9, 3):
        want = fg.want(("random", H), L, R, M, D, bs, 10)
        _run(torch, vl, vr, L.shape, want, f"views off={off} stride=W+{pad} block {bs}", (30, 3), uniqueness_ratio=10,
             min_disp=M, num_disp=D, block_size=bs, **BASE)


@pytest.mark.parametrize("W", [288, 292])
def test_rows_that_end_their_allocation(torch_dev, W):
    """The images are tensors of exactly H * W bytes.  W = 288: the last unaligned strip, x0 = 224, is followed by a
    ragged clamped one (x0 = 256, 32 of whose columns exist).  W = 292: the last unaligned strip is x0 = 256, whose
    reference bytes [252, 292) end with the row, so in the last row its final dword ends at the tensor's last byte."""
    torch = torch_dev
    H = 12
    for bs in (9, 3):
        R = bs // 2
        blocks = _blocks(H, 25, W=W, bs=bs)
        fast = _fast_x0(blocks)
        assert fast[-1] == (224 if W == 288 else 256), fast
        if bs == 9:
            assert (fast[-1] - R + 40 == W) == (W == 292)
        if W == 288:
            assert any(not s.fast and s.x0 == 256 for b in blocks for s in b)
        L, Rr = _pair(H, W=W, seed=W)
        dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(Rr).cuda()
        assert dL.numel() == H * W and dL.is_contiguous()
        for u in (0, 10):
            want = fg.want(("random", H, W), L, Rr, M, D, bs, u)
            _run(torch, dL, dR, L.shape, want, f"W={W} block {bs} u={u}", (0, 25, 3), uniqueness_ratio=u,
                 min_disp=M, num_disp=D, block_size=bs, **BASE)


# ---- disparity range -----------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [127, 96])
@pytest.mark.parametrize("m", [0, 3])
def test_disparity_range(torch_dev, d, m):
    """D = 127: the high half of the last pair is overwritten behind the tile stores.  D = 96: 16 lanes hold padding
    disparities only, update their group sums and store nothing.  min_disp = 3 moves the searched positions."""
    H = 24
    for gb in GRIDS:
        kinds = _kinds(_blocks(H, gb, m=m, d=d), H)
        assert {0: {"f:n1"}, 77: {"f:n2"}, 3: {"f:n4+", "c>f"}}[gb] <= kinds, (gb, sorted(kinds))
    L, R = _pair(H, m=m, d=d, seed=d + m)
    for bs in (9, 3):
        _all_modes(torch_dev, ("random", H, d, m), L, R, GRIDS, f"D={d} m={m} block {bs}", m=m, d=d, bs=bs)


# ---- batches and handles -------------------------------------------------------------------------------

def test_batch_of_three_frames(torch_dev):
    """Three frames per launch; of four blocks the inner ones go on from one frame into the next."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    H, NF = 12, 3
    grids = (0, 75, 4)
    assert any(len({s.frame for s in b}) == 2 for b in _blocks(H, 4, nf=NF))
    assert "f:n3" in _kinds(_blocks(H, 75, nf=NF), H)
    fr = [_pair(H, seed=s) for s in range(NF)]
    dL = torch.from_numpy(np.stack([f[0] for f in fr])).cuda()
    dR = torch.from_numpy(np.stack([f[1] for f in fr])).cuda()
    for bs in (9, 3):
        wants = [fg.want(("random", H, i), L, R, M, D, bs, 10) for i, (L, R) in enumerate(fr)]
        for g in grids:
            mt = HipBlockMatcher(grid_blocks=g, uniqueness_ratio=10, min_disp=M, num_disp=D, block_size=bs, **BASE)
            try:
                fx = torch.empty((NF, H, W0), dtype=torch.int16, device="cuda")
                fl = torch.empty((NF, H, W0), dtype=torch.float32, device="cuda")
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
    H, NF = 12, 4
    grids = (0, 25, 3)
    fr = [_pair(H, seed=s) for s in range(NF)]
    wants = [fg.want(("random", H, i), L, R, M, D, BS, 10) for i, (L, R) in enumerate(fr)]
    dev = [(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in fr]
    mts = [HipBlockMatcher(in_flight=True, grid_blocks=g, uniqueness_ratio=10, min_disp=M, num_disp=D, block_size=BS, **BASE)
           for g in grids]
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
