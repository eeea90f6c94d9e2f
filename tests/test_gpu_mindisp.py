"""The fused block-matching pass (csrc/dsx_bm.hip, bm2) away from min_disp = 0.  m = min_disp is no constant added at
the end: it moves the search base PB = x0 - R - m + NC - 1 (x0 - R + m in the right pass), with it the strips that take
the unaligned-dword copy (bm2_fast / bm2_fast_interval, csrc/dsx_partition.h), the strips a band-only launch covers
(bm2_strips) and the columns its invalid fill writes, the valid test of the epilogues, the right pass's edge test, the
diagonal exits of the LR pass and the int16 range of the output.

What can go wrong, and the cases for it:
  * the scalar-base loads of the unaligned copy rest on PB - 4 tj - 3 >= 1 and PB <= W - 1: an m at which a band
    strip starts exactly at the fast interval's lower end (no slack left of the lowest staged search byte) and m + 1,
    where the same strip falls to the clamped copy (LEFT0, every radius of the rotated loop); a negative m at which a
    band strip starts exactly at the interval's upper end, set by the search bytes and not, as at m >= 0, by the
    reference bytes, and m - 1 (RIGHT0);
  * a band strip right of the fast ones, clamped because of the search alone, in which the band ends (m = -37: the
    epilogue's ex <= W - 1 + m cuts inside the strip, which happens for m < 0 only), and beyond it a ragged last strip
    wholly outside the band, which only the invalid fill writes (W = 330);
  * clamped strips on both sides of the fast ones inside one band (m = -64);
  * a band that starts inside a strip and one that starts on a strip boundary (m = 33, m = -31: m + D - 1 = 160, 96);
  * m = 1, -1, 3, 60: a sign slip in PB or in the band next to m = 0, and a band of two strips;
  * the uniqueness branch (10, 15), which reads the blocks again, and the padding (D = 100, D = 127) next to real
    costs at m != 0;
  * winners known by construction, L(x) = R(x - m - d) for d = 0, an inner d and D - 1: the map is 16 (m + d) in a
    fast strip; a tie of sixteen disparities (period 8) at m != 0: the lowest wins;
  * the LR check on the one-wave pair layout, both forms: 'bm' (the left pass builds the right-view winners along
    the diagonals x - m - d of every strip, lr_fixup gathers key x - m - d*) and 'sgbm' (unique winners scatter to
    x - m - d*, OpenCV's band [max(m + D, 0), W + min(m, 0))), three calls through one handle (the key halves
    alternate), at disp12_max_diff 0, 1, 2;
  * the right-view map (bm_pass_right): PB = x0 - R + m, its own fast interval and its edge strips
    (x0 + m < 0 or x0 + TX - 1 + m + Dp - 1 > W - 1), against oracle.stereo_bm.right_argmin;
  * no valid column at all (m = -W, m = W - D + 1) and exactly one (m = W - D: column W - 1, m = -(W - 1): column 0),
    with and without the LR pass, both outputs and each alone: every other pixel is (m - 1) * 16 / float(m - 1);
  * the ends of the int16 range: m = -2047 (invalid is -32768, winners at d = 0 give -32752) and m = 1919
    (m + D = 2047, a winner at d = D - 1 gives 32736) on a 2304-column frame;
  * the other layouts: one disparity per lane (SAD at D = 64, and SSD, whose views - unlike test_ssd_lr_shapes' -
    are built from the true negative m) and the two-wave pair layout (D = 160, D = 256).

test_geometry needs no device: it derives the launch of every (W, m, block, D) below from tests/fused_geometry.py and
asserts that the segment shape the case is there for occurs in it.  Every map is compared bit for bit over all pixels
(fg.check_maps) with the C oracle (oracle/cref.py), the OpenCV form with oracle/sgbm_post.wta_sgbm, the right-view map
and the SSD maps with oracle/stereo_bm.py; every matcher case runs under grid_blocks 0 and 5.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from depthestimation_amd.synthetic import stereo_pair

import fused_geometry as fg

gpu = pytest.mark.gpu

D = 128
TX = fg.TX
S224, S330 = (12, 224), (24, 330)
SHAPES = [S224, S330]
BLOCKS = [1, 5, 7, 9, 11]  # R = 0, 2, 3, 4, 5: every radius of the rotated row loop
GRIDS = (0, 5)  # the default grid and five blocks (segments of many rows, cut inside strips)
TX0 = 160  # the strip of the 224-column frame that LEFT0 and RIGHT0 put on the ends of the fast interval

# per block size: the m at which the fast interval of the left pass starts at strip 160 (m + 1: the strip is clamped),
# and the negative m at which it ends there, bounded by the search (m - 1: clamped).  W = 224, D = 128; test_geometry
# confirms each.
LEFT0 = {1: 31, 5: 29, 7: 26, 9: 27, 11: 24}
RIGHT0 = {1: -32, 5: -30, 7: -29, 9: -28, 11: -27}
COMMON = [-64, -37, -31, -1, 1, 3, 33, 60]


def _ms(bs):
    """The m of the plain left pass at one block size (blocks 1 and 7: a few of them)."""
    if bs in (1, 7):
        return [LEFT0[bs], LEFT0[bs] + 1, RIGHT0[bs], -37, 3]
    return [LEFT0[bs], LEFT0[bs] + 1, RIGHT0[bs], RIGHT0[bs] - 1] + COMMON


PLAIN = [(bs, m) for bs in BLOCKS for m in _ms(bs)]
PADDED = [(d, m) for d in (100, 127) for m in (27, -37)]
KNOWN_M = (24, -37)  # a fast strip in the 224-column frame at blocks 5, 9 and 11
KNOWN_D = (0, 77, D - 1)
LR_M = (-37, -4, 3, 27, 40)
OTHER_M = (-37, -4, 3, 27, 60)
EMPTY_W = 224
EMPTY_M = {"empty on the right": -EMPTY_W, "empty on the left": EMPTY_W - D + 1, "column W - 1 only": EMPTY_W - D,
           "column 0 only": -(EMPTY_W - 1)}
RANGE_SHAPE = (6, 2304)
RANGE_M = (-2047, 1919)
OTHER = [  # layout, cost, D, block, (H, W)
    ("lane", "sad", 64, 5, S224),
    ("lane", "ssd", 64, 5, S224),
    ("pair", "sad", 160, 7, S330),
    ("pair", "sad", 256, 9, (12, 416)),
]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


# ---- geometry ------------------------------------------------------------------------------------------

def _launch(W, m, bs, d=D, H=12, layout=None, side=0, band=True):
    """Of one launch: (x0 of its strips, of the fast ones, of the clamped ones left of them, right of them)"""
    bl = fg.blocks(H, 0, W, m, 1, bs // 2, d, layout, side, band)
    xs = sorted({s.x0 for b in bl for s in b})
    sb, S = fg.strips(W, m, d, band)
    assert xs == [TX * (sb + i) for i in range(S)]
    lay = layout or fg.sad_layout(d)
    f = [x for x in xs if fg.fast(x, W, m, bs // 2, fg.dp(d, lay), side)]
    assert f == sorted({s.x0 for b in bl for s in b if s.fast})
    return xs, f, [x for x in xs if f and x < f[0]], [x for x in xs if f and x > f[-1]]


def _search_hi(W, m, R):
    """The upper end of the left pass's fast interval as the search bytes alone set it (PB <= W - 1), and as the
    reference bytes alone do"""
    NC = TX + 2 * R
    return W - 1 + R + m - NC + 1, W - 1 + R - 4 * ((NC + 3) // 4) + 1


def _edge(x0, W, m, Dp):
    """The right pass's edge test of the strip at x0 (csrc/dsx_bm.hip)"""
    return x0 + m < 0 or x0 + TX - 1 + m + Dp - 1 > W - 1


def test_geometry():
    """Every segment shape the cases below are there for occurs in the launch of its (W, m, block, D)."""
    W = S224[1]
    for bs in BLOCKS:
        R = bs // 2
        NC = TX + 2 * R
        # no slack on the left: the interval starts at a band strip, whose lowest staged search byte is byte 0 of the
        # row (PB - 4 NJ4 = 0); one more and the strip is clamped, still inside the band
        m = LEFT0[bs]
        assert m > 0 and fg.fast_interval(W, m, R, D)[0] == TX0, bs
        assert TX0 - R - m + NC - 1 - 4 * ((NC + D + 3) // 4) == 0, bs
        assert TX0 in _launch(W, m, bs)[1], bs
        xs, f, _, _ = _launch(W, m + 1, bs)
        assert TX0 in xs and TX0 not in f, bs
        assert TX0 in _launch(S330[1], m, bs)[1] and TX0 in _launch(S330[1], m + 1, bs)[2], bs
        # no slack on the right, for the search: the interval ends at a band strip, and the search bound is the lower
        m = RIGHT0[bs]
        search, ref = _search_hi(W, m, R)
        assert m < 0 and fg.fast_interval(W, m, R, D)[1] == TX0 == search < ref, bs
        assert TX0 in _launch(W, m, bs)[1], bs
        assert TX0 in _launch(W, m - 1, bs)[3], bs
    assert (LEFT0[9], RIGHT0[9]) == (27, -28) and _search_hi(W, -28, 4)[0] == W - 36 - 28
    for bs in BLOCKS:
        R = bs // 2
        for (H, W) in SHAPES:
            # m = -37: the last band strip lies right of the fast ones, its reference bytes are inside the row (the
            # search alone clamps it), and the band ends strictly inside it
            xs, f, left, right = _launch(W, -37, bs, H=H)
            x0 = xs[-1]
            assert f and left and right == [x0], (W, bs)
            assert x0 - R + 4 * ((TX + 2 * R + 3) // 4) - 1 <= W - 1 and x0 + TX <= W, (W, bs)
            search, ref = _search_hi(W, -37, R)
            assert fg.fast_interval(W, -37, R, D)[1] == search < x0 <= ref, (W, bs)
            assert x0 < W - 1 - 37 < x0 + TX - 1, (W, bs)
            # m = -64: clamped strips on both sides of the fast ones (a one-pixel block needs the wider frame for it)
            xs, f, left, right = _launch(W, -64, bs, H=H)
            assert f and left and (right or (bs, W) == (1, 224)), (W, bs)
        assert _launch(S224[1], -64, 9)[1] == [96]
        # W = 330: the ragged last strip (columns 320 .. 329) is wholly outside the band of m = -37, -64, -31
        for m in (-37, -64, -31, RIGHT0[bs], RIGHT0[bs] - 1):
            sb, S = fg.strips(S330[1], m, D)
            assert S330[1] % TX != 0 and 0 < S and TX * (sb + S) <= S330[1] // TX * TX, (bs, m)
    # the band starts on a strip boundary (m = 33, -31, 1) and inside a strip (every other m here)
    for (H, W) in SHAPES:
        for m in (33, -31, 1):
            assert (m + D - 1) % TX == 0 and TX * fg.strips(W, m, D)[0] == m + D - 1
    inside = {m for _, m in PLAIN if (m + D - 1) % TX != 0}
    assert {27, -37, -64, -1, 3, 60} <= inside and not {33, -31, 1} & inside
    assert _launch(S224[1], -37, 9)[:2] == ([64, 96, 128, 160], [96, 128])
    # every plain case has a launch, and every m meets a fast strip in one of the two frames
    for bs, m in PLAIN:
        ls = [_launch(W, m, bs, H=H) for (H, W) in SHAPES]
        assert all(xs for xs, _, _, _ in ls) and any(f for _, f, _, _ in ls), (bs, m)
        assert any(left or right for _, _, left, right in ls), (bs, m)
    for d, m in PADDED:
        for bs in (5, 9, 11):
            xs, f, left, right = _launch(S330[1], m, bs, d=d, H=S330[0])
            assert f and (left or right), (d, m, bs)
    # known winners and the tie: a fast strip in the 224-column frame
    for m in KNOWN_M:
        for bs in (5, 9, 11):
            assert _launch(S224[1], m, bs)[1], (m, bs)
    # LR, 'bm': every strip runs; 'sgbm': the band's.  Fast and clamped strips in both.
    for m in LR_M:
        for bs in (5, 9):
            for side, band in ((3, False), (0, True)):
                xs, f, left, right = _launch(S330[1], m, bs, H=S330[0], side=side, band=band)
                assert f and (left or right), (m, bs, side)
            assert len(_launch(S330[1], m, bs, side=3, band=False)[0]) == (S330[1] + TX - 1) // TX
    # the right pass: every strip runs; a fast strip and an edge strip, except that no strip of the 224-column frame
    # can be fast at m = 60: the 4 NJ4 staged search bytes from x0 - R + m on would have to end by column W - 1
    # (x0 <= 59 - m at R = 4, x0 <= 61 - m at R = 2) and the reference bytes start at x0 - R >= 0, an empty interval
    for (H, W) in SHAPES:
        for bs in (5, 9):
            for m in OTHER_M:
                xs, f, _, _ = _launch(W, m, bs, H=H, side=1, band=False)
                assert len(xs) == (W + TX - 1) // TX
                assert any(_edge(x0, W, m, D) for x0 in xs), (W, bs, m)
                if (W, m) == (224, 60):
                    XL, XU = fg.fast_interval(W, m, bs // 2, D, 1)
                    assert not f and XU < XL == bs // 2, (W, bs, m)
                else:
                    assert f, (W, bs, m)
    # empty and one-column bands
    W = EMPTY_W
    assert fg.strips(W, EMPTY_M["empty on the right"], D) == (0, 0) and W - 1 + EMPTY_M["empty on the right"] < 0
    assert fg.strips(W, EMPTY_M["empty on the left"], D) == (0, 0) and EMPTY_M["empty on the left"] + D - 1 > W - 1
    assert fg.strips(W, EMPTY_M["column W - 1 only"], D) == ((W - 1) // TX, 1) and EMPTY_M["column W - 1 only"] + D - 1 == W - 1
    assert fg.strips(W, EMPTY_M["column 0 only"], D) == (0, 1) and W - 1 + EMPTY_M["column 0 only"] == 0
    # the ends of the int16 range: bands [0, W - 2048] and [2046, W - 1], fast and clamped strips in both
    H, W = RANGE_SHAPE
    assert (-2047 - 1) * 16 == -32768 and 1919 + D == 2047 and (1919 + D - 1) * 16 == 32736
    assert (max(0, -2047 + D - 1), W - 1 - 2047) == (0, W - 2048) and 1919 + D - 1 == 2046 < W
    for m in RANGE_M:
        xs, f, left, right = _launch(W, m, 9, H=H)
        assert f and left and right, m
    # the other layouts: a fast strip, except at D = 160 (Dp = 256), W = 330, m >= 27: the fast interval is
    # [262 + m, min(295 + m, 293)] at R = 3 and holds no multiple of 32 for 27 <= m (above 31 it is empty)
    for layout, cost, d, bs, (H, W) in OTHER:
        lay = layout if cost == "ssd" else None
        assert fg.dp(d, layout) == {64: 64, 160: 256, 256: 256}[d] and (cost == "ssd" or fg.sad_layout(d) == layout)
        for m in OTHER_M:
            for side, band in ((0, True), (3, False)):
                xs, f, _, _ = _launch(W, m, bs, d=d, H=H, layout=lay, side=side, band=band)
                assert xs
                if d == 160 and m >= 27:
                    assert not f and fg.fast_interval(W, m, 3, 256) == (262 + m, min(295 + m, 293))
                else:
                    assert f, (layout, cost, d, m, side)


# ---- inputs, oracle maps and their properties (CPU) ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pair(H, W, m, d=D, seed=0, bands=6):
    L, R, _ = stereo_pair(H, W, m, d, seed=9100 + 17 * H + W + 131 * (m + 2048) + seed, bands=bands)
    return L, R


def _noise(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _periodic(seed, period, shape=S224):
    """Noise that repeats every `period` columns."""
    H, W = shape
    return np.ascontiguousarray(np.tile(_noise(seed, shape)[:, :period], (1, W // period + 1))[:, :W])


def _shift(R, s):
    """L with L(x) = R(x - s), s of either sign (columns outside the row: its first / last column, as the clamped
    search reads them)"""
    return np.ascontiguousarray(R[:, np.clip(np.arange(R.shape[1]) - s, 0, R.shape[1] - 1)])


def _costs(L, R, m, bs, d=D, cost="sad"):
    from oracle.stereo_bm import cost_volume
    return cost_volume(L, R, m, d, bs, cost)


def _band(W, m, d=D):
    """The valid band's column slice"""
    return slice(max(0, m + d - 1), max(0, min(W - 1, W - 1 + m) + 1))


def _inv(m):
    return (m - 1) * 16


def plain_inputs(shape, bs, m, d=D, u=0):
    """Random views with disparities in [m, m + d), their oracle maps; with u > 0 the uniqueness test decides both
    ways inside the band (a one-pixel block finds a zero cost nearly everywhere, and zero passes the test)."""
    H, W = shape
    # u > 0: thirteen disparity steps across the row, so that even a band of one strip holds ambiguous pixels
    L, R = _pair(H, W, m, d) if u == 0 else _pair(H, W, m, d, seed=u, bands=13)
    want = fg.want(("random", H, W, m, d), L, R, m, d, bs, u)
    band = want["fixed"][:, _band(W, m, d)]
    assert band.size and (band != _inv(m)).any(), (shape, bs, m, d, u)
    outside = np.delete(want["fixed"], np.r_[_band(W, m, d)], axis=1)
    assert np.all(outside == _inv(m)), (shape, bs, m, d, u)
    if u > 0:
        assert (band == _inv(m)).any() or bs == 1, (shape, bs, m, d, u)
    else:
        assert np.all(band != _inv(m)), (shape, bs, m, d, u)
    return L, R, want


def known_inputs(bs, m, d, sp):
    """A right view of period 160 (> D: one zero in range) and L(x) = R(x - m - d): inside the fast strips the cost at
    d is 0 and every other cost above it, and the oracle's map is 16 (m + d) - exactly where the sub-pixel step is
    off (d = 0, d = D - 1, or sp False), within the half disparity the step can move an inner winner otherwise."""
    R = _periodic(1000 + d, 160)
    L = _shift(R, m + d)
    f = _launch(S224[1], m, bs)[1]
    cols = np.concatenate([np.arange(x0, x0 + TX) for x0 in f])
    C = _costs(L, R, m, bs)[:, cols]
    assert np.all(C[:, :, d] == 0) and np.all(np.delete(C, d, axis=2) > 0), (bs, m, d)
    want = fg.want(("known", d), L, R, m, D, bs, 0, sp)
    w = want["fixed"][:, cols].astype(np.int64)
    if not sp or d in (0, D - 1):
        assert np.all(w == 16 * (m + d)), (bs, m, d, sp)
    else:
        assert np.all(np.abs(w - 16 * (m + d)) <= 8), (bs, m, d)
    return L, R, want


def tie_inputs(bs, m, u):
    """A right view of period 8 and L(x) = R(x - m): zero cost at d = 0, 8, 16, ... - the oracle's cost rows in the fast
    strips hold the sixteen-fold tie, and the lowest disparity wins."""
    R = _periodic(800 + m, 8)
    L = _shift(R, m)
    tied = list(range(0, D, 8))
    f = _launch(S224[1], m, bs)[1]
    cols = np.concatenate([np.arange(x0, x0 + TX) for x0 in f])
    C = _costs(L, R, m, bs)[:, cols]
    cmin = C.min(axis=2)
    assert all(np.all(C[:, :, d] == cmin) for d in tied) and np.all((C == cmin[..., None]).sum(axis=2) == len(tied))
    want = fg.want(("tie",), L, R, m, D, bs, u)
    if u == 0:  # d = 0: no sub-pixel step
        assert np.all(want["fixed"][:, cols] == 16 * m), (bs, m)
    return L, R, want


def lr_inputs(form, bs, m, lr, u=10):
    """Random views and the oracle's int16 map of one LR form; the check rejects some band pixels that the same
    oracle without the check keeps, and keeps others."""
    from oracle.sgbm_post import wta_sgbm
    H, W = S330
    L, R = _pair(H, W, m)
    free = fg.want(("random", H, W, m, D), L, R, m, D, bs, u)["fixed"]
    if form == "bm":
        want = fg.want(("random", H, W, m, D), L, R, m, D, bs, u, lr=lr)
        band = _band(W, m)
    else:
        want = wta_sgbm(_costs(L, R, m, bs), m, u, lr, True)["fixed"]
        band = slice(max(m + D, 0), W + min(m, 0))
        assert np.all(np.delete(want, np.r_[band], axis=1) == _inv(m))
    wf = (want["fixed"] if isinstance(want, dict) else want)[:, band]
    kept, lost = wf != _inv(m), (wf == _inv(m)) & (free[:, band] != _inv(m))
    assert kept.any() and lost.any(), (form, bs, m, lr)
    assert np.all(wf[kept] == free[:, band][kept])  # the check only ever invalidates
    return L, R, want


def right_inputs(shape, bs, m):
    from oracle.stereo_bm import right_argmin
    H, W = shape
    L, R = _pair(H, W, m)
    want = right_argmin(_costs(L, R, m, bs), m)
    # x + m + d inside the row for some d in [0, D): elsewhere the map is -1
    x = np.arange(W)
    empty = (x + m + D - 1 < 0) | (x + m > W - 1)
    assert np.all((want == -1) == empty[None, :]), (shape, bs, m)
    return L, R, want


def empty_inputs(name, lr):
    H, W, m = 12, EMPTY_W, EMPTY_M[name]
    L, R = _noise(60, (H, W)), _noise(61, (H, W))
    want = fg.want(("noise",), L, R, m, D, 9, 0, lr=lr)
    col = {"column W - 1 only": W - 1, "column 0 only": 0}.get(name)
    out = np.ones(W, bool)
    if col is not None:
        out[col] = False
        if lr < 0:
            assert np.all(want["fixed"][:, col] != _inv(m)), name
    assert np.all(want["fixed"][:, out] == _inv(m)), name
    assert np.all(want["parabola"][:, out] == np.float32(m - 1)), name
    return L, R, want


def range_inputs(m, u):
    """m = -2047: winners at d = 0 (the band's left half) and d = 2 in the band [0, W - 2048]; m = 1919: winners at
    d = D - 1 and d = D - 3 in the band [2046, W - 1].  The oracle's map holds values within 64 of that end of the
    int16 range, the invalid value aside, and the end's own winner exactly."""
    H, W = RANGE_SHAPE
    R = _noise(70 + (m > 0), RANGE_SHAPE)
    da, db = (0, 2) if m < 0 else (D - 1, D - 3)
    b = _band(W, m)
    mid = (b.start + b.stop) // 2
    L = np.concatenate([_shift(R, m + da)[:, :mid], _shift(R, m + db)[:, mid:]], axis=1)
    want = fg.want(("range",), L, R, m, D, 9, u)
    wf = want["fixed"].astype(np.int64)
    band = wf[:, b]
    near = (band != _inv(m)) & ((band <= -32768 + 64) if m < 0 else (band >= 32767 - 64))
    assert near.sum() > band.size * 3 // 4, (m, u)
    assert np.all(wf[:, b.start + 8:mid - 8] == 16 * (m + da)) and 16 * (m + da) == (-32752 if m < 0 else 32736), (m, u)
    assert np.all(np.delete(wf, np.r_[b], axis=1) == _inv(m)) and (_inv(m) == -32768 or m > 0)
    return L, R, want


def other_inputs(layout, cost, d, bs, shape, m, lr, u=10):
    H, W = shape
    L, R = _pair(H, W, m, d)  # the scene's disparities lie in [m, m + d), negative ones included
    if cost == "sad":
        want = fg.want(("random", H, W, m, d), L, R, m, d, bs, u, lr=lr)["fixed"]
    else:
        from oracle.stereo_bm import stereo_bm
        want = stereo_bm(L, R, m, d, bs, cost, u, lr, True)["fixed"]
    band = want[:, _band(W, m, d)]
    assert (band != _inv(m)).any() and (band == _inv(m)).any(), (layout, cost, d, m, lr)
    return L, R, want


# ---- the matcher ---------------------------------------------------------------------------------------

def _run(torch, L, R, want, what, fmodes=("fixed",), outs="both", calls=1, kernels=None, **kw):
    """One handle per grid and float mode; `calls` calls through it, every one compared.  kernels: (names that must
    have run, names that must not), by the handle's own timing."""
    from depthestimation_amd.matcher import HipBlockMatcher
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    for fmode in fmodes:
        for g in GRIDS:
            mt = HipBlockMatcher(grid_blocks=g, float_mode=fmode, timing=kernels is not None, **kw)
            try:
                for i in range(calls):
                    fx = torch.empty(L.shape, dtype=torch.int16, device="cuda") if outs in ("both", "fixed") else None
                    fl = torch.empty(L.shape, dtype=torch.float32, device="cuda") if outs in ("both", "float") else None
                    mt.compute_device(dL, dR, out_fixed=fx, out_float=fl)
                    torch.cuda.synchronize()
                    fg.check_maps(fx, fl, want, f"{what} {fmode} grid_blocks={g} outs={outs} call={i}", fmode)
                if kernels is not None:
                    kt = mt.kernel_times()
                    assert all(k in kt for k in kernels[0]) and not any(k in kt for k in kernels[1]), (what, sorted(kt))
            finally:
                mt.close()


def _kw(m, bs, d=D, u=0, lr=-1, cost="sad", sp=True, **more):
    return dict(cost=cost, min_disp=m, num_disp=d, block_size=bs, uniqueness_ratio=u, disp12_max_diff=lr, subpixel=sp,
                **more)


BOTH = ("fixed", "parabola")
_shape_id = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


@gpu
@pytest.mark.parametrize("bs,m", PLAIN)
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_plain_left_pass(torch_dev, shape, bs, m):
    L, R, want = plain_inputs(shape, bs, m)
    _run(torch_dev, L, R, want, f"{shape} block {bs} m={m}", fmodes=BOTH, **_kw(m, bs))


@gpu
@pytest.mark.parametrize("u", [10, 15])
@pytest.mark.parametrize("bs,m", PLAIN)
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_uniqueness(torch_dev, shape, bs, m, u):
    L, R, want = plain_inputs(shape, bs, m, u=u)
    _run(torch_dev, L, R, want, f"{shape} block {bs} m={m} u={u}", **_kw(m, bs, u=u))


@gpu
@pytest.mark.parametrize("bs", [5, 9, 11])
@pytest.mark.parametrize("d,m", PADDED)
def test_padded_and_odd_range(torch_dev, d, m, bs):
    """D = 100: whole padded blocks; D = 127: the last pair's high half is the padding."""
    L, R, want = plain_inputs(S330, bs, m, d=d)
    _run(torch_dev, L, R, want, f"D={d} block {bs} m={m}", fmodes=BOTH, **_kw(m, bs, d=d))
    for u in (10, 15):
        L, R, want = plain_inputs(S330, bs, m, d=d, u=u)
        _run(torch_dev, L, R, want, f"D={d} block {bs} m={m} u={u}", **_kw(m, bs, d=d, u=u))


@gpu
@pytest.mark.parametrize("bs", [5, 9, 11])
@pytest.mark.parametrize("d", KNOWN_D)
@pytest.mark.parametrize("m", KNOWN_M)
def test_known_winner(torch_dev, m, d, bs):
    for sp in (True, False):
        L, R, want = known_inputs(bs, m, d, sp)
        _run(torch_dev, L, R, want, f"winner {d} block {bs} m={m} subpixel={sp}", fmodes=BOTH, **_kw(m, bs, sp=sp))


@gpu
@pytest.mark.parametrize("bs", [5, 9, 11])
@pytest.mark.parametrize("m", KNOWN_M)
def test_tie_order(torch_dev, m, bs):
    L, R, want = tie_inputs(bs, m, 0)
    _run(torch_dev, L, R, want, f"tie block {bs} m={m}", fmodes=BOTH, **_kw(m, bs))
    for u in (10, 15):  # the second minimum equals the first
        L, R, want = tie_inputs(bs, m, u)
        _run(torch_dev, L, R, want, f"tie block {bs} m={m} u={u}", **_kw(m, bs, u=u))


@gpu
@pytest.mark.parametrize("lr", [0, 1, 2])
@pytest.mark.parametrize("m", LR_M)
@pytest.mark.parametrize("bs", [5, 9])
@pytest.mark.parametrize("form", ["bm", "sgbm"])
def test_lr_check(torch_dev, form, bs, m, lr):
    L, R, want = lr_inputs(form, bs, m, lr)
    fixup = "lr_fixup" if form == "bm" else "lr_fixup_sgbm"
    _run(torch_dev, L, R, want, f"lr {form} block {bs} m={m} disp12={lr}", fmodes=BOTH if form == "bm" else ("fixed",),
         calls=3, kernels=(("bm_pass_left", fixup), ("volume_wta", "cost_volume")),
         **_kw(m, bs, u=10, lr=lr, lr_form=form, path="fused"))


@gpu
@pytest.mark.parametrize("m", OTHER_M)
@pytest.mark.parametrize("bs", [5, 9])
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_right_map(torch_dev, shape, bs, m):
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    L, R, want = right_inputs(shape, bs, m)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    for g in GRIDS:
        mt = HipBlockMatcher(grid_blocks=g, **_kw(m, bs))
        try:
            out = torch.empty(shape, dtype=torch.int16, device="cuda")
            mt.right_map_device(dL, dR, out)
            torch.cuda.synchronize()
            fg.check(out.cpu().numpy().astype(np.int32), want, f"right map {shape} block {bs} m={m} grid_blocks={g}")
        finally:
            mt.close()


@gpu
@pytest.mark.parametrize("outs", ["both", "fixed", "float"])
@pytest.mark.parametrize("lr", [-1, 1])
@pytest.mark.parametrize("name", list(EMPTY_M))
def test_empty_and_one_column_bands(torch_dev, name, lr, outs):
    L, R, want = empty_inputs(name, lr)
    _run(torch_dev, L, R, want, f"{name} lr={lr}", fmodes=BOTH, outs=outs, **_kw(EMPTY_M[name], 9, lr=lr))


@gpu
@pytest.mark.parametrize("u", [0, 10])
@pytest.mark.parametrize("m", RANGE_M)
def test_int16_range_ends(torch_dev, m, u):
    L, R, want = range_inputs(m, u)
    _run(torch_dev, L, R, want, f"int16 end m={m} u={u}", fmodes=BOTH, **_kw(m, 9, u=u))


@gpu
@pytest.mark.parametrize("lr", [-1, 1])
@pytest.mark.parametrize("m", OTHER_M)
@pytest.mark.parametrize("case", OTHER, ids=lambda c: f"{c[0]}_{c[1]}_D{c[2]}_bs{c[3]}_{c[4][1]}")
def test_other_layouts(torch_dev, case, m, lr):
    layout, cost, d, bs, shape = case
    L, R, want = other_inputs(layout, cost, d, bs, shape, m, lr)
    _run(torch_dev, L, R, want, f"{layout} {cost} D={d} block {bs} m={m} lr={lr}", kernels=(("bm_pass_left",), ("volume_wta",)),
         **_kw(m, bs, d=d, u=10, lr=lr, cost=cost))
