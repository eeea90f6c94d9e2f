"""Launch geometry of the fused pass, restated once for the GPU tests, and their shared comparison helpers.

The launch is decided in csrc/dsx_partition.h: bm2_strips (which strips run), bm2_fast (which of them load unaligned
dwords, the others take clamped bytes), bm2_fast_interval (the same test solved for the strip start), bm2_grid (how
many blocks) and bm2_partition (which rows each block owns).  This module states the same rules in Python, so that a
GPU test can assert that the segment shapes it is there for occur in the launch it makes.  It is written from the
rules, needs no compiler, and tests/test_partition.py compares every function here with the header on the CPU.

One assumption is made here and nowhere else: the GPU tests do not know the device's residency (blocks per CU x
CUs), and grid() without one takes every grid the launcher could choose - half of the residency at the least - to be
no smaller than the launch's T rows of work, so that the clip to T decides.  The test frames have a few hundred rows
of work and the device holds thousands of blocks.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

TX = 32  # strip width

Seg = namedtuple("Seg", "frame strip x0 y0 rows fast")  # strip: index within the launch's strip range


# ---- the plan --------------------------------------------------------------------------------------------

def dp(d, layout):
    """Disparities per block of the layout that holds d: 'pair' (two per lane) in 1, 2 or 4 waves, 'lane' (one per
    lane) in 1, 2, 4 or 8."""
    unit = {"pair": 128, "lane": 64}[layout]
    nw = 1
    while nw * unit < d:
        nw *= 2
    assert nw <= 512 // unit, (d, layout)
    return nw * unit


def sad_layout(d):
    """The layout of a SAD handle's fused passes: one disparity per lane up to 64 disparities, else pairs."""
    return "lane" if d <= 64 else "pair"


def strips(W, m, d, band=True):
    """(first strip, strip count): the strips that meet the valid band [m + d - 1, W - 1 + m], or all of them."""
    if not band:
        return 0, (W + TX - 1) // TX
    xlo, xhi = max(0, m + d - 1), min(W - 1, W - 1 + m)
    if xlo > xhi:
        return 0, 0
    return xlo // TX, xhi // TX + 1 - xlo // TX


def fast(x0, W, m, R, Dp, side=0):
    """The kernel's test for the unaligned-dword loads of the strip at x0: the NJ = NC + Dp staged search positions
    (whole dwords) and the reference bytes [x0 - R, x0 - R + 4 NC4) lie inside the row.  side 1: the right pass."""
    NC = TX + 2 * R
    NJ4, NC4 = (NC + Dp + 3) // 4, (NC + 3) // 4
    if side == 1:
        PB = x0 - R + m
        search = PB >= 0 and PB + 4 * NJ4 <= W - 1
    else:
        PB = x0 - R - m + NC - 1
        search = PB - 4 * NJ4 >= 0 and PB <= W - 1
    return search and x0 - R >= 0 and x0 - R + 4 * NC4 - 1 <= W - 1


def fast_interval(W, m, R, Dp, side=0):
    """(XL, XU): fast(x0) for exactly the x0 in [XL, XU]."""
    NC = TX + 2 * R
    NJ4, NC4 = (NC + Dp + 3) // 4, (NC + 3) // 4
    ref_hi = W - 1 + R - 4 * NC4 + 1
    if side == 1:
        return max(R - m, R), min(W - 1 - 4 * NJ4 + R - m, ref_hi)
    return max(4 * NJ4 + R + m - NC + 1, R), min(W - 1 + R + m - NC + 1, ref_hi)


def grid(T, gb=0, R=4, NW=1, lane=False, side=0, sad1=False, nf=1, in_flight=False, residency=None,
         small_grid=True, flight_grid=True):
    """(blocks, age levels) of a launch with T rows of work and grid_blocks = gb.  residency: (blocks per CU, CUs),
    or None for the assumption in the module's docstring.  lane: one disparity per lane; sad1: its SAD kernels."""
    if residency is None:
        return max(1, min(gb, T) if gb > 0 else T), 1
    bpc, cus = residency
    full = g = bpc * cus
    if small_grid and not sad1 and T < g * (2 * R + 1) and bpc >= 3:  # small frames: two thirds
        g = cus * (bpc * 2 // 3)
    if flight_grid and in_flight and NW == 1 and bpc >= 3:  # in_flight: half (plain pair left pass) or two thirds
        g = min(g, cus * (bpc // 2 if not lane and side == 0 else bpc * 2 // 3))
    if gb > 0:
        g = gb
    g = max(1, min(g, T))
    nlev = min(max(bpc * NW // 4, 1), 4) if g == full and nf == 1 else 1
    return g, nlev


def partition(NG, S, sb, nf, H, XL, XU, w8=11):
    """bm2_partition with one age level (every block weighs the same): block b owns the linear (frame, strip, row)
    units [part[b], part[b + 1])."""
    NS = S * nf
    if NG < NS or NS <= 0:
        return [b * NS * H // NG for b in range(NG + 1)]
    slo = min(max((XL + TX - 1) // TX - sb, 0), S)
    shi = min(max(XU // TX - sb + 1, slo), S)
    if w8 < 8 or NG * 8 < NS * w8 + 8 * NS:
        w8 = 8
    ex = w8 - 8
    Pf = lambda s: 8 * s + ex * (min(s, slo) + max(0, s - shi))  # noqa: E731
    Uf = Pf(S)
    U = Uf * nf
    P = lambda g: (g // S) * Uf + Pf(g % S)  # noqa: E731
    start, b = [], 0
    for g in range(NS + 1):
        while b < NG and b * U < P(g) * NG:
            b += 1
        start.append(b)
    part = [0] * (NG + 1)
    for g in range(NS):
        qd = start[g + 1] - start[g]
        for bb in range(start[g], start[g + 1] + 1):
            part[bb] = g * H + (bb - start[g]) * H // qd
    part[NG] = NS * H
    return part


def blocks(H, gb, W, m, nf, R, d, layout=None, side=0, band=True, **grid_kw):
    """Per block of a launch its segments (runs of rows of one strip of one frame), in order.  layout: None for a
    SAD handle's; side 0 / 1 / 3; band: only the strips that meet the valid band (the left pass without the
    right-view winners); grid_kw: in_flight, residency and the switches of grid()."""
    sad1 = layout is None and d <= 64  # an explicit 'lane' is the SSD cost
    layout = layout or sad_layout(d)
    Dp = dp(d, layout)
    sb, S = strips(W, m, d, band)
    T = S * nf * H
    NG, _ = grid(T, gb, R, Dp // {"pair": 128, "lane": 64}[layout], layout == "lane", side, sad1, nf, **grid_kw)
    part = partition(NG, S, sb, nf, H, *fast_interval(W, m, R, Dp, side))
    out = []
    for b in range(NG):
        it, lin1, segs = part[b], part[b + 1], []
        while it < lin1:
            sidx, yb = it // H, it % H
            ye = min(H, yb + lin1 - it)
            x0 = TX * (sb + sidx % S)
            segs.append(Seg(sidx // S, sidx % S, x0, yb, ye - yb, fast(x0, W, m, R, Dp, side)))
            it += ye - yb
        out.append(segs)
    assert sum(s.rows for segs in out for s in segs) == T
    return out


# ---- comparison ------------------------------------------------------------------------------------------

def check(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} of {got.size} pixels differ, first {bad[:4].tolist()}: "
                           f"got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


def check_maps(fixed, flt, want, what, fmode="fixed"):
    """Bit for bit: the int16 x16 map, and the float map - mode 'fixed' against x16 / 16 (exact in f32), 'parabola'
    by bit pattern.  fixed / flt: device tensors, or None for an output the call did not ask for.  want: the oracle's
    dict, or its x16 map alone (mode 'fixed' only)."""
    wf = want["fixed"] if isinstance(want, dict) else want
    if fixed is not None:
        check(fixed.cpu().numpy(), wf, what + " fixed")
    if flt is not None:
        if fmode == "fixed":
            check(flt.cpu().numpy(), wf.astype(np.float32) / np.float32(16), what + " float")
        else:
            check(flt.cpu().numpy().view(np.int32), want["parabola"].view(np.int32), what + " float (parabola, bits)")


_CREF = []
_WANT = {}


def want(key, L, R, m, d, bs, u, sp=True, lr=-1):
    """Oracle maps (C oracle, SAD), computed once per (input, parameters) and shared by the tests of a run.  key names
    the input for the reader; the cache goes by the images themselves, so two files may use one name."""
    k = (key, L.shape, hash(L.tobytes()), hash(R.tobytes()), m, d, bs, u, sp, lr)
    if k not in _WANT:
        if not _CREF:
            from oracle.cref import CRef
            _CREF.append(CRef())
        _WANT[k] = _CREF[0](L, R, m, d, bs, "sad", u, lr, sp)
    return _WANT[k]
