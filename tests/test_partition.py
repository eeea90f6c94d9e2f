"""Host-side launch plan of the fused pass (csrc/dsx_partition.h, used by bm2's launcher).

The header is plain C++; this test compiles a small harness against it with g++ and checks, over
many launch shapes, that the partition covers every (frame, strip, row) unit exactly once, keeps
one strip per block whenever there are at least as many blocks as strips, gives every strip a
block, and splits work across age levels in proportion to their weights.  The GPU parity tests
(tests/test_gpu_parity.py) run the same code path on the device at full-size grids.

It also pins the Python restatement that the GPU tests choose their cases by (tests/fused_geometry.py)
to the header: strips, fast test, fast interval, grid, age levels and the blocks' segments agree over
a sweep of kernels, frames and residencies, and the fast interval is the fast test solved for x0.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fused_geometry as fg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "depthestimation_amd", "csrc", "dsx_partition.h")

HARNESS = r"""
#include "dsx_partition.h"
#include <cstdio>
static void print(const std::vector<int> &p) {
    for (size_t i = 0; i < p.size(); ++i) printf("%d%c", p[i], i + 1 < p.size() ? ' ' : '\n');
}
int main() {
    char tag;
    while (scanf(" %c", &tag) == 1) {
        if (tag == 'P') {  // a partition
            int NG, S, sb, nf, H, XL, XU, TX, w8, nl, w[4];
            if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &NG, &S, &sb, &nf, &H, &XL, &XU, &TX, &w8, &nl, &w[0],
                      &w[1], &w[2], &w[3]) != 14) return 1;
            print(dsx::bm2_partition(NG, S, sb, nf, H, XL, XU, TX, w8, nl, w));
        } else {  // 'L': a launch plan; line 1 the plan and the fast test of every strip of the row, line 2 (part != 0)
                  // its partition with one age level
            int side, R, NW, ssd, abs1, W, m, D, band, H, nf, gb, bpc, ncu, fl, small, flight, part;
            if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &side, &R, &NW, &ssd, &abs1, &W, &m, &D, &band,
                      &H, &nf, &gb, &bpc, &ncu, &fl, &small, &flight, &part) != 18) return 1;
            const int TX = 32, NC = TX + 2 * R, NJ = NC + NW * (ssd ? 64 : 128);
            const dsx::Bm2Strips st = dsx::bm2_strips(W, m, D, band != 0, TX);
            const dsx::Bm2Interval fi = dsx::bm2_fast_interval(side, R, NC, NJ, W, m);
            const dsx::Bm2Grid g = dsx::bm2_grid(bpc, ncu, R, NW, ssd != 0, side, abs1 != 0, (long)st.count * nf * H, nf,
                                                 fl != 0, gb, small != 0, flight != 0);
            printf("%d %d %d %d %ld %d", st.begin, st.count, fi.XL, fi.XU, g.grid, g.nlev);
            for (int x0 = 0; x0 < W; x0 += TX) printf(" %d", (int)dsx::bm2_fast(side, x0, R, NC, NJ, W, m));
            printf("\n");
            const int w[4] = {64, 64, 64, 64};
            if (part) print(dsx::bm2_partition((int)g.grid, st.count, st.begin, nf, H, fi.XL, fi.XU, TX, 11, 1, w));
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("part")
    src = d / "h.cpp"
    src.write_text(HARNESS)
    exe = d / "h"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True)

    def run(cases, tag="P"):
        inp = "".join(tag + " " + " ".join(map(str, c)) + "\n" for c in cases)
        out = subprocess.run([str(exe)], input=inp, capture_output=True, text=True, check=True).stdout
        return [np.array(list(map(int, line.split())), np.int64) for line in out.strip().split("\n")]

    return run


def _cases():
    rng = np.random.default_rng(7)
    cases = []
    for NG in (1, 3, 37, 256, 1024, 3072, 4000):
        for (S, H) in ((60, 1080), (40, 720), (5, 34), (120, 2160), (1, 17)):
            for nf in (1, 4):
                XL, XU = int(rng.integers(0, 200)), int(S * 32 - rng.integers(0, 200))
                for nl, w in ((1, (64, 64, 64, 64)), (3, (78, 70, 64, 64)), (4, (90, 80, 70, 64)), (3, (64, 64, 64, 64))):
                    cases.append((NG, S, 0, nf, H, XL, XU, 32, 11, nl, *w))
    return cases


def test_partition_covers_every_unit_once(harness):
    cases = _cases()
    parts = harness(cases)
    assert len(parts) == len(cases)
    for c, p in zip(cases, parts):
        NG, S, sb, nf, H = c[:5]
        NS = S * nf
        assert len(p) == NG + 1
        assert p[0] == 0 and p[-1] == NS * H, c
        assert np.all(np.diff(p) >= 0), c
        if NG >= NS:
            # one strip per block, and every strip owns at least one block
            lo, hi = p[:-1], p[1:]
            ne = hi > lo
            assert np.all((lo[ne] // H) == ((hi[ne] - 1) // H)), c
            owners = np.unique(lo[ne] // H)
            assert len(owners) == NS, c


def test_partition_age_weights_shift_work(harness):
    # one strip, 3 levels of 100 blocks: rows per block follow the level weights
    NG, H = 300, 30000
    (p,) = harness([(NG, 1, 0, 1, H, -10 ** 6, 10 ** 6, 32, 8, 3, 96, 80, 64, 64)])
    rows = np.diff(p)
    per_level = [rows[i * 100:(i + 1) * 100].mean() for i in range(3)]
    assert per_level[0] > per_level[1] > per_level[2]
    np.testing.assert_allclose(np.array(per_level) / per_level[2], [96 / 64, 80 / 64, 1.0], rtol=0.02)


def test_partition_equal_weights_is_the_plain_split(harness):
    # equal weights: strip g's cnt blocks split its rows as j * H / cnt
    NG, S, H = 3072, 60, 1080
    (p,) = harness([(NG, S, 0, 1, H, 0, S * 32, 32, 8, 3, 64, 64, 64, 64)])
    starts = [int(np.searchsorted(p[:-1], g * H, side="left")) for g in range(S + 1)]
    for g in range(S):
        b0, b1 = starts[g], starts[g + 1]
        cnt = b1 - b0
        for j in range(cnt):
            assert p[b0 + j] == g * H + j * H // cnt


# ---- the launch plan and its Python restatement (tests/fused_geometry.py) ------------------------------

RADII = range(8)
KERNELS = [("pair", nw) for nw in (1, 2, 4)] + [("lane", nw) for nw in (1, 2, 4, 8)]  # layout, waves per block
SIDES = (0, 1, 3)
WIDTHS = (64, 200, 256, 640)
MIN_DISPS = (-16, 0, 8)
NUM_DISPS = (16, 48, 64, 128, 200)
HEIGHTS = (1, 2, 3, 7, 8, 9, 12, 13, 20, 24, 41, 48)  # 1 .. 48, thinned
GRID_BLOCKS = (0, 1, 2, 3, 5, 7, 35, "T")
RESIDENCIES = ((12, 256), (6, 256), (2, 256), (1, 4))
UNIT = {"pair": 128, "lane": 64}


def _record(side, R, layout, NW, sad1, W, m, D, band, H, nf, gb, res, fl, small, flight, part):
    """One 'L' line of the harness; gb 'T' is the launch's row count."""
    if gb == "T":
        gb = fg.strips(W, m, D, band)[1] * nf * H
    return (side, R, NW, int(layout == "lane"), int(sad1), W, m, D, int(band), H, nf, gb, res[0], res[1], int(fl),
            int(small), int(flight), int(part))


@pytest.fixture(scope="module")
def geometry_sweep(harness):
    """Every (side, R, kernel, W, m, D), with and without the band rule: (arguments, the harness's plan line)."""
    args = [(side, R, layout, NW, W, m, D, band) for side in SIDES for R in RADII for layout, NW in KERNELS
            for W in WIDTHS for m in MIN_DISPS for D in NUM_DISPS for band in (True, False)]
    recs = [_record(side, R, layout, NW, False, W, m, D, band, 7, 1, 0, (12, 256), False, True, True, False)
            for side, R, layout, NW, W, m, D, band in args]
    return list(zip(args, harness(recs, "L")))


@pytest.fixture(scope="module")
def grid_sweep(harness):
    """20000 draws from the whole sweep, and full-size frames: (arguments, the harness's plan line)."""
    rng = np.random.default_rng(11)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]  # noqa: E731
    args = []
    for _ in range(20000):
        layout, NW = pick(KERNELS)
        sad1 = layout == "lane" and NW == 1 and bool(rng.integers(2))
        args.append((pick(SIDES), pick(RADII), layout, NW, sad1, pick(WIDTHS), pick(MIN_DISPS), pick(NUM_DISPS),
                     bool(rng.integers(2)), pick(HEIGHTS), pick((1, 2, 3)), pick(GRID_BLOCKS), pick(RESIDENCIES),
                     bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2))))
    # and a full-size frame (1920 x 1080, more rows than any residency holds blocks) for every kernel and residency
    args += [(0, 4, layout, NW, False, 1920, 0, 128, True, 1080, nf, 0, res, fl, True, True)
             for layout, NW in KERNELS for res in RESIDENCIES for nf in (1, 2) for fl in (False, True)]
    return list(zip(args, harness([_record(*a, False) for a in args], "L")))


def test_restatement_equals_the_header(harness, geometry_sweep, grid_sweep):
    for (side, R, layout, NW, W, m, D, band), out in geometry_sweep:
        Dp = NW * UNIT[layout]
        assert fg.strips(W, m, D, band) == (out[0], out[1]), (W, m, D, band)
        assert fg.fast_interval(W, m, R, Dp, side) == (out[2], out[3]), (side, R, Dp, W, m)
        assert [fg.fast(x0, W, m, R, Dp, side) for x0 in range(0, W, fg.TX)] == [bool(f) for f in out[6:]], (side, R, Dp, W, m)
    for (side, R, layout, NW, sad1, W, m, D, band, H, nf, gb, res, fl, small, flight), out in grid_sweep:
        T = out[1] * nf * H
        got = fg.grid(T, T if gb == "T" else gb, R, NW, layout == "lane", side, sad1, nf, fl, res, small, flight)
        assert got == (out[4], out[5]), (side, R, layout, NW, sad1, T, nf, gb, res, fl, small, flight)
        assert fg.grid(T, T if gb == "T" else gb)[0] == max(1, min(T, out[4] if gb else T))  # no residency: the clip decides
    # blocks(): the layout follows from D as in a handle (None: a SAD handle's, 'lane' alone: SSD)
    rng = np.random.default_rng(12)
    pick = lambda seq: seq[int(rng.integers(len(seq)))]  # noqa: E731
    args = [(pick(SIDES), pick(RADII), pick((None, "pair", "lane")), pick(WIDTHS), pick(MIN_DISPS), pick(NUM_DISPS),
             bool(rng.integers(2)), pick(HEIGHTS), pick((1, 2, 3)), pick(GRID_BLOCKS), pick(RESIDENCIES),
             bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2))) for _ in range(1500)]
    recs = []
    for side, R, layout, W, m, D, band, H, nf, gb, res, fl, small, flight in args:
        lay = layout or fg.sad_layout(D)
        recs.append(_record(side, R, lay, fg.dp(D, lay) // UNIT[lay], layout is None and D <= 64, W, m, D, band, H, nf, gb,
                            res, fl, small, flight, True))
    out = harness(recs, "L")
    assert len(out) == 2 * len(args)
    for (side, R, layout, W, m, D, band, H, nf, gb, res, fl, small, flight), rec, plan, part in zip(args, recs, out[0::2], out[1::2]):
        blocks = fg.blocks(H, rec[11], W, m, nf, R, D, layout, side, band, in_flight=fl, residency=res, small_grid=small,
                           flight_grid=flight)
        sb, S = int(plan[0]), int(plan[1])
        assert len(blocks) == plan[4] == len(part) - 1, rec
        lin = 0
        for b, segs in enumerate(blocks):
            assert lin == part[b], (rec, b)
            for s in segs:  # a segment is where its block's rows say, and fast where the header says
                assert (s.frame * S + s.strip) * H + s.y0 == lin and s.y0 + s.rows <= H and s.rows > 0, (rec, b, s)
                assert s.x0 == fg.TX * (sb + s.strip) and s.fast == bool(plan[6 + sb + s.strip]), (rec, b, s)
                lin += s.rows
        assert lin == part[-1] == S * nf * H, rec


def test_fast_interval_is_the_fast_test_solved_for_x0(geometry_sweep):
    """For every strip start of the row, fast(x0) exactly when XL <= x0 <= XU: in the header and in the restatement."""
    seen = set()
    for (side, R, layout, NW, W, m, D, band), out in geometry_sweep:
        Dp = NW * UNIT[layout]
        XL, XU = fg.fast_interval(W, m, R, Dp, side)
        for i, x0 in enumerate(range(0, W, fg.TX)):
            assert bool(out[6 + i]) == (out[2] <= x0 <= out[3]), ("header", side, R, Dp, W, m, x0)
            assert fg.fast(x0, W, m, R, Dp, side) == (XL <= x0 <= XU), ("restatement", side, R, Dp, W, m, x0)
            seen.add(bool(out[6 + i]))
    assert seen == {True, False}


def test_age_levels_only_at_the_full_residency_with_one_frame(grid_sweep):
    levels = set()
    for (side, R, layout, NW, sad1, W, m, D, band, H, nf, gb, res, fl, small, flight), out in grid_sweep:
        full = bool(out[4] == res[0] * res[1]) and nf == 1
        assert out[5] == (min(max(res[0] * NW // 4, 1), 4) if full else 1), (res, NW, nf, out[4], out[5])
        levels.add((full, int(out[5])))
    assert {(False, 1), (True, 1), (True, 2), (True, 3), (True, 4)} <= levels
