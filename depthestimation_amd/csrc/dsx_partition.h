// Launch plan of the fused pass (bm2, dsx_bm.hip): which strips a launch covers (bm2_strips), which of them take
// the unaligned-dword loads (bm2_fast, and bm2_fast_interval, the same test solved for the strip start), how many
// blocks it gets and in how many age levels (bm2_grid), and which rows each block owns (bm2_partition).
// launch_bm2_side only adds what needs HIP or the process: the occupancy query, the environment switches, the
// device copy of the partition and the launch.  Plain C++ (no HIP header), so the CPU tests compile it directly:
// tests/test_partition.py, which also pins the tests' Python restatement (tests/fused_geometry.py) to it.
#pragma once

#include <algorithm>
#include <vector>

namespace dsx {

// Strips [begin, begin + count) of TX columns that a launch covers.  band_only (left pass without the
// right-view winners): only strips meeting the valid band [m + D - 1, W - 1 + m] need a search
// (stereo_core.py:168 crops the rest; OpenCV's band lies inside it); count 0 when the band is empty.
struct Bm2Strips {
    int begin, count;
};
inline Bm2Strips bm2_strips(int W, int min_disp, int num_disp, bool band_only, int TX) {
    if (!band_only) return {0, (W + TX - 1) / TX};
    const int xlo = std::max(0, min_disp + num_disp - 1);
    const int xhi = std::min(W - 1, W - 1 + min_disp);
    if (xlo > xhi) return {0, 0};
    return {xlo / TX, xhi / TX + 1 - xlo / TX};
}

// bm2's per-strip test for the unaligned-dword loads: every staged search position (NJ entries, whole dwords)
// and the reference bytes [x0 - R, x0 - R + 4 * ceil(NC / 4)) lie inside the row.  side 1: the right-view pass.
// The kernel (bm2, dsx_bm.hip) keeps the same expression written out: a call to this function changed the
// code of its kernels.  Keep the two equal.
constexpr bool bm2_fast(int side, int x0, int R, int NC, int NJ, int W, int m) {
    const int PB = side == 1 ? (x0 - R + m) : (x0 - R - m + NC - 1);
    const int NJ4 = (NJ + 3) / 4;
    return (side == 1 ? (PB >= 0 && PB + 4 * NJ4 <= W - 1) : (PB - 4 * NJ4 >= 0 && PB <= W - 1)) &&
           x0 - R >= 0 && x0 - R + 4 * ((NC + 3) / 4) - 1 <= W - 1;
}

// bm2_fast solved for x0: true exactly for XL <= x0 <= XU (tests/test_partition.py checks it for every strip).
struct Bm2Interval {
    int XL, XU;
};
inline Bm2Interval bm2_fast_interval(int side, int R, int NC, int NJ, int W, int m) {
    const int NJ4 = (NJ + 3) / 4, NC4 = (NC + 3) / 4;
    if (side == 1) return {std::max(R - m, R), std::min(W - 1 - 4 * NJ4 + R - m, W - 1 + R - 4 * NC4 + 1)};
    return {std::max(4 * NJ4 + R + m - NC + 1, R), std::min(W - 1 + R + m - NC + 1, W - 1 + R - 4 * NC4 + 1)};
}

// Grid and age levels of a launch of bm2<R, SSD, NW, SIDE, ABS> with T = strip_count * nframes * H rows of work
// on a device that holds blocks_per_cu * num_cu blocks.  small_grid / flight_grid: DSX_SMALL_GRID /
// DSX_FLIGHT_GRID (0 disables the rule).
struct Bm2Grid {
    long grid;
    int nlev;
};
inline Bm2Grid bm2_grid(int blocks_per_cu, int num_cu, int R, int NW, bool SSD, int SIDE, bool ABS, long T,
                        int nframes, bool in_flight, int grid_override, bool small_grid, bool flight_grid) {
    // one block per resident slot: the DSX_TIMELINE census showed all 12 reported blocks of
    // the C2 kernel co-resident (3072 on 256 CUs) and 12/CU beat 11/CU by 5% (C2, C4) while
    // 13/CU ran a second generation.
    const long full = (long)blocks_per_cu * num_cu;
    long grid = full;
    // Small frames: when a full grid leaves each block fewer rows than its (2R+1)-row segment
    // start, two thirds of the residency measured faster (C1 single frame, 2.97 rows per block at
    // 12 blocks/CU: 22.9 -> 20.6 us at 8 blocks/CU; grids of 1792-3072 otherwise within 2 %).
    // C2-C5 keep the full grid.
    // The SAD1 kernels (ABS) are measured fastest on the full grid (C1: 14.9 us at two thirds, 13.6 us
    // full; tools/c1_grid.sh), so the rule applies to the pair / SSD layouts only.
    if (small_grid && !ABS && T < grid * (2L * R + 1) && blocks_per_cu >= 3) grid = (long)num_cu * (blocks_per_cu * 2 / 3);
    // in_flight handles, one-wave blocks: two thirds of the residency.  A launch that shares the device with two others
    // gains nothing from a block per resident slot, and every block pays a (2R+1)-row segment start for its rows (C2:
    // about 20 rows behind a 9-row start at 3072 blocks).  Parent library, three frames in flight, grids of 1, 2/3,
    // 1/2, 1/3 of the residency (profiles/sref_ab.txt): C2 44.5k / 46.0k / 46.8k / 45.3k Mpix/s, C4 22.4k / 22.9k /
    // 21.7k / 22.5k, C2r 23.1k / 23.3k / 23.0k / 22.9k, C1 33.2k / 36.6k / 37.7k and 24.8k / 35.9k; half loses on C4.
    // The two- and four-wave blocks (6 and 4 per CU) keep the full grid: C5 20.57k / 20.55k / 20.29k / 16.9k,
    // C3 7.18k / 7.25k / 7.26k / 6.41k.  Lone-frame handles keep the full grid.
    // The plain left pass of the pair layout (SIDE 0, C2's kernel) takes half of the residency: with the output stores
    // behind the staging its optimum moved (grids of 1, 2/3, 1/2: 46.5k / 47.7k / 48.1k Mpix/s, three runs each within
    // 0.1k; profiles/stageahead_ab.txt).  The LR passes lose at half (C4 above), and the SAD1 layout, which gained there
    // in this sweep (C1 38.8k -> 39.8k), once fell to 24.8k on one of two runs at half and stays on two thirds.
    if (flight_grid && in_flight && NW == 1 && blocks_per_cu >= 3) {
        const bool half = !SSD && SIDE == 0;
        const long g23 = (long)num_cu * (half ? blocks_per_cu / 2 : blocks_per_cu * 2 / 3);
        if (g23 < grid) grid = g23;
    }
    if (grid_override > 0) grid = grid_override;
    if (grid > T) grid = T;
    if (grid < 1) grid = 1;
    // age levels: with one block per resident slot, block b is the (b / num_cu)-th block its CU
    // received, and co-resident waves of a SIMD differ in age (issue arbitration) by that rank
    int nlev = 1;
    if (grid == full && nframes == 1) {  // batches: equal weights
        const int lv = blocks_per_cu * NW / 4;
        nlev = lv < 1 ? 1 : (lv > 4 ? 4 : lv);
    }
    return {grid, nlev};
}

// Work partition over the (frame, strip, row) space, computed on the host once per launch shape
// and cached on the device (a per-block binary search with 64-bit / f64 arithmetic cost every
// block microseconds at kernel start).  With at least one block per (frame, strip), every block
// owns ONE contiguous run of rows of ONE strip of one frame; otherwise an even split of the
// linearised space.  Strips on the clamped-load path (image edges) weigh slow_w8/8 of a fast
// strip, so they get proportionally more blocks.  Fast strips are those with x0 in [XL, XU]
// (bm2_fast_interval).
//
// Block capacities by age level (DSX_AGEW, 1/64): with one block per resident slot, block b is
// the (b * nlev / NG)-th block its CU received; co-resident waves on a SIMD issue by age, so a
// level's blocks take work in proportion to its weight.  Q(b) = total weight of blocks < b; strip
// g starts at the first block b with Q(b) * U >= P(g) * Qtot.  Every strip keeps >= 1 block while
// 8 * NG * wmin >= U * wmax (else equal weights).
inline std::vector<int> bm2_partition(int NG, int S, int sb, int nframes, int H, int XL, int XU, int TX, int slow_w8,
                                      int nlev, const int *agew) {
    std::vector<int> part(NG + 1);
    const int NS = S * nframes;
    if (NG < NS || NS <= 0) {
        const long T = (long)NS * H;
        for (int b = 0; b <= NG; ++b) part[b] = (int)(b * T / NG);
        return part;
    }
    auto fdiv = [](long x, long y) { return x >= 0 ? x / y : -((-x + y - 1) / y); };
    const int slo = std::min(std::max((int)fdiv(XL + TX - 1, TX) - sb, 0), S);
    const int shi = std::min(std::max((int)fdiv(XU, TX) - sb + 1, slo), S);  // fast strips: [slo, shi)
    int w8 = slow_w8;
    if (w8 < 8 || NG * 8 < NS * w8 + 8 * NS) w8 = 8;  // every strip keeps >= 1 block
    const int ex = w8 - 8;
    auto Pf = [&](int s) -> long { return 8L * s + (long)ex * (std::min(s, slo) + std::max(0, s - shi)); };
    const long Uf = Pf(S), U = Uf * nframes;
    auto P = [&](int g) -> long { const int f = g / S; return f * Uf + Pf(g - f * S); };
    int nl = nlev > 1 ? std::min(nlev, 4) : 1;
    {
        int wmin = 1 << 30, wmax = 0;
        for (int L = 0; L < nl; ++L) {
            wmin = std::min(wmin, agew[L]);
            wmax = std::max(wmax, agew[L]);
        }
        if (nl > 1 && (wmin < 1 || 8L * NG * wmin < U * wmax)) nl = 1;
    }
    std::vector<long> Q(NG + 1, 0);
    for (int b = 0; b < NG; ++b) Q[b + 1] = Q[b] + (nl > 1 ? agew[(long)b * nl / NG] : 64);
    const long Qtot = Q[NG];
    std::vector<int> start(NS + 1);
    int b = 0;
    for (int g = 0; g <= NS; ++g) {
        const long T = P(g) * Qtot;
        while (b < NG && Q[b] * U < T) ++b;
        start[g] = b;
    }
    for (int g = 0; g < NS; ++g) {
        const long q0 = Q[start[g]], qd = Q[start[g + 1]] - q0;
        for (int bb = start[g]; bb <= start[g + 1]; ++bb)
            part[bb] = g * H + (int)((Q[bb] - q0) * H / qd);
    }
    part[NG] = NS * H;
    return part;
}

}  // namespace dsx
