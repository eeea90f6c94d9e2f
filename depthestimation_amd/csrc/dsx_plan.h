// The pure decisions of a matcher handle (dsx_api.hip): launch geometry, cost bounds, the SGM form and
// plan_call(): the path, the stages and the handle buffers of one call.  The handle sizes its buffers and
// launches its kernels from the same CallPlan.  Plain C++ (no HIP header): tests/test_plan.py runs it on the host.
#pragma once
#include <stdint.h>

#include "../../include/dsx.h"

namespace dsx {

// Launch geometry derived from (num_disp, cost), see pick_geometry.  NW: waves per bm2 block; Dp: padded
// disparity count; TX, TPP: K2 (vol_wta) tile = 32-disparity slices, TPP = Dp / 32 lanes per pixel; DB: key
// shift bits for K2's packed (cost << DB | d) keys
struct Geometry {
    int NW, Dp, TX, TPP, DB;
    int kind;  // BM_SAD / BM_SSD / BM_SAD1 (the fused passes' cost layout)
};

// bm2 cost layouts: SAD disparity pairs (u16), SSD one disparity per lane (u32), SAD1 = SAD in the SSD
// layout (u32 sums, one disparity per lane; fused passes with D <= 64)
enum { BM_SAD = 0, BM_SSD = 1, BM_SAD1 = 2 };

// bm2 geometry: SAD lanes own disparity pairs (Dp = 128 * nw, nw in {1,2,4}); SSD lanes own
// one disparity (Dp = 64 * nw, nw in {1,2,4,8}).  K2 (vol_wta) reuses Dp with 32-d slices.
// SAD with D <= 64 on the fused path takes the SSD layout with u32 |.| sums (BM_SAD1, Dp = 64): the
// pair layout would spend half of every wave on padding disparities.  no_sad1 (DSX_NO_SAD1=1) disables it.
// false: num_disp is too large for the cost.
inline bool pick_geometry(const dsx_params &p, bool no_sad1, Geometry &g) {
    const int D = p.num_disp, cost = p.cost;
    const bool sad1 = !no_sad1 && cost == DSX_COST_SAD && D <= 64 && p.path == DSX_PATH_FUSED &&
                      p.aggregation == DSX_AGG_NONE;
    const bool lane1 = cost == DSX_COST_SSD || sad1;  // one disparity per lane
    g.kind = cost == DSX_COST_SSD ? BM_SSD : (sad1 ? BM_SAD1 : BM_SAD);
    const int unit = lane1 ? 64 : 128;
    const int maxnw = lane1 ? 8 : 4;
    int nw = 1;
    while (nw * unit < D) nw *= 2;
    if (nw > maxnw) return false;
    g.NW = nw;
    g.Dp = nw * unit;
    g.TX = 32;
    g.TPP = g.Dp / 32;
    for (g.DB = 1; (1 << g.DB) < g.Dp;) ++g.DB;  // smallest DB with (1 << DB) >= Dp
    return true;
}

// The geometry of a handle's volume-path launches: its own, except BM_SAD1 (the volume path has the pair layout).
inline bool pick_volume_geometry(const dsx_params &p, Geometry &g) {
    dsx_params q = p;
    q.path = DSX_PATH_VOLUME;
    return pick_geometry(q, false, g);
}

inline int bt_ftzero(const dsx_params &p) { return (p.prefilter_cap > 15 ? p.prefilter_cap : 15) | 1; }

inline bool is_census(int cost) { return cost == DSX_COST_CENSUS9X7 || cost == DSX_COST_CENSUS5X5; }
// costs that exist only as a volume (no fused pass, no right-view pass): BT and census
inline bool volume_only(int cost) { return cost == DSX_COST_BT || is_census(cost); }

inline uint64_t max_cost(const dsx_params &p) {
    const uint64_t n = (uint64_t)p.block_size * p.block_size;
    if (is_census(p.cost)) return n * (p.cost == DSX_COST_CENSUS9X7 ? 62ull : 24ull);  // Hamming bits per pixel
    if (p.cost == DSX_COST_BT) return n * (uint64_t)(2 * bt_ftzero(p) + 63);  // oracle/bt_cost.py max_cost_bt
    return n * (p.cost == DSX_COST_SSD ? 255ull * 255ull : 255ull);
}

inline int sgm_p1(const dsx_params &p) { return p.p1 > 0 ? p.p1 : 8 * p.block_size * p.block_size; }
inline int sgm_p2(const dsx_params &p) { return p.p2 > 0 ? p.p2 : 32 * p.block_size * p.block_size; }

// All directions in one launch with u16 L_r per direction while max cost + P2 stays below 0xFFFF
// (L_r <= C + P2), else the sequential u32 accumulation, which force_seq (DSX_SGM_SEQ=1) forces.
inline bool sgm_concurrent(const dsx_params &p, bool force_seq) {
    return !force_seq && max_cost(p) + (uint64_t)sgm_p2(p) < 0xFFFFull;
}

// SGM path sets by mode (oracle/sgm.py DIRECTIONS order): indices into kSgmDirs
constexpr int kSgmDirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};
constexpr int kSgmSet3[] = {0, 1, 2}, kSgmSet4[] = {0, 1, 2, 3}, kSgmSet5[] = {0, 1, 2, 4, 5},
              kSgmSet8[] = {0, 1, 2, 3, 4, 5, 6, 7};
inline int sgm_set(int mode, const int **set) {
    switch (mode) {
        case DSX_AGG_HH4: *set = kSgmSet4; return 4;
        case DSX_AGG_SGBM: *set = kSgmSet5; return 5;
        case DSX_AGG_HH: *set = kSgmSet8; return 8;
        default: *set = kSgmSet3; return 3;
    }
}

enum CallKind { CALL_COMPUTE = 0, CALL_BATCH, CALL_RIGHT_MAP, CALL_PAIR_FAST, CALL_PAIR_FULL };
enum Builder { BUILD_NONE = 0, BUILD_BLOCK, BUILD_BT, BUILD_CENSUS };  // BLOCK: SAD / SSD (bm2's volume side)
enum LrForm { LR_NONE = 0, LR_BM, LR_SGBM };
enum SgmForm { SGM_NONE = 0, SGM_CONCURRENT, SGM_SEQUENTIAL };
// The handle's cached buffers, by the group sized together (the host entry points' staging is theirs alone).
enum : uint32_t {
    BUF_PREFILTER = 1u << 0,  // filtered views of every frame
    BUF_LR = 1u << 1,         // both key halves + the left winners, `nframes` frames
    BUF_VOLUME = 1u << 2,     // one frame's cost volume (the volume geometry)
    BUF_BT = 1u << 3,         // BT prep records | horizontal sums
    BUF_CENSUS = 1u << 4,     // census code planes of both views
    BUF_POST = 1u << 5,       // sgbm_post: `nframes` int16 maps + the tail's workspace
    BUF_SGM_L = 1u << 6,      // concurrent SGM: `sgm_ndir` u16 volumes
    BUF_SGM_S = 1u << 7,      // sequential SGM: one u32 volume
    BUF_PAIR_DISP = 1u << 8,  // process_pair, fast mode: the matcher's float map
    BUF_PAIR_FIXED = 1u << 9, // process_pair, full mode: the matcher's x16 map
    BUF_PAIR_WS = 1u << 10,   // process_pair, full mode: the post-processing workspace
};

struct CallPlan {
    int nframes;
    bool conf;        // K2's confidence variant: a confidence output, or the handle's threshold > 0
    bool fused;       // the fused pass runs; else (except the right map) the volume path: builder, SGM, K2
    int builder;      // Builder of the volume path
    int lr;           // LrForm in effect; on the fused path it selects the key format and the fix-up kernel
    int sgm;          // SgmForm
    int sgm_ndir;     // directions of the aggregation mode (0 without SGM)
    const int *sgm_dirs;  // sgm_ndir indices into kSgmDirs
    bool scratch;     // the matcher touches handle scratch: ordered by the handle's event (process_pair always is)
    bool prefilter;   // both views are filtered first
    bool texture;     // the texture mask runs after the last matcher kernel (given a disparity output)
    bool post;        // the sgbm_post tail runs, from the handle's int16 maps
    bool defer_lr_ok; // process_pair, full mode: the fused pass's LR check may move into the speckle pass
    uint32_t buffers; // BUF_* the call needs at its shape
};

// conf_out: the call was handed a confidence output.  sgm_seq: DSX_SGM_SEQ.  The sets have passed dsx_check_*.
inline CallPlan plan_call(const dsx_params &p, const dsx_prefilter &pf, const dsx_confidence &cf, int kind,
                          bool conf_out, int nframes, bool sgm_seq) {
    CallPlan pl{};
    pl.nframes = nframes;
    const bool right = kind == CALL_RIGHT_MAP;
    // a confidence call takes the volume path on any handle (the variant lives in K2); the right pass has none
    const bool fused_handle = p.path == DSX_PATH_FUSED && !p.aggregation && !volume_only(p.cost);
    pl.conf = !right && (conf_out || cf.threshold > 0);
    const int lr = p.lr_form == DSX_LR_FORM_SGBM ? LR_SGBM  // OpenCV's form: always on
                                                 : (p.disp12_max_diff >= 0 ? LR_BM : LR_NONE);
    const bool agg = p.aggregation != DSX_AGG_NONE;
    const bool concurrent = agg && sgm_concurrent(p, sgm_seq);
    if (agg) pl.sgm_ndir = sgm_set(p.aggregation, &pl.sgm_dirs);
    pl.prefilter = pf.type != DSX_PREFILTER_NONE;  // the filtered images are handle scratch too

    // Buffers follow the handle's parameters, not this call's launches: a fused handle keeps its LR buffers
    // through confidence calls, and a right-map call sizes what a compute call without confidence would.
    if (pl.prefilter) pl.buffers |= BUF_PREFILTER;
    if (lr != LR_NONE && fused_handle) pl.buffers |= BUF_LR;
    if (!fused_handle || pl.conf) pl.buffers |= BUF_VOLUME;
    if (p.cost == DSX_COST_BT) pl.buffers |= BUF_BT;
    if (is_census(p.cost)) pl.buffers |= BUF_CENSUS;
    if (p.sgbm_post) pl.buffers |= BUF_POST;
    if (agg) pl.buffers |= concurrent ? BUF_SGM_L : BUF_SGM_S;
    if (kind == CALL_PAIR_FAST) pl.buffers |= BUF_PAIR_DISP;
    if (kind == CALL_PAIR_FULL) pl.buffers |= BUF_PAIR_FIXED | BUF_PAIR_WS;

    if (right) {  // one bm_pass_right launch behind the prefilter
        pl.scratch = pl.prefilter;
        return pl;
    }
    pl.fused = fused_handle && !pl.conf;
    pl.builder = pl.fused ? BUILD_NONE
                          : (p.cost == DSX_COST_BT ? BUILD_BT : (is_census(p.cost) ? BUILD_CENSUS : BUILD_BLOCK));
    pl.lr = lr;
    pl.sgm = !agg ? SGM_NONE : (concurrent ? SGM_CONCURRENT : SGM_SEQUENTIAL);
    pl.post = p.sgbm_post != 0;
    pl.texture = pl.prefilter && pf.texture_threshold > 0;
    // only the plain fused pass (no LR check, no sgbm_post, no prefilter) owns no scratch and runs unordered
    pl.scratch = lr != LR_NONE || !pl.fused || pl.post || pl.prefilter;
    // a texture threshold masks the checked map: the fix-up then runs in the matcher, before the mask
    pl.defer_lr_ok = kind == CALL_PAIR_FULL && pl.fused && !pl.post && lr != LR_NONE && pf.texture_threshold == 0;
    return pl;
}

}  // namespace dsx
