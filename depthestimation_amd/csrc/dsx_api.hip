// C-ABI implementation of include/dsx.h: matcher handles, device buffer cache, pass
// sequencing and per-kernel HIP-event timing.  The reference equivalents are cited in dsx.h.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dsx.h"
#include "dsx_internal.h"
#include "dsx_partition.h"
#include "dsx_plan.h"

extern char **environ;  // the DSX_* tuning variables: dsx_env()

#ifndef DSX_RESET_LEFT  // 1: the LR pass resets the other key half; 0: lr_fixup does
#define DSX_RESET_LEFT 1
#endif

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define DSX_HIP(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(e_ == hipErrorOutOfMemory ? DSX_ENOMEM : DSX_EHIP,                  \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                 \
    } while (0)

using namespace dsx;  // the pure decisions of dsx_plan.h

bool env_flag(const char *name) {
    const char *e = getenv(name);
    return e && *e == '1';
}

bool pick_geometry(const dsx_params &p, dsx::Geometry &g) {
    static const bool no_sad1 = env_flag("DSX_NO_SAD1");
    return dsx::pick_geometry(p, no_sad1, g);
}

// odd and in [1, 15]: the matcher's block and dsx_texture_sum_device's
int check_block_size(int bs) {
    if (bs < 1 || bs > 15 || (bs & 1) == 0) return fail(DSX_EINVAL, "block_size must be odd and in [1, 15]");
    return DSX_OK;
}

int check(const dsx_params *p) {
    if (!p) return fail(DSX_EINVAL, "params is NULL");
    if (int rc = check_block_size(p->block_size)) return rc;
    if (p->num_disp < 1 || p->num_disp > 512) return fail(DSX_EINVAL, "num_disp must be in [1, 512]");
    if (p->cost != DSX_COST_SAD && p->cost != DSX_COST_SSD && p->cost != DSX_COST_BT && !is_census(p->cost))
        return fail(DSX_EINVAL, "cost must be SAD (0), SSD (1), BT (2), CENSUS9X7 (3) or CENSUS5X5 (4)");
    if (p->cost == DSX_COST_BT && (p->prefilter_cap < 1 || p->prefilter_cap > 63))
        return fail(DSX_EINVAL, "prefilter_cap must be in [1, 63]");
    if (p->sgbm_post != 0 && p->sgbm_post != 1) return fail(DSX_EINVAL, "sgbm_post must be 0 or 1");
    if (p->sgbm_post) {
        if (p->float_mode != DSX_FLOAT_FIXED)
            return fail(DSX_EINVAL, "sgbm_post filters the int16 map: float_mode must be fixed");
        if (p->speckle_window_size < 0 || p->speckle_range < 0 || p->speckle_range > 2047)
            return fail(DSX_EINVAL, "speckle_window_size must be >= 0 and speckle_range in [0, 2047]");
    }
    if (p->uniqueness_ratio < 0 || p->uniqueness_ratio >= 100)
        return fail(DSX_EINVAL, "uniqueness_ratio must be in [0, 100)");
    if (p->float_mode != DSX_FLOAT_FIXED && p->float_mode != DSX_FLOAT_PARABOLA)
        return fail(DSX_EINVAL, "float_mode must be 0 or 1");
    if (p->path != DSX_PATH_FUSED && p->path != DSX_PATH_VOLUME) return fail(DSX_EINVAL, "path must be 0 or 1");
    if (p->lr_form != DSX_LR_FORM_BM && p->lr_form != DSX_LR_FORM_SGBM)
        return fail(DSX_EINVAL, "lr_form must be 0 (bm) or 1 (sgbm)");
    if (p->in_flight != 0 && p->in_flight != 1) return fail(DSX_EINVAL, "in_flight must be 0 or 1");
    if (p->grid_blocks < 0) return fail(DSX_EINVAL, "grid_blocks must be >= 0");
    if (p->min_disp < -2047 || p->min_disp + p->num_disp > 2047)
        return fail(DSX_EINVAL, "min_disp/num_disp out of the int16 x16 fixed-point range");
    if (p->aggregation != DSX_AGG_NONE) {
        if (p->aggregation != DSX_AGG_SGBM_3WAY && p->aggregation != DSX_AGG_HH4 && p->aggregation != DSX_AGG_SGBM &&
            p->aggregation != DSX_AGG_HH)
            return fail(DSX_EINVAL, "aggregation must be 0, 3 (sgbm_3way), 4 (hh4), 5 (sgbm) or 8 (hh)");
        if (p->cost == DSX_COST_SSD) return fail(DSX_EINVAL, "SGM aggregation runs on SAD, BT or census block costs");
        if (p->num_disp > 256) return fail(DSX_EINVAL, "SGM aggregation supports num_disp <= 256");
        if (p->p1 > 65535 || p->p2 > 65535 || (p->p1 > 0 && p->p2 > 0 && p->p2 < p->p1))
            return fail(DSX_EINVAL, "SGM penalties must satisfy 0 < P1 <= P2 <= 65535");
    }
    dsx::Geometry g;
    if (!pick_geometry(*p, g)) return fail(DSX_EINVAL, "num_disp too large");
    if (max_cost(*p) >= (1ull << (32 - g.DB)) - 1)
        return fail(DSX_EINVAL, "block_size/cost/num_disp combination exceeds the 32-bit (cost<<DB|d) key");
    return DSX_OK;
}

// p may be NULL (the filter's own ranges only)
int check_prefilter(const dsx_params *p, const dsx_prefilter *f) {
    if (!f) return fail(DSX_EINVAL, "prefilter is NULL");
    if (f->type != DSX_PREFILTER_NONE && f->type != DSX_PREFILTER_XSOBEL && f->type != DSX_PREFILTER_MEAN)
        return fail(DSX_EINVAL, "prefilter type must be NONE (0), XSOBEL (1) or MEAN (2)");
    if (f->texture_threshold < 0 || f->texture_threshold > 65535)
        return fail(DSX_EINVAL, "texture_threshold must be in [0, 65535]");
    if (p && is_census(p->cost) && (f->type != DSX_PREFILTER_NONE || f->texture_threshold > 0))
        return fail(DSX_EINVAL, "census ranks intensities itself: a census cost cannot be combined with a prefilter "
                                "or a texture threshold");
    if (f->type == DSX_PREFILTER_NONE) {
        if (f->texture_threshold > 0)
            return fail(DSX_EINVAL, "texture_threshold > 0 needs a prefilter (the cap has no meaning on raw images)");
        return DSX_OK;
    }
    if (f->size < 5 || f->size > 21 || (f->size & 1) == 0)
        return fail(DSX_EINVAL, "prefilter size must be odd and in [5, 21]");
    if (f->cap < 1 || f->cap > 63) return fail(DSX_EINVAL, "prefilter cap must be in [1, 63]");
    if (p && p->cost == DSX_COST_BT)
        return fail(DSX_EINVAL, "cost BT filters for itself: it cannot be combined with a prefilter");
    return DSX_OK;
}

// p may be NULL (the set's own ranges only)
int check_confidence(const dsx_params *p, const dsx_confidence *c) {
    if (!c) return fail(DSX_EINVAL, "confidence is NULL");
    if (c->type != DSX_CONF_PEAK_RATIO) return fail(DSX_EINVAL, "confidence type must be PEAK_RATIO (1)");
    if (c->threshold < 0 || c->threshold > 255) return fail(DSX_EINVAL, "confidence threshold must be in [0, 255]");
    if (p) return check(p);
    return DSX_OK;
}

struct TimedLaunch {
    int kernel;
    hipEvent_t a, b;
};

// One cached device allocation of a handle: the pointer and the bytes it holds (0: not allocated).
struct DevBuf {
    void *ptr = nullptr;
    size_t held = 0;
    template <class T>
    T *as() const { return static_cast<T *>(ptr); }
    // Grows to at least `need` bytes (it may stay larger; the contents are scratch and are not kept).
    // hipFree waits for the device, so no earlier launch still uses the old block.  *fresh: it reallocated.
    int grow(size_t need, bool *fresh = nullptr) {
        if (fresh) *fresh = false;
        if (held >= need) return DSX_OK;
        release();
        DSX_HIP(hipMalloc(&ptr, need));
        held = need;
        if (fresh) *fresh = true;
        return DSX_OK;
    }
    void release() {
        (void)hipFree(ptr);
        ptr = nullptr;
        held = 0;
    }
};

}  // namespace

struct dsx_handle {
    int device = 0;
    dsx_params p{};
    dsx_prefilter pf{};  // type NONE: no filter, no mask, no buffer
    dsx_confidence cf{};  // threshold 0: no effect
    dsx::Geometry g{};
    // geometry of the volume path: g, except on a fused SAD handle with D <= 64 (BM_SAD1), whose confidence
    // calls run K1 / K2 in the pair layout the volume path always has
    dsx::Geometry gv{};
    hipStream_t stream = nullptr;  // for dsx_compute_host
    // buffer cache keyed by (H, W, geometry); single entry like RectificationCache (rectify.py:49-50)
    int cH = 0, cW = 0, cDp = 0, cCostBytes = 0;
    int lrFrames = 0;  // frames the LR buffers hold: the stride between the two key halves
    int lrParity = 0;  // which half of lrKeys the next frame's left pass fills
    int lrDirty[2] = {0, 0};  // frames of each half holding keys that were not reset yet
    // Handle-owned scratch (LR keys / left winners, cost volume, BT records, SGM sums, the
    // sgbm_post input and workspace) is reused by every call: a call that touches it on another
    // stream than the previous such call waits for that call's last kernel (event) first.  Only
    // the plain fused pass (no LR check, no sgbm_post, no prefilter) owns no scratch and runs unordered.
    hipEvent_t scratchDone = nullptr;
    hipStream_t scratchStream = nullptr;
    bool scratchPending = false;
    // The cached buffers, named once (DSX_BUFS).  begin_call drops them all when the shape or the geometry
    // changes, ensure_buffers grows those the call's plan names, dsx_workspace_bytes sums what they hold.
    //   stageL / R / Fixed / Float, dConf: dsx_compute_host's views and maps, dsx_compute_conf_host's map
    //   pfBuf: the filtered left views of every frame, then the right views (rows pf_pitch(W) apart)
    //   lrKeys: right-view winner keys per pixel (atomicMin target), two halves of lrFrames frames;  dStar: left
    //   winners (or -1);  vol: one frame's cost volume;  btWs: BT prep records | horizontal sums;  censusWs: codes L | R
    //   postIn, postWs: sgbm_post's input maps of every frame; median | speckle components
    //   ppDisp, ppFixed, ppWs: dsx_process_pair_device's float map (fast), x16 map (full), workspace
    //   sgmS: SGM path sums [H][W][Dp] u32 (sequential);  sgmL: ndir x [H][W][Dp] u16 L_r (concurrent)
#define DSX_BUFS(X)                                                                                             \
    X(stageL) X(stageR) X(stageFixed) X(stageFloat) X(dConf) X(pfBuf) X(lrKeys) X(dStar) X(vol) X(btWs) X(censusWs) \
    X(postIn) X(postWs) X(ppDisp) X(ppFixed) X(ppWs) X(sgmS) X(sgmL)
#define X(name) DevBuf name;
    DSX_BUFS(X)
#undef X
    const uint32_t *lastKeys = nullptr;  // the last fused call's LR key half (run, defer_lr)
    const int16_t *lastDstar = nullptr;
    int lastKshift = 0;
    // timing
    std::vector<std::string> knames;
    std::vector<double> ktotal;
    std::vector<int> kcount;
    std::vector<TimedLaunch> pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> free_events;
};

namespace {

template <class F>
void for_each_buf(dsx_handle *h, F f) {
#define X(name) f(h->name);
    DSX_BUFS(X)
#undef X
}

void free_buffers(dsx_handle *h) {
    for_each_buf(h, [](DevBuf &b) { b.release(); });
    h->cH = h->cW = h->cDp = h->cCostBytes = 0;
    h->lrFrames = 0;
    h->lrDirty[0] = h->lrDirty[1] = 0;
    h->scratchPending = false;
}

int cost_bytes(const dsx_params &p) { return p.cost == DSX_COST_SSD ? 4 : 2; }

// Row pitch of the filtered images: whole 16-B groups, so every row takes the wide stores.
int64_t pf_pitch(int W) { return ((int64_t)W + 15) & ~(int64_t)15; }

// New LR buffers of `nframes` frames: every key ~0 (the passes restore that after every frame), both halves clean.
int init_lr_keys(dsx_handle *h, int nframes) {
    // The handle's streams are non-blocking, so the fill must have landed before any later launch:
    // wait for it here (allocation time only)
    DSX_HIP(hipMemsetAsync(h->lrKeys.ptr, 0xFF, h->lrKeys.held, nullptr));
    DSX_HIP(hipStreamSynchronize(nullptr));
    h->lrFrames = nframes;
    h->lrParity = 0;
    h->lrDirty[0] = h->lrDirty[1] = 0;
    return DSX_OK;
}

// Grows the buffers the plan names to what the call needs at H x W (other translation units' sizes included).
int ensure_buffers(dsx_handle *h, int H, int W, const dsx::CallPlan &pl) {
    const size_t n = (size_t)H * W, nf = (size_t)pl.nframes;
    const auto need = [&pl](uint32_t b) { return (pl.buffers & b) != 0; };
    int rc = DSX_OK;
    if (need(dsx::BUF_LR)) {
        bool fresh = false;  // two key halves: this frame / next frame
        if ((rc = h->lrKeys.grow(2 * n * nf * 4, &fresh)) || (rc = h->dStar.grow(n * nf * 2)) ||
            (fresh && (rc = init_lr_keys(h, pl.nframes)))) {
            h->lrKeys.release();  // never keys without their fill and their frame count
            h->lrFrames = 0;
            return rc;
        }
    }
    if (need(dsx::BUF_PREFILTER) && (rc = h->pfBuf.grow(2 * nf * H * (size_t)pf_pitch(W)))) return rc;
    if (need(dsx::BUF_VOLUME) && (rc = h->vol.grow(n * h->gv.Dp * cost_bytes(h->p)))) return rc;
    if (need(dsx::BUF_BT) && (rc = h->btWs.grow(dsx::bt_workspace(H, W, h->g.Dp)))) return rc;
    if (need(dsx::BUF_CENSUS) && (rc = h->censusWs.grow(2 * n * dsx::census_code_bytes(h->p.cost)))) return rc;
    if (need(dsx::BUF_POST) &&
        ((rc = h->postIn.grow(n * nf * 2)) || (rc = h->postWs.grow(dsx::sgbm_post_workspace(H, W)))))
        return rc;
    // one u16 plane set per direction: the buffer follows the mode's direction count
    // (sgm_paths_all writes L + dir * lstride for every dir below the count)
    if (need(dsx::BUF_SGM_L) && (rc = h->sgmL.grow((size_t)pl.sgm_ndir * n * h->g.Dp * 2))) return rc;
    if (need(dsx::BUF_SGM_S) && (rc = h->sgmS.grow(n * h->g.Dp * 4))) return rc;
    if (need(dsx::BUF_PAIR_DISP) && (rc = h->ppDisp.grow(n * 4))) return rc;
    if (need(dsx::BUF_PAIR_FIXED) && (rc = h->ppFixed.grow(n * 2))) return rc;
    if (need(dsx::BUF_PAIR_WS) && (rc = h->ppWs.grow(dsx::post_full_workspace(H, W, std::max(0, h->p.num_disp)))))
        return rc;
    h->cH = H;
    h->cW = W;
    h->cDp = h->g.Dp;
    h->cCostBytes = cost_bytes(h->p);
    return DSX_OK;
}

// The front of every handle call, after its argument checks: the handle's device, the call's plan, and the
// buffer cache at the call's shape.  The cache is invalidated here and nowhere else, before anything is grown.
int begin_call(dsx_handle *h, int kind, bool conf_out, int nframes, int H, int W, dsx::CallPlan &pl) {
    DSX_HIP(hipSetDevice(h->device));
    static const bool sgm_seq = env_flag("DSX_SGM_SEQ");
    pl = dsx::plan_call(h->p, h->pf, h->cf, kind, conf_out, nframes, sgm_seq);
    if (h->cH != H || h->cW != W || h->cDp != h->g.Dp || h->cCostBytes != cost_bytes(h->p)) free_buffers(h);
    return ensure_buffers(h, H, W, pl);
}

uint32_t pad_value(dsx_handle *h, int DB) {
    const uint32_t keymax = (uint32_t)((1ull << (32 - DB)) - 1ull);
    return h->p.cost == DSX_COST_SSD ? keymax : (keymax < 0xFFFFu ? keymax : 0xFFFFu);
}

int kernel_id(dsx_handle *h, const char *name) {
    for (size_t i = 0; i < h->knames.size(); ++i)
        if (h->knames[i] == name) return (int)i;
    h->knames.emplace_back(name);
    h->ktotal.push_back(0.0);
    h->kcount.push_back(0);
    return (int)h->knames.size() - 1;
}

int begin_timed(dsx_handle *h, const char *name, hipStream_t st, TimedLaunch &t) {
    t.kernel = kernel_id(h, name);
    if (!h->free_events.empty()) {
        t.a = h->free_events.back().first;
        t.b = h->free_events.back().second;
        h->free_events.pop_back();
    } else {
        // timing-only events: no system-scope fence (cache writeback + invalidate) at each record,
        // which made every timed kernel start on cold caches (C3's left pass read 331 us against 298 us
        // under rocprofv3, profiles/r04_final_bench_c3.json)
        DSX_HIP(hipEventCreateWithFlags(&t.a, hipEventDisableSystemFence));
        DSX_HIP(hipEventCreateWithFlags(&t.b, hipEventDisableSystemFence));
    }
    DSX_HIP(hipEventRecord(t.a, st));
    return DSX_OK;
}

int end_timed(dsx_handle *h, hipStream_t st, TimedLaunch &t) {
    DSX_HIP(hipEventRecord(t.b, st));
    h->pending.push_back(t);
    return DSX_OK;
}

int collect_times(dsx_handle *h) {
    for (auto &t : h->pending) {
        DSX_HIP(hipEventSynchronize(t.b));
        float ms = 0.f;
        DSX_HIP(hipEventElapsedTime(&ms, t.a, t.b));
        h->ktotal[t.kernel] += ms;
        h->kcount[t.kernel] += 1;
        h->free_events.emplace_back(t.a, t.b);
    }
    h->pending.clear();
    return DSX_OK;
}

// Records the handle's scratch event on `st` when it goes out of scope (any return path of a call
// that may have enqueued launches touching handle scratch), so a later call on another stream
// orders after them; finish() does it explicitly and reports a failure to record.
struct ScratchRecord {
    dsx_handle *h;
    hipStream_t st;
    bool active;
    ScratchRecord(dsx_handle *h_, hipStream_t st_, bool active_) : h(h_), st(st_), active(active_) {}
    int record() {
        active = false;
        if (!h->scratchDone) {
            hipError_t e = hipEventCreateWithFlags(&h->scratchDone, hipEventDisableTiming);
            if (e != hipSuccess) return fail(DSX_EHIP, std::string("hipEventCreate: ") + hipGetErrorString(e));
        }
        hipError_t e = hipEventRecord(h->scratchDone, st);
        if (e != hipSuccess) return fail(DSX_EHIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
        h->scratchStream = st;
        h->scratchPending = true;
        return DSX_OK;
    }
    int finish() { return active ? record() : DSX_OK; }
    ~ScratchRecord() {
        if (active) (void)record();
    }
};

// The DSX_* tuning variables a fused launch reads, in one pass over the environment (seven getenv
// scans cost ~2 us of host time per call; tests and tools change them at run time, so no caching)
struct DsxEnv {
    const char *prio = nullptr, *prio_t = nullptr, *slow_w8 = nullptr, *agew = nullptr, *variant = nullptr,
               *timeline = nullptr;
};
DsxEnv dsx_env() {
    DsxEnv e;
    for (char **p = environ; p && *p; ++p) {
        const char *s = *p;
        if (s[0] != 'D' || s[1] != 'S' || s[2] != 'X' || s[3] != '_') continue;
        s += 4;
        const auto take = [s](const char *key, const char *&dst) {
            const size_t n = strlen(key);
            if (strncmp(s, key, n) == 0 && s[n] == '=') dst = s + n + 1;
        };
        take("PRIO", e.prio);
        take("PRIO_T", e.prio_t);
        take("SLOW_W8", e.slow_w8);
        take("AGEW", e.agew);
        take("VARIANT", e.variant);
        take("TIMELINE", e.timeline);
    }
    return e;
}

// the strips a fused launch covers (bm2_strips, dsx_partition.h): all of them, or those meeting the valid band
void set_strips(dsx::Bm2Args &a, const dsx_handle *h, bool band_only) {
    const dsx::Bm2Strips s = dsx::bm2_strips(a.W, h->p.min_disp, h->p.num_disp, band_only, dsx::kStripWidth);
    a.strip_begin = s.begin;
    a.strip_count = s.count;
}

// side: the pass (dsx::Side); sg_keys: the left pass takes OpenCV-form LR keys (the caller sets the pointer)
dsx::Bm2Args base_args(dsx_handle *h, int H, int W, int64_t stride, int side, bool sg_keys = false,
                       const DsxEnv &env = dsx_env()) {
    dsx::Bm2Args a{};
    a.side = side;
    a.stride = stride;
    a.H = H;
    a.W = W;
    a.m = h->p.min_disp;
    a.D = h->p.num_disp;
    a.uniq = h->p.uniqueness_ratio;
    a.lr = h->p.disp12_max_diff;
    a.subpix = h->p.subpixel;
    a.float_mode = h->p.float_mode;
    a.padv = pad_value(h, h->g.DB);
    // the plain left pass up to R = 5 takes block minima as f16 bit patterns: finite padding (dsx_internal.h)
    if (dsx::bm2_blockmin(h->p.block_size / 2, h->g.kind, h->g.NW, side, sg_keys)) a.padv = dsx::kBlockminPad;
    set_strips(a, h, false);
    a.grid_override = h->p.grid_blocks;
    {
        // Balance (measured on C2-C5, profiles/README.md r01d): co-resident waves drop their issue
        // priority as they pass 50 / 80 / 95 % of their rows, and strips on the clamped-load
        // path count 11/8 of a fast strip.  DSX_PRIO=0 / DSX_PRIO_T / DSX_SLOW_W8 override.
        // in_flight handles: no priority bands and equal age weights (profiles/r04af_balance_in_flight.txt:
        // C4 19.5k -> 20.8k Mpix/s with 3 frames in flight; a lone launch needs the balance)
        const bool fl = h->p.in_flight != 0;
        a.in_flight = fl ? 1 : 0;
        a.prio = env.prio ? atoi(env.prio) : (fl ? 0 : 1);
        a.pt1 = 128, a.pt2 = 205, a.pt3 = 243;
        if (env.prio_t) sscanf(env.prio_t, "%d,%d,%d", &a.pt1, &a.pt2, &a.pt3);
        a.slow_w8 = env.slow_w8 ? atoi(env.slow_w8) : 11;
        // age-level work weights (single frames; r01f A/B: C2 83.6 -> 81.7 us, C4 61.4 -> 59.9 us)
        a.agew[0] = fl ? 64 : 78, a.agew[1] = fl ? 64 : 70, a.agew[2] = a.agew[3] = 64;
        if (env.agew) sscanf(env.agew, "%d,%d,%d,%d", &a.agew[0], &a.agew[1], &a.agew[2], &a.agew[3]);
        a.nlev = 0;  // set by the launcher from the residency it computes
        a.variant = env.variant ? atoi(env.variant) : 0;
    }
    a.nframes = 1;
    a.frame_stride = 0;
    return a;
}

#define DSX_LAUNCH(h, name, st, call)                                    \
    do {                                                                 \
        TimedLaunch t_;                                                  \
        if ((h)->p.timing) {                                             \
            int rc_ = begin_timed((h), (name), (st), t_);                \
            if (rc_) return rc_;                                         \
        }                                                                \
        hipError_t e_ = (call);                                          \
        if (e_ != hipSuccess) return fail(DSX_EHIP, std::string(name) + " launch: " + hipGetErrorString(e_)); \
        if ((h)->p.timing) {                                             \
            int rc_ = end_timed((h), (st), t_);                          \
            if (rc_) return rc_;                                         \
        }                                                                \
    } while (0)

// The handle's per-kernel timing around the post-processing launch groups (launch_post_full).
struct TimingHook : dsx::LaunchHook {
    dsx_handle *h;
    TimedLaunch t{};
    int rc = DSX_OK;
    bool open = false;
    explicit TimingHook(dsx_handle *h_) : h(h_) {}
    void before(const char *name, hipStream_t st) override {
        if (rc == DSX_OK) rc = begin_timed(h, name, st, t);
        open = rc == DSX_OK;
    }
    void after(hipStream_t st) override {
        if (open && rc == DSX_OK) rc = end_timed(h, st, t);
        open = false;
    }
};

// key: the caller's workspace (dsx_fill_holes_device, dsx_postprocess_full_ex_device) or the handle
// (dsx_process_pair_device); nullptr: any
int sticky_inpaint_timeout(const void *key) {
    if (key ? dsx::inpaint_take_timeout(key) : dsx::inpaint_take_timeout_any())
        return fail(DSX_EHIP, "hole filling: the persistent march timed out; the holes of that call were left "
                              "unfilled (its results are invalid)");
    return DSX_OK;
}

int check_fill_shape(int64_t H, int64_t W) {
    if (H * W >= dsx::kInpaintMaxPixels) return fail(DSX_EINVAL, "image too large for hole filling (H * W >= 2^27)");
    return DSX_OK;
}

// Orders a call that touches handle scratch on `st` after the previous such call on another stream.
int wait_scratch(dsx_handle *h, hipStream_t st) {
    if (h->scratchPending && h->scratchStream != st) DSX_HIP(hipStreamWaitEvent(st, h->scratchDone, 0));
    return DSX_OK;
}

// Filters both views of every frame into the handle's buffers (one launch) and redirects the inputs
// to them: the passes that follow read the filtered images like any caller's.
int run_prefilter(dsx_handle *h, const void *&dL, const void *&dR, int H, int W, int64_t &stride, hipStream_t st,
                  int nframes, int64_t &frame_stride) {
    const int64_t P = pf_pitch(W);
    dsx::PrefilterArgs a{};
    a.src[0] = static_cast<const uint8_t *>(dL);
    a.src[1] = static_cast<const uint8_t *>(dR);
    a.stride = stride;
    a.frame_stride = nframes > 1 ? frame_stride : 0;
    a.dst[0] = h->pfBuf.as<uint8_t>();
    a.dst[1] = a.dst[0] + (size_t)nframes * H * P;
    a.dpitch = P;
    a.dframe = (int64_t)H * P;
    a.dwidth = (int)P;
    a.nviews = 2;
    a.nframes = nframes;
    a.H = H;
    a.W = W;
    a.type = h->pf.type;
    a.n = h->pf.size;
    a.cap = h->pf.cap;
    DSX_LAUNCH(h, "prefilter", st, dsx::launch_prefilter(a, st));
    dL = a.dst[0];
    dR = a.dst[1];
    stride = P;
    frame_stride = a.dframe;
    return DSX_OK;
}

// rows per census_volume segment: DSX_CENSUS_SEG = 16 | 32 | 64 (the sweep of DESIGN 4.3e), else the default
int census_seg() {
    const char *e = getenv("DSX_CENSUS_SEG");
    const int v = e ? atoi(e) : 0;
    return v == 16 || v == 32 || v == 64 ? v : 0;
}

int run_right_pass(dsx_handle *h, const dsx::CallPlan &pl, const void *dL, const void *dR, int H, int W,
                   int64_t stride, int16_t *out, hipStream_t st) {
    if (volume_only(h->p.cost))
        return fail(DSX_EINVAL, "the right-view map is a block-matching (SAD/SSD) pass");
    int rc = DSX_OK;
    if (pl.scratch && (rc = wait_scratch(h, st))) return rc;
    ScratchRecord rec_(h, st, pl.scratch);
    int64_t fs = 0;
    if (pl.prefilter && (rc = run_prefilter(h, dL, dR, H, W, stride, st, 1, fs))) return rc;
    dsx::Bm2Args a = base_args(h, H, W, stride, dsx::SIDE_RIGHT);
    a.ref = static_cast<const uint8_t *>(dR);
    a.src = static_cast<const uint8_t *>(dL);
    a.out_dR = out;
    const int radius = h->p.block_size / 2;
    DSX_LAUNCH(h, "bm_pass_right", st, dsx::launch_bm2(radius, h->g.kind, h->g.NW, a, st));
    return rec_.finish();
}

// One matcher call as run()'s stages see it: the inputs after the prefilter and the matcher kernels' outputs
// (with sgbm_post the handle's int16 maps); frames frame_stride bytes apart, outputs H * W elements apart.
struct Call {
    dsx_handle *h;
    const dsx::CallPlan &pl;
    const void *dL, *dR;
    int H, W;
    int64_t stride, frame_stride;
    void *outFixed, *outFloat, *outConf;
    hipStream_t st;
    bool defer_lr;
    const uint8_t *view(const void *base, int f) const { return static_cast<const uint8_t *>(base) + f * frame_stride; }
};

// The fused pass's LR keys are double-buffered: a call fills one half of lrKeys, its fix-up consumes it,
// and the next call's left pass resets it (every frame a call dirtied, however many the next call has).
struct LrHalves {
    uint32_t *keys, *reset;  // this call's half; the other one, with reset_n keys of the previous call not reset yet
    int64_t reset_n;
};
LrHalves lr_halves(const dsx_handle *h, int H, int W) {
    const size_t half = (size_t)H * W * h->lrFrames;
    const int P = h->lrParity;
    uint32_t *k = h->lrKeys.as<uint32_t>();
    return {k + P * half, k + (P ^ 1) * half, (int64_t)H * W * h->lrDirty[P ^ 1]};
}
// after the launches of a call that dirtied nframes frames of its half and reset the other
void lr_advance(dsx_handle *h, int nframes) {
    const int P = h->lrParity;
    h->lrDirty[P ^ 1] = 0;
    h->lrDirty[P] = nframes;
    h->lrParity = P ^ 1;
}

// The fused pass and its LR fix-up.  defer_lr (dsx_process_pair_device): the left-right check is left to
// the caller's next kernel (spk_tile applies it while loading the map): no fix-up launch; h->lastKeys /
// lastDstar name this call's key half and winners.
int run_fused(const Call &c) {
    dsx_handle *h = c.h;
    const int H = c.H, W = c.W, nframes = c.pl.nframes, lr = c.pl.lr;
    const DsxEnv env = dsx_env();
    // bm: every strip (below), the LR build of the left pass
    const int side = lr == dsx::LR_BM ? dsx::SIDE_LEFT_LR : dsx::SIDE_LEFT;
    dsx::Bm2Args a = base_args(h, H, W, c.stride, side, lr == dsx::LR_SGBM, env);
    a.ref = static_cast<const uint8_t *>(c.dL);
    a.src = static_cast<const uint8_t *>(c.dR);
    a.out_fixed = static_cast<int16_t *>(c.outFixed);
    a.out_float = static_cast<float *>(c.outFloat);
    a.nframes = nframes;
    a.frame_stride = c.frame_stride;
    LrHalves k{};
    int reset_rows = 0;  // rows lr_fixup resets when the left pass does not (DSX_RESET_LEFT 0)
    if (lr != dsx::LR_NONE) {
        // bm: the left pass also builds the right-view winners for lr_fixup.  sgbm (OpenCV's form): unique winners
        // scatter (cost, d) into the keys for lr_fixup_sgbm, the x16 outputs stay in dStar.  Both reset the other half.
        k = lr_halves(h, H, W);
        (lr == dsx::LR_BM ? a.lr_keys : a.sg_keys) = k.keys;
        a.lr_reset = k.reset;
        a.lr_reset_n = (lr == dsx::LR_SGBM || DSX_RESET_LEFT) ? k.reset_n : 0;
        reset_rows = DSX_RESET_LEFT ? 0 : H * h->lrDirty[h->lrParity ^ 1];
        a.dstar = h->dStar.as<int16_t>();
        a.kshift = h->g.kind != dsx::BM_SAD ? h->g.DB : 16;  // u32 layouts: (C << DB) | d
    }
    // bm: every strip, a right pixel's diagonal starts left of the valid band; otherwise only strips meeting the
    // valid band need a search
    if (lr != dsx::LR_BM) set_strips(a, h, true);
    uint64_t *tl = nullptr;
    const char *tlpath = env.timeline;
    if (tlpath && *tlpath) DSX_HIP(hipMalloc(&tl, 12 * 8 * 65536));
    if (tl) DSX_HIP(hipMemsetAsync(tl, 0, 12 * 8 * 65536, c.st));
    a.timeline = tl;
    DSX_LAUNCH(h, "bm_pass_left", c.st, dsx::launch_bm2(h->p.block_size / 2, h->g.kind, h->g.NW, a, c.st));
    h->lastKeys = k.keys;
    h->lastDstar = h->dStar.as<int16_t>();
    h->lastKshift = a.kshift;
    if (lr == dsx::LR_SGBM && !c.defer_lr)
        DSX_LAUNCH(h, "lr_fixup_sgbm", c.st,
                   dsx::launch_lr_fixup_sgbm(a.dstar, k.keys, H * nframes, W, h->p.min_disp, h->p.disp12_max_diff,
                                             a.kshift, a.out_fixed, a.out_float, c.st));
    if (lr == dsx::LR_BM && (!c.defer_lr || !DSX_RESET_LEFT))
        DSX_LAUNCH(h, "lr_fixup", c.st,
                   dsx::launch_lr_fixup(a.dstar, k.keys, k.reset, reset_rows, H * nframes, W, h->p.min_disp,
                                        h->p.disp12_max_diff, a.kshift, a.out_fixed, a.out_float, c.st));
    if (lr != dsx::LR_NONE) lr_advance(h, nframes);
    if (tl) {
        std::vector<uint64_t> host(12 * 65536);
        DSX_HIP(hipStreamSynchronize(c.st));
        DSX_HIP(hipMemcpy(host.data(), tl, host.size() * 8, hipMemcpyDeviceToHost));
        FILE *f = fopen(tlpath, "wb");
        if (f) {
            fwrite(host.data(), 8, host.size(), f);
            fclose(f);
        }
        (void)hipFree(tl);
    }
    return DSX_OK;
}

// the volume, shape and search range of BtArgs / CensusVolArgs
template <class A>
void volume_args(const Call &c, A &a) {
    a.vol = c.h->vol.ptr;
    a.H = c.H;
    a.W = c.W;
    a.m = c.h->p.min_disp;
    a.D = c.h->p.num_disp;
    a.Dp = c.h->gv.Dp;
    a.R = c.h->p.block_size / 2;
    a.padv = pad_value(c.h, c.h->gv.DB);
}

// K1 of the volume path: frame f's costs of the plan's builder into the handle's volume
int build_volume(const Call &c, int f) {
    dsx_handle *h = c.h;
    const int H = c.H, W = c.W;
    const uint8_t *l = c.view(c.dL, f), *r = c.view(c.dR, f);
    if (c.pl.builder == dsx::BUILD_BT) {
        const size_t n = (size_t)H * W;
        uint2 *prepL = h->btWs.as<uint2>(), *prepR = prepL + n;
        const int ftz = bt_ftzero(h->p);
        DSX_LAUNCH(h, "bt_prep", c.st, dsx::launch_bt_prep(l, c.stride, H, W, ftz, prepL, c.st));
        DSX_LAUNCH(h, "bt_prep", c.st, dsx::launch_bt_prep(r, c.stride, H, W, ftz, prepR, c.st));
        dsx::BtArgs b{};
        b.prepL = prepL;
        b.prepR = prepR;
        b.hs = reinterpret_cast<uint16_t *>(prepR + n);
        volume_args(c, b);
        DSX_LAUNCH(h, "bt_hsum", c.st, dsx::launch_bt_volume(b, 0, c.st));
        DSX_LAUNCH(h, "bt_vsum", c.st, dsx::launch_bt_volume(b, 1, c.st));
    } else if (c.pl.builder == dsx::BUILD_CENSUS) {
        dsx::CensusArgs t{};
        t.src[0] = l;
        t.src[1] = r;
        t.stride = c.stride;
        t.dst[0] = h->censusWs.ptr;
        t.dst[1] = h->censusWs.as<uint8_t>() + (size_t)H * W * dsx::census_code_bytes(h->p.cost);
        t.nviews = 2;
        t.H = H;
        t.W = W;
        t.window = h->p.cost;
        t.out64 = h->p.cost == DSX_COST_CENSUS9X7;
        DSX_LAUNCH(h, "census_transform", c.st, dsx::launch_census_transform(t, c.st));
        dsx::CensusVolArgs v{};
        v.codeL = t.dst[0];
        v.codeR = t.dst[1];
        volume_args(c, v);
        v.window = h->p.cost;
        v.seg = census_seg();
        DSX_LAUNCH(h, "census_volume", c.st, dsx::launch_census_volume(v, c.st));
    } else {  // SAD / SSD block costs: bm2's volume side
        dsx::Bm2Args a = base_args(h, H, W, c.stride, dsx::SIDE_VOLUME);
        a.ref = l;
        a.src = r;
        a.vol = h->vol.ptr;
        a.padv = pad_value(h, h->gv.DB);
        const int kind = h->p.cost == DSX_COST_SSD ? dsx::BM_SSD : dsx::BM_SAD;
        DSX_LAUNCH(h, "cost_volume", c.st, dsx::launch_bm2(h->p.block_size / 2, kind, h->gv.NW, a, c.st));
    }
    return DSX_OK;
}

// SGM over the handle's volume: every path of every direction in one launch with L_r per direction (u16),
// or one pass per direction of the mode's path set (oracle/sgm.py DIRECTIONS) into u32 sums
template <class A>
void sgm_args(const Call &c, A &sa) {
    sa.C = c.h->vol.as<const uint16_t>();
    sa.H = c.H;
    sa.W = c.W;
    sa.D = c.h->p.num_disp;
    sa.Dp = c.h->g.Dp;
    sa.P1 = dsx::sgm_p1(c.h->p);
    sa.P2 = dsx::sgm_p2(c.h->p);
}
int run_sgm(const Call &c) {
    dsx_handle *h = c.h;
    const int nd = c.pl.sgm_ndir, *set = c.pl.sgm_dirs;
    if (c.pl.sgm == dsx::SGM_CONCURRENT) {
        dsx::SgmAllArgs sa{};
        sgm_args(c, sa);
        sa.L = h->sgmL.as<uint16_t>();
        sa.lstride = (size_t)c.H * c.W * h->g.Dp;
        sa.ndir = nd;
        for (int i = 0; i < nd; ++i) {
            sa.dx[i] = dsx::kSgmDirs[set[i]][0];
            sa.dy[i] = dsx::kSgmDirs[set[i]][1];
            sa.poff[i + 1] = sa.poff[i] + dsx::sgm_num_paths_host(c.H, c.W, sa.dx[i], sa.dy[i]);
        }
        DSX_LAUNCH(h, "sgm_paths", c.st, dsx::launch_sgm_all(sa, c.st));
    } else if (c.pl.sgm == dsx::SGM_SEQUENTIAL) {
        dsx::SgmArgs sa{};
        sgm_args(c, sa);
        sa.S = h->sgmS.as<uint32_t>();
        sa.pads = (uint32_t)((1ull << (32 - h->g.DB)) - 1ull);
        for (int i = 0; i < nd; ++i) {
            sa.dx = dsx::kSgmDirs[set[i]][0];
            sa.dy = dsx::kSgmDirs[set[i]][1];
            DSX_LAUNCH(h, "sgm_path", c.st, dsx::launch_sgm_path(sa, i == 0, c.st));
        }
    }
    return DSX_OK;
}

// K2: winner, uniqueness, sub-pixel, LR check and confidence of frame f from the volume or the SGM sums
int run_volume_wta(const Call &c, int f) {
    dsx_handle *h = c.h;
    const dsx::Geometry &gv = h->gv;
    const size_t fo = (size_t)f * c.H * c.W;
    const int sgm = c.pl.sgm;
    dsx::VolArgs v{};
    v.vol = sgm == dsx::SGM_CONCURRENT ? h->sgmL.ptr : (sgm == dsx::SGM_SEQUENTIAL ? h->sgmS.ptr : h->vol.ptr);
    v.nsum = sgm == dsx::SGM_CONCURRENT ? c.pl.sgm_ndir : 0;
    v.sstride = (size_t)c.H * c.W * gv.Dp;
    v.H = c.H;
    v.W = c.W;
    v.m = h->p.min_disp;
    v.D = h->p.num_disp;
    v.Dp = gv.Dp;
    v.DB = gv.DB;
    v.TPP = gv.TPP;
    v.uniq = h->p.uniqueness_ratio;
    v.lr = h->p.disp12_max_diff;
    v.lr_form = h->p.lr_form;
    v.subpix = h->p.subpixel;
    v.float_mode = h->p.float_mode;
    v.out_fixed = c.outFixed ? static_cast<int16_t *>(c.outFixed) + fo : nullptr;
    v.out_float = c.outFloat ? static_cast<float *>(c.outFloat) + fo : nullptr;
    v.conf = c.pl.conf ? 1 : 0;
    v.conf_t = h->cf.threshold;
    v.out_conf = c.outConf ? static_cast<uint8_t *>(c.outConf) + fo : nullptr;
    const bool wide = h->p.cost == DSX_COST_SSD || sgm != dsx::SGM_NONE;  // u32 costs: SSD block costs or SGM path sums
    if (dsx::volume_smem_bytes(gv.TX, wide, gv.Dp, gv.TPP, c.W, c.pl.conf) > 160 * 1024)
        return fail(DSX_EINVAL, "image too wide for the volume path's row kernel");
    DSX_LAUNCH(h, "volume_wta", c.st, dsx::launch_volume_wta(gv.TX, wide, v, c.st));
    return DSX_OK;
}

// After the last matcher kernel: the texture mask on its maps, then sgbm_post from the handle's int16 maps.
int run_tail(const Call &c, void *finalFixed, void *finalFloat) {
    dsx_handle *h = c.h;
    if (c.pl.texture && (c.outFixed || c.outFloat)) {  // a map-only confidence call has neither
        dsx::TextureArgs t{};
        t.pref = static_cast<const uint8_t *>(c.dL);  // the filtered left views
        t.stride = c.stride;
        t.frame_stride = c.frame_stride;
        t.nframes = c.pl.nframes;
        t.H = c.H;
        t.W = c.W;
        t.block = h->p.block_size;
        t.cap = h->pf.cap;
        t.thr = h->pf.texture_threshold;
        t.out_fixed = static_cast<int16_t *>(c.outFixed);
        t.out_float = static_cast<float *>(c.outFloat);
        t.inv16 = (h->p.min_disp - 1) * 16;
        t.invf = (float)(h->p.min_disp - 1);
        DSX_LAUNCH(h, "texture_mask", c.st, dsx::launch_texture(t, c.st));
    }
    if (c.pl.post) {
        for (int f = 0; f < c.pl.nframes; ++f) {
            const size_t fo = (size_t)f * c.H * c.W;
            DSX_LAUNCH(h, "sgbm_post", c.st,
                       dsx::launch_sgbm_post(h->postIn.as<int16_t>() + fo, c.H, c.W, (h->p.min_disp - 1) * 16,
                                             h->p.speckle_window_size, 16 * h->p.speckle_range,
                                             finalFixed ? static_cast<int16_t *>(finalFixed) + fo : nullptr,
                                             finalFloat ? static_cast<float *>(finalFloat) + fo : nullptr,
                                             h->postWs.ptr, c.st));
        }
    }
    return DSX_OK;
}

// The matcher of a compute, batch or process_pair call, launched stage by stage from the call's plan.
int run(dsx_handle *h, const dsx::CallPlan &pl, const void *dL, const void *dR, int H, int W, int64_t stride,
        void *outFixed, void *outFloat, hipStream_t st, int64_t frame_stride = 0, bool defer_lr = false,
        void *outConf = nullptr) {
    int rc = DSX_OK;
    if (pl.scratch && (rc = wait_scratch(h, st))) return rc;
    ScratchRecord rec_(h, st, pl.scratch);  // on every exit once launches may have been enqueued
    if (pl.prefilter && (rc = run_prefilter(h, dL, dR, H, W, stride, st, pl.nframes, frame_stride))) return rc;
    // sgbm_post: the matcher writes int16 maps into postIn, the tail then writes the outputs
    const Call c{h, pl, dL, dR, H, W, stride, frame_stride, pl.post ? h->postIn.ptr : outFixed,
                 pl.post ? nullptr : outFloat, outConf, st, defer_lr};
    if (pl.fused) {
        if ((rc = run_fused(c))) return rc;
    } else {
        // volume path: one K1 (+ SGM) + K2 group per frame (the volume buffer holds one frame)
        for (int f = 0; f < pl.nframes; ++f) {
            rc = build_volume(c, f);
            if (!rc) rc = run_sgm(c);
            if (!rc) rc = run_volume_wta(c, f);
            if (rc) return rc;
        }
    }
    if ((rc = run_tail(c, outFixed, outFloat))) return rc;
    return rec_.finish();
}

int check_shape(int H, int W, int64_t stride) {
    if (H <= 0 || W <= 0) return fail(DSX_EINVAL, "image must be non-empty");
    if (stride < W) return fail(DSX_EINVAL, "stride_bytes must be >= W");
    if ((int64_t)H * W > (int64_t)1 << 31) return fail(DSX_EINVAL, "image too large");
    return DSX_OK;
}

// dsx_compute_device, dsx_compute_conf_device (CALL_COMPUTE, one frame) and dsx_compute_batch_device (CALL_BATCH)
int compute_device(dsx_handle *h, int kind, int nframes, const void *dL, const void *dR, int64_t frame_stride, int H,
                   int W, int64_t stride, void *out_fixed, void *out_float, void *out_conf, void *hip_stream) {
    g_err.clear();
    if (!h) return fail(DSX_EINVAL, "handle is NULL");
    if (!dL || !dR) return fail(DSX_EINVAL, "input pointers are NULL");
    if (!out_fixed && !out_float && !out_conf) return fail(DSX_EINVAL, "at least one output is required");
    if (nframes < 1) return fail(DSX_EINVAL, "nframes must be >= 1");
    int rc = check_shape(H, W, stride);
    if (rc) return rc;
    if (nframes > 1 && frame_stride < (int64_t)(H - 1) * stride + W)
        return fail(DSX_EINVAL, "frame_stride_bytes smaller than one frame");
    if (kind == dsx::CALL_BATCH && (int64_t)nframes * H * W > ((int64_t)1 << 31) - 1)
        return fail(DSX_EINVAL, "nframes * H * W must stay below 2^31 pixels per launch");
    dsx::CallPlan pl;
    if ((rc = begin_call(h, kind, out_conf != nullptr, nframes, H, W, pl))) return rc;
    return run(h, pl, dL, dR, H, W, stride, out_fixed, out_float, static_cast<hipStream_t>(hip_stream), frame_stride,
               false, out_conf);
}

// dsx_compute_host / dsx_compute_conf_host (out_fixed may be NULL only with out_conf)
int compute_host(dsx_handle *h, const uint8_t *L, const uint8_t *R, int H, int W, int64_t stride_bytes,
                 int16_t *out_fixed, float *out_float, uint8_t *out_conf) {
    g_err.clear();
    if (!h) return fail(DSX_EINVAL, "handle is NULL");
    if (!L || !R || (!out_fixed && !out_conf))
        return fail(DSX_EINVAL, out_conf ? "input pointers are NULL" : "NULL argument (out_fixed is required)");
    int rc = check_shape(H, W, stride_bytes);
    if (rc) return rc;
    dsx::CallPlan pl;
    if ((rc = begin_call(h, dsx::CALL_COMPUTE, out_conf != nullptr, 1, H, W, pl))) return rc;
    const size_t n = (size_t)H * W;
    if ((rc = h->stageL.grow(n)) || (rc = h->stageR.grow(n)) || (rc = h->stageFixed.grow(n * 2)) ||
        (rc = h->stageFloat.grow(n * 4)) || (out_conf && (rc = h->dConf.grow(n))))
        return rc;
    hipStream_t st = h->stream;
    DSX_HIP(hipMemcpy2DAsync(h->stageL.ptr, W, L, stride_bytes, W, H, hipMemcpyHostToDevice, st));
    DSX_HIP(hipMemcpy2DAsync(h->stageR.ptr, W, R, stride_bytes, W, H, hipMemcpyHostToDevice, st));
    rc = run(h, pl, h->stageL.ptr, h->stageR.ptr, H, W, W, h->stageFixed.ptr, out_float ? h->stageFloat.ptr : nullptr,
             st, 0, false, out_conf ? h->dConf.ptr : nullptr);
    if (rc) return rc;
    if (out_fixed) DSX_HIP(hipMemcpyAsync(out_fixed, h->stageFixed.ptr, n * 2, hipMemcpyDeviceToHost, st));
    if (out_float) DSX_HIP(hipMemcpyAsync(out_float, h->stageFloat.ptr, n * 4, hipMemcpyDeviceToHost, st));
    if (out_conf) DSX_HIP(hipMemcpyAsync(out_conf, h->dConf.ptr, n, hipMemcpyDeviceToHost, st));
    DSX_HIP(hipStreamSynchronize(st));
    return DSX_OK;
}

// the C-ABI's step count (0 adaptive, > 0 that many, < 0 none) as InpaintOpts.steps
int fill_steps(int32_t steps) { return steps == 0 ? -1 : std::max(0, (int)steps); }

// The shape, the outputs and the depth conversion (PostArgs and PostFullArgs name them alike); depth only
// when has_depth.
template <class A>
void post_args(A &a, const dsx_post_params &pp, int64_t in_pitch, int H, int W, int crop, void *d_out_disp,
               void *d_out_depth) {
    a.in_pitch = in_pitch;
    a.H = H;
    a.W = W;
    a.crop = crop;
    a.out_disp = static_cast<float *>(d_out_disp);
    a.out_depth = pp.has_depth ? static_cast<float *>(d_out_depth) : nullptr;
    a.fB = (float)(pp.focal_length * pp.baseline);
    a.doffs = (float)pp.doffs;
    a.eps = (float)pp.eps;
    a.max_depth = (float)pp.max_depth;
    a.has_max = pp.has_max_depth ? 1 : 0;
}

// the full chain's filters and hole filling on top; the input and the status key are the caller's
void post_full_args(dsx::PostFullArgs &a, const dsx_post_params &pp, int64_t in_pitch, int H, int W, int crop,
                    void *d_out_disp, void *d_out_depth) {
    post_args(a, pp, in_pitch, H, W, crop, d_out_disp, d_out_depth);
    a.max_speckle = pp.max_speckle_size;
    a.max_diff16 = (int)(pp.max_diff * 16);  // int(max_diff * 16), postprocess.py:30
    a.apply_outliers = pp.apply_outlier_removal ? 1 : 0;
    a.kernel = pp.outlier_kernel;
    a.thr = (float)pp.outlier_threshold;
    a.fill_radius = pp.fill_radius;
    a.fill_method = pp.fill_method;
    a.fill_opts.spin_limit = pp.fill_spin_limit;
    a.fill_opts.steps = fill_steps(pp.fill_steps);
}

}  // namespace

namespace dsx {
// shared with dsx_comm.hip: one thread-local message behind dsx_last_error()
int set_error(int code, const std::string &msg) { return fail(code, msg); }
}  // namespace dsx

static_assert(dsx::kFillInpaint == DSX_FILL_INPAINT && dsx::kFillNearest == DSX_FILL_NEAREST, "fill methods");
static_assert(dsx::kCensus9x7 == DSX_COST_CENSUS9X7 && dsx::kCensus5x5 == DSX_COST_CENSUS5X5, "census windows");
static_assert(dsx::kPrefNone == DSX_PREFILTER_NONE && dsx::kPrefXsobel == DSX_PREFILTER_XSOBEL &&
                  dsx::kPrefMean == DSX_PREFILTER_MEAN, "prefilter types");
static_assert(dsx::kNearestFused == DSX_NEAREST_FUSED && dsx::kNearestStep == DSX_NEAREST_STEPWISE &&
                  dsx::kNearestFusedMaxK == DSX_NEAREST_FUSED_MAX, "nearest paths");

extern "C" {

int dsx_version(void) { return DSX_VERSION; }

int dsx_device_count(int *n) {
    if (!n) return fail(DSX_EINVAL, "n is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        if (e == hipErrorNoDevice) return DSX_OK;
        return fail(DSX_EHIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *n = c;
    return DSX_OK;
}

void dsx_default_params(dsx_params *p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->min_disp = 0;
    p->num_disp = 128;
    p->block_size = 5;
    p->cost = DSX_COST_SAD;
    p->uniqueness_ratio = 10;
    p->disp12_max_diff = 1;
    p->subpixel = 1;
    p->float_mode = DSX_FLOAT_FIXED;
    p->path = DSX_PATH_FUSED;
    p->timing = 0;
    p->prefilter_cap = 31;
    p->sgbm_post = 0;
    p->speckle_window_size = 50;
    p->speckle_range = 2;
}

int dsx_check_params(const dsx_params *p) {
    g_err.clear();
    return check(p);
}

int dsx_create(int device, const dsx_params *p, dsx_handle **out) {
    g_err.clear();
    if (!out) return fail(DSX_EINVAL, "out is NULL");
    *out = nullptr;
    int rc = check(p);
    if (rc) return rc;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(DSX_EHIP, "no HIP device available");
    if (device < 0 || device >= n) return fail(DSX_EINVAL, "device index out of range");
    DSX_HIP(hipSetDevice(device));
    dsx_handle *h = new dsx_handle();
    h->device = device;
    h->p = *p;
    dsx_default_confidence(&h->cf);
    pick_geometry(*p, h->g);
    dsx::pick_volume_geometry(*p, h->gv);
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete h;
        return fail(DSX_EHIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    *out = h;
    return DSX_OK;
}

int dsx_set_params(dsx_handle *h, const dsx_params *p) {
    g_err.clear();
    int rc = check(p);  // first: a rejected set reports its own cause, whatever the handle
    if (rc) return rc;
    if (!h) return fail(DSX_EINVAL, "handle is NULL");
    if (h->pf.type != DSX_PREFILTER_NONE && p->cost == DSX_COST_BT)
        return fail(DSX_EINVAL, "the handle has a prefilter set (dsx_set_prefilter): cost BT filters for itself; "
                                "switch the prefilter off first");
    if ((h->pf.type != DSX_PREFILTER_NONE || h->pf.texture_threshold > 0) && is_census(p->cost))
        return fail(DSX_EINVAL, "the handle has a prefilter set (dsx_set_prefilter): census ranks intensities "
                                "itself; switch the prefilter off first");
    DSX_HIP(hipSetDevice(h->device));
    DSX_HIP(hipStreamSynchronize(h->stream));
    h->p = *p;
    pick_geometry(*p, h->g);
    dsx::pick_volume_geometry(*p, h->gv);
    return DSX_OK;
}

void dsx_default_prefilter(dsx_prefilter *f) {
    if (!f) return;
    std::memset(f, 0, sizeof(*f));
    f->type = DSX_PREFILTER_NONE;
    f->size = 9;
    f->cap = 31;
    f->texture_threshold = 0;
}

int dsx_check_prefilter(const dsx_params *p, const dsx_prefilter *f) {
    g_err.clear();
    return check_prefilter(p, f);
}

int dsx_set_prefilter(dsx_handle *h, const dsx_prefilter *f) {
    g_err.clear();
    if (!h) return fail(DSX_EINVAL, "handle is NULL");
    dsx_prefilter off;
    dsx_default_prefilter(&off);
    if (!f) f = &off;
    int rc = check_prefilter(&h->p, f);
    if (rc) return rc;
    DSX_HIP(hipSetDevice(h->device));
    DSX_HIP(hipStreamSynchronize(h->stream));
    h->pf = *f;
    return DSX_OK;
}

int dsx_prefilter_device(const void *d_img, int32_t H, int32_t W, int64_t stride_bytes, const dsx_prefilter *f,
                         void *d_out, int64_t out_stride_bytes, void *hip_stream) {
    g_err.clear();
    if (!d_img || !d_out) return fail(DSX_EINVAL, "NULL image or output");
    if (d_img == d_out) return fail(DSX_EINVAL, "d_out must not be d_img (every output reads its neighbours)");
    int rc = check_prefilter(nullptr, f);
    if (rc) return rc;
    if (f->type == DSX_PREFILTER_NONE) return fail(DSX_EINVAL, "prefilter type NONE: nothing to run");
    if ((rc = check_shape(H, W, stride_bytes))) return rc;
    if (out_stride_bytes < W) return fail(DSX_EINVAL, "out_stride_bytes must be >= W");
    dsx::PrefilterArgs a{};
    a.src[0] = static_cast<const uint8_t *>(d_img);
    a.stride = stride_bytes;
    a.dst[0] = static_cast<uint8_t *>(d_out);
    a.dpitch = out_stride_bytes;
    a.dwidth = W;  // the caller's rows end at W
    a.nviews = 1;
    a.nframes = 1;
    a.H = H;
    a.W = W;
    a.type = f->type;
    a.n = f->size;
    a.cap = f->cap;
    DSX_HIP(dsx::launch_prefilter(a, static_cast<hipStream_t>(hip_stream)));
    return DSX_OK;
}

int dsx_texture_sum_device(const void *d_pref, int32_t H, int32_t W, int64_t stride_bytes, int32_t block_size,
                           int32_t cap, void *d_out_u16, void *hip_stream) {
    g_err.clear();
    if (!d_pref || !d_out_u16) return fail(DSX_EINVAL, "NULL image or output");
    int rc = check_block_size(block_size);
    if (rc) return rc;
    if (cap < 1 || cap > 63) return fail(DSX_EINVAL, "cap must be in [1, 63]");
    if ((rc = check_shape(H, W, stride_bytes))) return rc;
    dsx::TextureArgs t{};
    t.pref = static_cast<const uint8_t *>(d_pref);
    t.stride = stride_bytes;
    t.nframes = 1;
    t.H = H;
    t.W = W;
    t.block = block_size;
    t.cap = cap;
    t.out_sum = static_cast<uint16_t *>(d_out_u16);
    DSX_HIP(dsx::launch_texture(t, static_cast<hipStream_t>(hip_stream)));
    return DSX_OK;
}

int dsx_census_device(const void *d_img, int32_t H, int32_t W, int64_t stride_bytes, int32_t cost, void *d_out_u64,
                      void *hip_stream) {
    g_err.clear();
    if (!d_img || !d_out_u64) return fail(DSX_EINVAL, "NULL image or output");
    if (!is_census(cost)) return fail(DSX_EINVAL, "cost must be CENSUS9X7 (3) or CENSUS5X5 (4)");
    int rc = check_shape(H, W, stride_bytes);
    if (rc) return rc;
    dsx::CensusArgs c{};
    c.src[0] = static_cast<const uint8_t *>(d_img);
    c.stride = stride_bytes;
    c.dst[0] = d_out_u64;
    c.nviews = 1;
    c.H = H;
    c.W = W;
    c.window = cost;
    c.out64 = 1;
    DSX_HIP(dsx::launch_census_transform(c, static_cast<hipStream_t>(hip_stream)));
    return DSX_OK;
}

namespace {
__global__ __launch_bounds__(256) void block_min8_kernel(const uint4 *blocks, int64_t n, uint32_t *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = dsx::block_min8<true>(blocks[i]);
}
}  // namespace

int dsx_block_min8_device(const void *d_blocks, int64_t n, void *d_out_u32, void *hip_stream) {
    g_err.clear();
    if (!d_blocks || !d_out_u32) return fail(DSX_EINVAL, "NULL blocks or output");
    if (n < 1 || n > (int64_t)1 << 30) return fail(DSX_EINVAL, "n must be in [1, 2^30]");
    hipLaunchKernelGGL(block_min8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(hip_stream),
                       static_cast<const uint4 *>(d_blocks), n, static_cast<uint32_t *>(d_out_u32));
    DSX_HIP(hipGetLastError());
    return DSX_OK;
}

int dsx_compute_device(dsx_handle *h, const void *dL, const void *dR, int32_t H, int32_t W, int64_t stride_bytes,
                       void *d_out_fixed, void *d_out_float, void *hip_stream) {
    return compute_device(h, dsx::CALL_COMPUTE, 1, dL, dR, 0, H, W, stride_bytes, d_out_fixed, d_out_float, nullptr,
                          hip_stream);
}

void dsx_default_confidence(dsx_confidence *c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->type = DSX_CONF_PEAK_RATIO;
    c->threshold = 0;
}

int dsx_check_confidence(const dsx_params *p, const dsx_confidence *c) {
    g_err.clear();
    return check_confidence(p, c);
}

int dsx_set_confidence(dsx_handle *h, const dsx_confidence *c) {
    g_err.clear();
    if (!h) return fail(DSX_EINVAL, "handle is NULL");
    dsx_confidence off;
    dsx_default_confidence(&off);
    if (!c) c = &off;
    int rc = check_confidence(nullptr, c);
    if (rc) return rc;
    DSX_HIP(hipSetDevice(h->device));
    DSX_HIP(hipStreamSynchronize(h->stream));
    h->cf = *c;
    return DSX_OK;
}

int dsx_compute_conf_device(dsx_handle *h, const void *dL, const void *dR, int32_t H, int32_t W, int64_t stride_bytes,
                            void *d_out_fixed, void *d_out_float, void *d_out_conf, void *hip_stream) {
    return compute_device(h, dsx::CALL_COMPUTE, 1, dL, dR, 0, H, W, stride_bytes, d_out_fixed, d_out_float, d_out_conf,
                          hip_stream);
}

int dsx_postprocess_fast_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t crop,
                                void *d_out_disp, void *d_out_depth, double focal_length, double baseline,
                                double doffs, double eps, double max_depth, int32_t has_max_depth,
                                void *hip_stream) {
    g_err.clear();
    if (!d_disp) return fail(DSX_EINVAL, "d_disp is NULL");
    if (H <= 0 || W <= 0 || in_pitch < W) return fail(DSX_EINVAL, "bad shape / pitch");
    if (crop < 0) return fail(DSX_EINVAL, "crop must be >= 0");
    if (crop >= W || (!d_out_disp && !d_out_depth)) return DSX_OK;  // empty result, as disp[:, crop:] is
    dsx_post_params pp{};
    pp.focal_length = focal_length, pp.baseline = baseline, pp.doffs = doffs, pp.eps = eps, pp.max_depth = max_depth;
    pp.has_depth = 1, pp.has_max_depth = has_max_depth;
    dsx::PostArgs a{};
    a.disp = static_cast<const float *>(d_disp);
    post_args(a, pp, in_pitch, H, W, crop, d_out_disp, d_out_depth);
    DSX_HIP(dsx::launch_post_fast(a, static_cast<hipStream_t>(hip_stream)));
    return DSX_OK;
}

size_t dsx_postprocess_workspace_bytes(int32_t H, int32_t W, int32_t crop) {
    if (H <= 0 || W <= 0 || crop < 0) return 0;
    return dsx::post_full_workspace(H, W, crop);
}

int dsx_postprocess_full_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t crop,
                                int32_t max_speckle_size, double max_diff, int32_t apply_outlier_removal,
                                double outlier_threshold, int32_t outlier_kernel, void *d_out_disp,
                                void *d_out_depth, double focal_length, double baseline, double doffs, double eps,
                                double max_depth, int32_t has_max_depth, void *d_workspace,
                                size_t workspace_bytes, void *hip_stream) {
    return dsx_postprocess_full_ex_device(d_disp, H, W, in_pitch, crop, max_speckle_size, max_diff,
                                          apply_outlier_removal, outlier_threshold, outlier_kernel, 0, d_out_disp,
                                          d_out_depth, focal_length, baseline, doffs, eps, max_depth, has_max_depth,
                                          d_workspace, workspace_bytes, hip_stream);
}

namespace {
// fill_method / fill_radius of the full chain (post_full_standalone, dsx_process_pair_device)
int check_fill(int32_t fill_method, int32_t fill_radius) {
    if (fill_radius < 0) return fail(DSX_EINVAL, "fill_radius must be >= 0");
    if (fill_method != DSX_FILL_INPAINT && fill_method != DSX_FILL_NEAREST)
        return fail(DSX_EINVAL, "fill_method must be DSX_FILL_INPAINT or DSX_FILL_NEAREST");
    if (fill_method == DSX_FILL_NEAREST && fill_radius > dsx::kNearestMaxK)
        return fail(DSX_EINVAL, "fill_method 'nearest': kernel_size (fill_radius) must be in [0, 31]");
    return DSX_OK;
}

int check_refine(const dsx_refine *rf) {
    if (!rf) return fail(DSX_EINVAL, "NULL refine");
    if (rf->type == DSX_REFINE_NONE) return DSX_OK;
    if (rf->type != DSX_REFINE_WMEDIAN) return fail(DSX_EINVAL, "refine type must be DSX_REFINE_NONE or DSX_REFINE_WMEDIAN");
    if (rf->radius < dsx::kWmedianMinRadius || rf->radius > dsx::kWmedianMaxRadius)
        return fail(DSX_EINVAL, "refine radius must be in [1, 7]");
    if (rf->sigma < dsx::kWmedianMinSigma || rf->sigma > dsx::kWmedianMaxSigma)
        return fail(DSX_EINVAL, "refine sigma must be in [1, 64]");
    if (rf->fill != 0 && rf->fill != 1) return fail(DSX_EINVAL, "refine fill must be 0 or 1");
    return DSX_OK;
}

// the chain's refinement hop from the C-ABI's arguments (rf NULL or type NONE: off, the guide unused)
int refine_args(const dsx_refine *rf, const void *d_guide, int64_t guide_stride_bytes, int32_t W, dsx::RefineArgs &ra) {
    ra = dsx::RefineArgs{};
    if (!rf || rf->type == DSX_REFINE_NONE) return DSX_OK;
    if (int rc = check_refine(rf)) return rc;
    if (!d_guide) return fail(DSX_EINVAL, "refine needs a guide image (d_guide is NULL)");
    if (guide_stride_bytes < W) return fail(DSX_EINVAL, "guide_stride_bytes must be >= W");
    ra.type = dsx::kRefineWmedian;
    ra.radius = rf->radius;
    ra.sigma = rf->sigma;
    ra.fill = rf->fill;
    ra.guide = static_cast<const uint8_t *>(d_guide);
    ra.guide_stride = guide_stride_bytes;
    return DSX_OK;
}

// the stand-alone chain behind dsx_postprocess_full_ex_device and dsx_postprocess_device
int post_full_standalone(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t crop,
                         const dsx_post_params &pp, void *d_out_disp, void *d_out_depth, void *d_workspace,
                         size_t workspace_bytes, void *hip_stream, const dsx_refine *rf = nullptr,
                         const void *d_guide = nullptr, int64_t guide_stride_bytes = 0) {
    if (int rc = check_fill(pp.fill_method, pp.fill_radius)) return rc;
    if (!d_disp) return fail(DSX_EINVAL, "d_disp is NULL");
    if (H <= 0 || W <= 0 || in_pitch < W || crop < 0) return fail(DSX_EINVAL, "bad shape / pitch / crop");
    if (pp.outlier_kernel < 1 || (pp.outlier_kernel & 1) == 0) return fail(DSX_EINVAL, "outlier_kernel must be odd");
    dsx::RefineArgs ra{};
    if (int rc = refine_args(rf, d_guide, guide_stride_bytes, W, ra)) return rc;
    if (crop >= W || (!d_out_disp && !(pp.has_depth && d_out_depth))) return DSX_OK;
    if (!d_workspace || workspace_bytes < dsx::post_full_workspace(H, W, crop))
        return fail(DSX_EINVAL, "workspace too small (dsx_postprocess_workspace_bytes)");
    if ((int64_t)H * (W - crop) > 0x7FFFFFFF) return fail(DSX_EINVAL, "image too large for int32 labels");
    if (pp.fill_radius > 0 && pp.fill_method == DSX_FILL_INPAINT) {
        int rc = check_fill_shape(H, W - crop);
        if (!rc) rc = sticky_inpaint_timeout(d_workspace);
        if (rc) return rc;
    }
    dsx::PostFullArgs a{};
    a.disp = static_cast<const float *>(d_disp);
    post_full_args(a, pp, in_pitch, H, W, crop, d_out_disp, d_out_depth);
    DSX_HIP(dsx::launch_post_full(a, d_workspace, static_cast<hipStream_t>(hip_stream), nullptr, &ra));
    return DSX_OK;
}
}  // namespace

int dsx_postprocess_full_ex_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t crop,
                                   int32_t max_speckle_size, double max_diff, int32_t apply_outlier_removal,
                                   double outlier_threshold, int32_t outlier_kernel, int32_t fill_radius,
                                   void *d_out_disp, void *d_out_depth, double focal_length, double baseline,
                                   double doffs, double eps, double max_depth, int32_t has_max_depth,
                                   void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    g_err.clear();
    // in declaration order; has_depth 1, and the rest 0: Telea's march with its default launch options
    const dsx_post_params pp{max_diff, outlier_threshold, focal_length, baseline, doffs, eps, max_depth, DSX_POST_FULL,
                             max_speckle_size, apply_outlier_removal, outlier_kernel, fill_radius, 1, has_max_depth};
    return post_full_standalone(d_disp, H, W, in_pitch, crop, pp, d_out_disp, d_out_depth, d_workspace, workspace_bytes,
                                hip_stream);
}

int dsx_postprocess_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t crop,
                           const dsx_post_params *pp, void *d_out_disp, void *d_out_depth, void *d_workspace,
                           size_t workspace_bytes, void *hip_stream) {
    return dsx_postprocess_refine_device(d_disp, H, W, in_pitch, crop, pp, d_out_disp, d_out_depth, d_workspace,
                                         workspace_bytes, hip_stream, nullptr, nullptr, 0);
}

int dsx_postprocess_refine_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t crop,
                                  const dsx_post_params *pp, void *d_out_disp, void *d_out_depth, void *d_workspace,
                                  size_t workspace_bytes, void *hip_stream, const dsx_refine *rf, const void *d_guide,
                                  int64_t guide_stride_bytes) {
    g_err.clear();
    if (!pp) return fail(DSX_EINVAL, "NULL post parameters");
    if (pp->mode != DSX_POST_FULL) return fail(DSX_EINVAL, "dsx_postprocess_device runs mode DSX_POST_FULL");
    return post_full_standalone(d_disp, H, W, in_pitch, crop, *pp, d_out_disp, d_out_depth, d_workspace,
                                workspace_bytes, hip_stream, rf, d_guide, guide_stride_bytes);
}

void dsx_default_refine(dsx_refine *rf) {
    if (!rf) return;
    std::memset(rf, 0, sizeof(*rf));
    rf->type = DSX_REFINE_NONE;
    rf->radius = 5;
    rf->sigma = 8;
    rf->fill = 1;
}

int dsx_check_refine(const dsx_refine *rf) {
    g_err.clear();
    return check_refine(rf);
}

int dsx_wmedian_weights(int32_t sigma, uint16_t *out256) {
    g_err.clear();
    if (sigma < dsx::kWmedianMinSigma || sigma > dsx::kWmedianMaxSigma) return fail(DSX_EINVAL, "sigma must be in [1, 64]");
    if (!out256) return fail(DSX_EINVAL, "out256 is NULL");
    return dsx::wmedian_weights(sigma, out256) == 0 ? DSX_OK : fail(DSX_EINVAL, "bad sigma");
}

int dsx_wmedian_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, const void *d_guide,
                       int64_t guide_stride_bytes, const dsx_refine *rf, void *d_out, void *hip_stream) {
    g_err.clear();
    if (!d_disp || !d_out) return fail(DSX_EINVAL, "NULL input or output");
    if (!d_guide) return fail(DSX_EINVAL, "d_guide is NULL");
    if (d_out == d_disp) return fail(DSX_EINVAL, "d_out must not be d_disp (every window reads its neighbours' inputs)");
    if (H <= 0 || W <= 0 || in_pitch < W || guide_stride_bytes < W) return fail(DSX_EINVAL, "bad shape / pitch / stride");
    if ((int64_t)H > 16 * 65535) return fail(DSX_EINVAL, "image too tall (H > 1048560)");
    if (int rc = check_refine(rf)) return rc;
    if (rf->type != DSX_REFINE_WMEDIAN) return fail(DSX_EINVAL, "dsx_wmedian_device runs type DSX_REFINE_WMEDIAN");
    DSX_HIP(dsx::launch_wmedian(static_cast<const float *>(d_disp), in_pitch, H, W, static_cast<const uint8_t *>(d_guide),
                                guide_stride_bytes, rf->radius, rf->sigma, rf->fill, static_cast<float *>(d_out),
                                static_cast<hipStream_t>(hip_stream)));
    return DSX_OK;
}

size_t dsx_fill_nearest_workspace_bytes(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return 0;
    return dsx::nearest_workspace(H, W);
}

int dsx_fill_nearest_footprint(int32_t kernel_size, int32_t *halfwidths, int32_t cap) {
    g_err.clear();
    if (kernel_size < 0 || kernel_size > dsx::kNearestMaxK) return fail(DSX_EINVAL, "kernel_size must be in [0, 31]");
    if (!halfwidths || cap < 2 * (kernel_size / 2) + 1)
        return fail(DSX_EINVAL, "halfwidths needs 2 * (kernel_size / 2) + 1 entries");
    return dsx::nearest_footprint(kernel_size, halfwidths, cap);
}

int dsx_fill_nearest_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t kernel_size,
                            void *d_out, void *d_workspace, size_t workspace_bytes, int32_t path, void *hip_stream) {
    g_err.clear();
    if (!d_disp || !d_out) return fail(DSX_EINVAL, "NULL input or output");
    if (d_out == d_disp) return fail(DSX_EINVAL, "d_out must not be d_disp (every iteration reads the previous one)");
    if (H <= 0 || W <= 0 || in_pitch < W) return fail(DSX_EINVAL, "bad shape / pitch");
    if (kernel_size < 0 || kernel_size > dsx::kNearestMaxK) return fail(DSX_EINVAL, "kernel_size must be in [0, 31]");
    if (path != DSX_NEAREST_AUTO && path != DSX_NEAREST_FUSED && path != DSX_NEAREST_STEPWISE)
        return fail(DSX_EINVAL, "path must be DSX_NEAREST_AUTO, DSX_NEAREST_FUSED or DSX_NEAREST_STEPWISE");
    if (path == DSX_NEAREST_FUSED && kernel_size > DSX_NEAREST_FUSED_MAX)
        return fail(DSX_EINVAL, "the fused path covers kernel_size <= DSX_NEAREST_FUSED_MAX");
    if ((int64_t)H > 4 * 65535) return fail(DSX_EINVAL, "image too tall (H > 262140)");
    if (path == DSX_NEAREST_AUTO) path = kernel_size <= DSX_NEAREST_FUSED_MAX ? DSX_NEAREST_FUSED : DSX_NEAREST_STEPWISE;
    if (path == DSX_NEAREST_STEPWISE && kernel_size >= 2 &&
        (!d_workspace || workspace_bytes < dsx::nearest_workspace(H, W)))
        return fail(DSX_EINVAL, "workspace too small (dsx_fill_nearest_workspace_bytes)");
    DSX_HIP(dsx::launch_nearest(static_cast<const float *>(d_disp), in_pitch, H, W, kernel_size,
                                static_cast<float *>(d_out), static_cast<float *>(d_workspace),
                                path == DSX_NEAREST_FUSED ? dsx::kNearestFused : dsx::kNearestStep,
                                static_cast<hipStream_t>(hip_stream)));
    return DSX_OK;
}

size_t dsx_fill_holes_workspace_bytes(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return 0;
    return dsx::inpaint_workspace(H, W);
}

int dsx_fill_holes_ex_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t radius, void *d_out,
                             void *d_workspace, size_t workspace_bytes, const dsx_fill_opts *opts, void *hip_stream) {
    g_err.clear();
    if (!d_disp || !d_out) return fail(DSX_EINVAL, "NULL input or output");
    if (H <= 0 || W <= 0 || in_pitch < W) return fail(DSX_EINVAL, "bad shape / pitch");
    if (radius < 0) return fail(DSX_EINVAL, "radius must be >= 0");
    int rc = check_fill_shape(H, W);
    if (rc) return rc;
    if (!d_workspace || workspace_bytes < dsx::inpaint_workspace(H, W))
        return fail(DSX_EINVAL, "workspace too small (dsx_fill_holes_workspace_bytes)");
    rc = sticky_inpaint_timeout(d_workspace);
    if (rc) return rc;
    dsx::InpaintOpts o;
    if (opts) {
        o.spin_limit = opts->spin_limit;
        o.steps = fill_steps(opts->steps);
    }
    DSX_HIP(dsx::launch_inpaint(static_cast<const float *>(d_disp), in_pitch, H, W, radius, static_cast<float *>(d_out),
                                d_workspace, static_cast<hipStream_t>(hip_stream), o));
    return DSX_OK;
}

int dsx_fill_holes_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t radius, void *d_out,
                          void *d_workspace, size_t workspace_bytes, void *hip_stream) {
    return dsx_fill_holes_ex_device(d_disp, H, W, in_pitch, radius, d_out, d_workspace, workspace_bytes, nullptr,
                                    hip_stream);
}

int dsx_rectify_device(const void *d_img, int32_t Hs, int32_t Ws, int64_t stride_bytes, int32_t channels,
                       const float *d_mapx, const float *d_mapy, int32_t H, int32_t W, void *d_out,
                       void *hip_stream) {
    g_err.clear();
    if (!d_img || !d_out) return fail(DSX_EINVAL, "NULL image or output");
    if (channels != 1 && channels != 3) return fail(DSX_EINVAL, "channels must be 1 or 3");
    if (Hs <= 0 || Ws <= 0 || stride_bytes < (int64_t)Ws * channels) return fail(DSX_EINVAL, "bad source shape");
    if ((d_mapx == nullptr) != (d_mapy == nullptr)) return fail(DSX_EINVAL, "give both maps or neither");
    if (!d_mapx && (H != Hs || W != Ws || channels != 3))
        return fail(DSX_EINVAL, "gray conversion alone needs a 3-channel image and H, W = Hs, Ws");
    if (H <= 0 || W <= 0) return fail(DSX_EINVAL, "bad output shape");
    dsx::RectArgs a{};
    a.img = static_cast<const uint8_t *>(d_img);
    a.stride = stride_bytes;
    a.Hs = Hs;
    a.Ws = Ws;
    a.mapx = d_mapx;
    a.mapy = d_mapy;
    a.H = H;
    a.W = W;
    a.out = static_cast<uint8_t *>(d_out);
    DSX_HIP(dsx::launch_rectify(a, channels, static_cast<hipStream_t>(hip_stream)));
    return DSX_OK;
}

int dsx_resize_area_table(int32_t in_size, int32_t out_size, int32_t *start, int32_t *count, int32_t *coef) {
    g_err.clear();
    if (!start || !count || !coef) return fail(DSX_EINVAL, "NULL table array");
    if (out_size < 1 || out_size > in_size) return fail(DSX_EINVAL, "out_size must be in [1, in_size]");
    if (dsx::resize_area_table(in_size, out_size, start, count, coef) != 0) return fail(DSX_EINVAL, "bad sizes");
    return DSX_OK;
}

int dsx_resize_area_device(const void *d_img, int32_t Hs, int32_t Ws, int64_t stride_bytes, int32_t channels,
                           int32_t Ho, int32_t Wo, int32_t gray_out, void *d_out, int64_t out_stride_bytes,
                           void *hip_stream) {
    g_err.clear();
    if (!d_img || !d_out) return fail(DSX_EINVAL, "NULL image or output");
    if (channels != 1 && channels != 3) return fail(DSX_EINVAL, "channels must be 1 or 3");
    if (gray_out != 0 && gray_out != 1) return fail(DSX_EINVAL, "gray_out must be 0 or 1");
    if (gray_out && channels != 3) return fail(DSX_EINVAL, "gray_out needs a 3-channel image");
    if (Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1) return fail(DSX_EINVAL, "sizes must be >= 1");
    if (Ho > Hs || Wo > Ws) return fail(DSX_EINVAL, "the output must not be larger than the source (no upscaling)");
    if (stride_bytes < (int64_t)Ws * channels) return fail(DSX_EINVAL, "stride_bytes must be >= Ws * channels");
    if (out_stride_bytes < (int64_t)Wo * (gray_out ? 1 : channels))
        return fail(DSX_EINVAL, "out_stride_bytes must be >= the output row");
    if ((int64_t)Ws * channels > 0x7FFFFFFF || Ho > 4 * 65535) return fail(DSX_EINVAL, "image too large");
    // the tables live on the image's device
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, d_img) == hipSuccess) DSX_HIP(hipSetDevice(attr.device));
    else (void)hipGetLastError();
    DSX_HIP(dsx::launch_resize_area(static_cast<const uint8_t *>(d_img), stride_bytes, Hs, Ws, channels, Ho, Wo,
                                    gray_out != 0, static_cast<uint8_t *>(d_out), out_stride_bytes,
                                    static_cast<hipStream_t>(hip_stream)));
    return DSX_OK;
}

int dsx_compute_batch_device(dsx_handle *h, int32_t nframes, const void *dL, const void *dR, int64_t frame_stride_bytes,
                             int32_t H, int32_t W, int64_t stride_bytes, void *d_out_fixed, void *d_out_float,
                             void *hip_stream) {
    return compute_device(h, dsx::CALL_BATCH, nframes, dL, dR, frame_stride_bytes, H, W, stride_bytes, d_out_fixed,
                          d_out_float, nullptr, hip_stream);
}

int dsx_right_map_device(dsx_handle *h, const void *dL, const void *dR, int32_t H, int32_t W, int64_t stride_bytes,
                         void *d_out_dR, void *hip_stream) {
    g_err.clear();
    if (!h || !dL || !dR || !d_out_dR) return fail(DSX_EINVAL, "NULL argument");
    int rc = check_shape(H, W, stride_bytes);
    if (rc) return rc;
    dsx::CallPlan pl;
    if ((rc = begin_call(h, dsx::CALL_RIGHT_MAP, false, 1, H, W, pl))) return rc;
    return run_right_pass(h, pl, dL, dR, H, W, stride_bytes, static_cast<int16_t *>(d_out_dR),
                          static_cast<hipStream_t>(hip_stream));
}

int dsx_compute_host(dsx_handle *h, const uint8_t *L, const uint8_t *R, int32_t H, int32_t W, int64_t stride_bytes,
                     int16_t *out_fixed, float *out_float) {
    return compute_host(h, L, R, H, W, stride_bytes, out_fixed, out_float, nullptr);
}

int dsx_compute_conf_host(dsx_handle *h, const uint8_t *L, const uint8_t *R, int32_t H, int32_t W, int64_t stride_bytes,
                          int16_t *out_fixed, float *out_float, uint8_t *out_conf) {
    return compute_host(h, L, R, H, W, stride_bytes, out_fixed, out_float, out_conf);
}

int dsx_fill_holes_status(void) {
    g_err.clear();
    return sticky_inpaint_timeout(nullptr);
}

int dsx_fill_holes_release(const void *d_workspace) {
    g_err.clear();
    if (!d_workspace) return fail(DSX_EINVAL, "dsx_fill_holes_release: null workspace");
    const int rc = sticky_inpaint_timeout(d_workspace);
    dsx::inpaint_forget(d_workspace);
    return rc;
}

int dsx_shutdown(void) {
    g_err.clear();
    if (!dsx::inpaint_has_words() && !dsx::resize_has_tables()) return DSX_OK;  // nothing kept: no HIP call (CPU-only hosts)
    // the device may still write a workspace's mapped words: drain every device first.  (Freeing
    // them matters at exit: left to the HIP runtime's own teardown, the pinned mapped words were
    // the difference between a clean exit and a SIGSEGV inside libhsa-runtime64 under rocprofv3,
    // tools/exit_probe.py, profiles/README.md.)
    int n = 0;
    if (hipGetDeviceCount(&n) == hipSuccess) {
        int prev = 0;
        (void)hipGetDevice(&prev);
        for (int d = 0; d < n; ++d)
            if (hipSetDevice(d) == hipSuccess) (void)hipDeviceSynchronize();
        (void)hipSetDevice(prev);
    }
    dsx::inpaint_forget_all();
    dsx::resize_forget_all();
    return DSX_OK;
}

int dsx_fill_holes_status_ws(const void *d_workspace) {
    g_err.clear();
    if (!d_workspace) return fail(DSX_EINVAL, "workspace is NULL");
    return sticky_inpaint_timeout(d_workspace);
}

int dsx_fill_holes_status_handle(dsx_handle *h) {
    g_err.clear();
    if (!h) return fail(DSX_EINVAL, "handle is NULL");
    return sticky_inpaint_timeout(h);
}

int dsx_process_pair_device(dsx_handle *h, const void *dL, const void *dR, int32_t H, int32_t W, int64_t stride_bytes,
                            const dsx_post_params *pp, void *d_out_disp, void *d_out_depth, void *hip_stream) {
    return dsx_process_pair_refine_device(h, dL, dR, H, W, stride_bytes, pp, d_out_disp, d_out_depth, hip_stream, nullptr);
}

int dsx_process_pair_refine_device(dsx_handle *h, const void *dL, const void *dR, int32_t H, int32_t W,
                                   int64_t stride_bytes, const dsx_post_params *pp, void *d_out_disp, void *d_out_depth,
                                   void *hip_stream, const dsx_refine *rf) {
    g_err.clear();
    if (!h || !pp) return fail(DSX_EINVAL, "NULL handle or post parameters");
    if (!dL || !dR) return fail(DSX_EINVAL, "input pointers are NULL");
    int rc = check_shape(H, W, stride_bytes);
    if (rc) return rc;
    if (pp->mode != DSX_POST_FAST && pp->mode != DSX_POST_FULL)
        return fail(DSX_EINVAL, "post mode must be DSX_POST_FAST or DSX_POST_FULL");
    if (pp->mode == DSX_POST_FULL) {
        if (pp->outlier_kernel < 1 || (pp->outlier_kernel & 1) == 0) return fail(DSX_EINVAL, "outlier_kernel must be odd");
        if ((rc = check_fill(pp->fill_method, pp->fill_radius))) return rc;
    }
    if (h->p.float_mode != DSX_FLOAT_FIXED)
        return fail(DSX_EINVAL, "process_pair needs float_mode DSX_FLOAT_FIXED (stereo_core.py:232: fixed / 16)");
    // the guide is the caller's raw left image (the chain reads it from column num_disp on), never the
    // prefiltered copy; fast mode runs no refinement
    dsx::RefineArgs ra{};
    if (pp->mode == DSX_POST_FULL && (rc = refine_args(rf, dL, stride_bytes, W, ra))) return rc;
    const int crop = std::max(0, h->p.num_disp);  // stereo_core.py:168 crops num_disp columns
    const int Wc = W - crop;
    if (Wc <= 0 || (!d_out_disp && !(pp->has_depth && d_out_depth))) return DSX_OK;  // disp[:, num_disp:] is empty
    if (pp->mode == DSX_POST_FULL && pp->fill_radius > 0 && pp->fill_method == DSX_FILL_INPAINT) {
        rc = check_fill_shape(H, Wc);
        if (!rc) rc = sticky_inpaint_timeout(h);
        if (rc) return rc;
    }
    const bool full = pp->mode == DSX_POST_FULL;
    dsx::CallPlan pl;
    if ((rc = begin_call(h, full ? dsx::CALL_PAIR_FULL : dsx::CALL_PAIR_FAST, false, 1, H, W, pl))) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    // the matcher's map and the workspace are handle scratch: order after the previous call's use
    if ((rc = wait_scratch(h, st))) return rc;
    ScratchRecord rec_(h, st, true);
    dsx::PostFullArgs a{};
    bool defer = false;
    if (full) {
        // full mode reads the x16 map itself (postprocess.py:27 computes int16(d * 16) of d = fixed / 16,
        // which is `fixed` again): 2 B per pixel written by the matcher and read by the speckle pass
        a.in16 = h->ppFixed.as<int16_t>();
        post_full_args(a, *pp, W, H, W, crop, d_out_disp, d_out_depth);
        a.fill_opts.status_key = h;  // the handle's own timeout flag and step history
        // the fused pass's LR check moves into the speckle pass's loads (no lr_fixup launch) when the plan
        // allows it (a fused matcher with a check, no mask) and that pass is the two-launch form
        defer = pl.defer_lr_ok && dsx::post_full_two_launch(a) && getenv("DSX_NO_DEFER_LR") == nullptr;
    }
    rc = run(h, pl, dL, dR, H, W, stride_bytes, full ? h->ppFixed.ptr : nullptr, full ? nullptr : h->ppDisp.ptr, st, 0,
             defer);
    if (rc) return rc;
    rec_.active = true;  // run() recorded its own event; this call's kernels continue below
    if (full) {
        if (defer) {
            a.lr_keys = h->lastKeys;
            a.lr_dstar = h->lastDstar;
            a.lr_form = h->p.lr_form == DSX_LR_FORM_SGBM ? 1 : 0;
            a.lr_m = h->p.min_disp;
            a.lr_max = h->p.disp12_max_diff;
            a.lr_kshift = h->lastKshift;
        }
        TimingHook hook(h);
        hipError_t e = dsx::launch_post_full(a, h->ppWs.ptr, st, h->p.timing ? &hook : nullptr, &ra);
        if (e != hipSuccess) return fail(DSX_EHIP, std::string("post-processing launch: ") + hipGetErrorString(e));
        if (hook.rc) return hook.rc;
    } else {
        dsx::PostArgs f{};
        f.disp = h->ppDisp.as<float>();
        post_args(f, *pp, W, H, W, crop, d_out_disp, d_out_depth);
        DSX_LAUNCH(h, "median_depth", st, dsx::launch_post_fast(f, st));
    }
    return rec_.finish();
}

int dsx_kernel_times(dsx_handle *h, char *names, int names_cap, float *ms, int *counts, int cap, int *n) {
    g_err.clear();
    if (!h || !n) return fail(DSX_EINVAL, "NULL argument");
    DSX_HIP(hipSetDevice(h->device));
    int rc = collect_times(h);
    if (rc) return rc;
    std::string all;
    const int k = (int)h->knames.size();
    for (int i = 0; i < k; ++i) {
        if (i) all += ";";
        all += h->knames[i];
        if (i < cap) {
            if (ms) ms[i] = h->kcount[i] ? (float)(h->ktotal[i] / h->kcount[i]) : 0.f;
            if (counts) counts[i] = h->kcount[i];
        }
    }
    if (names && names_cap > 0) {
        std::strncpy(names, all.c_str(), (size_t)names_cap - 1);
        names[names_cap - 1] = '\0';
    }
    *n = k;
    return DSX_OK;
}

int dsx_reset_times(dsx_handle *h) {
    g_err.clear();
    if (!h) return fail(DSX_EINVAL, "handle is NULL");
    int rc = collect_times(h);
    if (rc) return rc;
    for (size_t i = 0; i < h->ktotal.size(); ++i) {
        h->ktotal[i] = 0.0;
        h->kcount[i] = 0;
    }
    return DSX_OK;
}

int dsx_workspace_bytes(dsx_handle *h, int64_t *bytes) {
    g_err.clear();
    if (!h || !bytes) return fail(DSX_EINVAL, "NULL argument");
    size_t sum = 0;
    for_each_buf(h, [&sum](const DevBuf &b) { sum += b.held; });
    *bytes = (int64_t)sum;
    return DSX_OK;
}

int dsx_destroy(dsx_handle *h) {
    g_err.clear();
    if (!h) return DSX_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    collect_times(h);
    dsx::inpaint_forget(h);
    for (auto &e : h->free_events) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    free_buffers(h);
    if (h->scratchDone) (void)hipEventDestroy(h->scratchDone);
    (void)hipStreamDestroy(h->stream);
    delete h;
    return DSX_OK;
}

const char *dsx_last_error(void) { return g_err.c_str(); }

}  // extern "C"
