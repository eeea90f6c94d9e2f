// Internal declarations shared by dsx_kernels.hip and dsx_api.cpp. Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsx_plan.h"  // Geometry and the BM_* cost layouts

namespace dsx {

enum Side : int { SIDE_LEFT = 0, SIDE_RIGHT = 1, SIDE_VOLUME = 2, SIDE_LEFT_LR = 3 };

constexpr int kVolThreads = 256;    // K2 (volume WTA) block size

// DSX_ROWSTEP_BLOCKMIN (=1 by default; =0 restores the previous form): the rotated row loop of bm2<R, SAD, 1, 0>,
// R <= 5, takes a tile block's minimum with v_pk_minimum3_f16 (block_min8 below; dsx_bm.hip).
// Declared here because the host's padding value goes with it: those costs are compared as f16 bit patterns, so the
// padding is the largest finite one instead of 0xFFFF (a NaN pattern).
#ifndef DSX_ROWSTEP_BLOCKMIN
#define DSX_ROWSTEP_BLOCKMIN 1
#endif
constexpr bool kRowstepBlockmin = DSX_ROWSTEP_BLOCKMIN;
constexpr uint32_t kBlockminPad = 0x7BFFu;  // 31,743 > 255 * 11 * 11 = 30,855, the largest cost of those kernels
// a launch of one of those kernels (side and sg_keys as launch_bm2_one reads them)
constexpr bool bm2_blockmin(int radius, int kind, int nw, int side, bool sg_keys) {
    return kRowstepBlockmin && kind == BM_SAD && nw == 1 && side == SIDE_LEFT && !sg_keys && radius <= 5;
}

// Arguments of the fused pass kernel bm2 (dsx_bm.hip).
struct Bm2Args {
    const uint8_t *ref;  // reference image (L for left/volume passes, R for the right pass)
    const uint8_t *src;  // searched image
    int64_t stride;      // row stride of both images in bytes
    int nframes;         // frames in this launch (>= 1); frame f's inputs start f * frame_stride bytes
    int64_t frame_stride;  // in, its outputs / LR buffers f * H * W elements in
    int H, W;
    int m;               // min_disp
    int D;               // num_disp (padded internally to the kernel's Dp)
    int side;            // 0 left (full epilogue; with sg_keys the launcher runs the side-4 build), 1 right (dR map), 2 volume (K1 store), 3 left + LR keys
    int uniq, lr, subpix, float_mode;
    uint32_t padv;       // cost stored for disparities outside [0, D) / outside the image
    int strip_begin, strip_count;  // 32-column strips forming the work space
    int grid_override;   // >0: force the persistent grid size (tests)
    int prio;            // 1: waves raise their issue priority while behind (progress bands below)
    int pt1, pt2, pt3;   // progress band edges in 1/256 of a block's rows (priority 3, 2, 1, 0)
    int variant;         // experiment bits (DSX_VARIANT env), 0 = production
    int slow_w8;         // work weight of a strip on the clamped-load path, in 1/8 of a fast strip
    int agew[4];         // work weight (1/64) of a block by co-residency age level (dispatch order)
    int nlev;            // age levels (co-resident waves per SIMD, <= 4); <= 1: equal weights
    const int *part;     // device: block b owns linear (frame, strip, row) units [part[b], part[b+1])
    uint32_t *lr_keys;     // left pass with LR: per-pixel right-view winner keys (C << kshift | d),
    int kshift;            //   filled by atomicMin (memset to ~0 first)
    int16_t *dstar;        // left pass with LR: winning d (or -1) for lr_fixup; with sg_keys: the x16 output
    uint32_t *sg_keys;     // left pass (side 0), OpenCV's LR form: per right pixel the min key
                           //   (cost << kshift | (kmask - d)) over the unique left winners mapping to it
    uint32_t *lr_reset;    // left pass with LR: the other key half, reset to ~0 here for the next call
    int64_t lr_reset_n;    //   (keys the previous call's lr_fixup consumed)
    int16_t *out_fixed;    // left pass outputs (either may be null)
    float *out_float;
    int16_t *out_dR;       // right pass output
    void *vol;             // side 2 output [H][W][Dp]
    uint64_t *timeline;    // debug (DSX_TIMELINE env): per block {start, end, hw_id, xcc_id}
    int in_flight;         // host only: the handle's launches overlap others on the device (launch_bm2_side's grid)
};

struct VolArgs {
    const void *vol;  // [H][W][Dp] u16 (SAD) or u32 (SSD); with nsum > 0: nsum u16 volumes summed
    int nsum;         // > 0: vol = nsum u16 volumes `sstride` elements apart (SGM L_r per direction)
    size_t sstride;
    int H, W, m, D, Dp, DB, TPP;
    int uniq, lr, subpix, float_mode;
    int lr_form;      // DSX_LR_FORM_BM: right-view argmin over every cost; DSX_LR_FORM_SGBM: OpenCV's form
    int16_t *out_fixed;
    float *out_float;
    // confidence variant of K2 (dsx_confidence of dsx.h): conf selects it; out_conf (uint8 H x W, may be
    // null) takes the peak-ratio map; pixels with q < conf_t get the invalid value after the LR test
    int conf, conf_t;
    uint8_t *out_conf;
};

constexpr int kStripWidth = 32;  // TX of bm2

// The minimum of the eight u16 costs of a 16-byte tile block.  Integer form: three v_pk_min_u16 and the low against
// the high half.  F16 form: v_pk_minimum3_f16 of three words, one v_pk_min_u16 with the fourth, then the halves - one
// packed op fewer.  For costs below 0x7C00 only: as f16 bit patterns those are finite and non-negative, which order as
// the integers do, and kernels run with f16 denormals kept (float_denorm_mode_16_64 = 3), so patterns below 0x0400
// are not flushed.  v_pk_minimum3_f16 issues in 4.12 cycles, as v_pk_min_u16 does (tools/ubench3.hip).  The nested
// llvm.minimum is how the instruction is named: gfx950 selects it as one op (tools/rowloop_isa.py counts them), and
// unlike an asm statement it leaves the block's 16-byte LDS read whole (the asm form read 12 + 4 bytes and spilled).
template <bool F16>
__device__ __forceinline__ uint32_t block_min8(uint4 v) {
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    typedef _Float16 hf2 __attribute__((ext_vector_type(2)));
    us2 mm;
    if constexpr (F16) {
        const hf2 m3 = __builtin_elementwise_minimum(
            __builtin_elementwise_minimum(__builtin_bit_cast(hf2, v.x), __builtin_bit_cast(hf2, v.y)), __builtin_bit_cast(hf2, v.z));
        mm = __builtin_elementwise_min(__builtin_bit_cast(us2, m3), __builtin_bit_cast(us2, v.w));
    } else {
        mm = __builtin_elementwise_min(__builtin_elementwise_min(__builtin_bit_cast(us2, v.x), __builtin_bit_cast(us2, v.y)),
                                       __builtin_elementwise_min(__builtin_bit_cast(us2, v.z), __builtin_bit_cast(us2, v.w)));
    }
    return mm.x < mm.y ? mm.x : mm.y;
}

// q = trunc(num / den2) (C semantics), den2 > 0, |q| small (the sub-pixel correction): float
// reciprocal estimate + exact integer fix-up; replaces the ~40-instruction integer division.
__device__ __forceinline__ int div_trunc_small(int num, int den2) {
    int q = (int)__builtin_truncf((float)num * __builtin_amdgcn_rcpf((float)den2));
    int r = num - q * den2;
    if (num >= 0) {
        if (r < 0) { --q; r += den2; }
        if (r >= den2) { ++q; }
    } else {
        if (r > 0) { ++q; r -= den2; }
        if (r <= -den2) { --q; }
    }
    return q;
}

// nw = waves per block: SAD Dp = 128*nw (nw in {1,2,4}), SSD Dp = 64*nw (nw in {1,2,4,8}); kind: the BM_*
// cost layout (pick_geometry in dsx_plan.h)
hipError_t launch_bm2(int radius, int kind, int nw, const Bm2Args &a, hipStream_t st);
hipError_t launch_volume_wta(int TX, bool ssd, const VolArgs &a, hipStream_t st);
// LR check after the left pass: invalidate x where |dR(x - m - d*) - d*| > lr over `rows` rows
// (frames stacked), reading this call's key buffer (double-buffered keys, see dsx_api.hip; the left
// pass resets the other half).
hipError_t launch_lr_fixup(const int16_t *dstar, const uint32_t *keys, uint32_t *keys_next, int reset_rows, int rows,
                           int W, int m, int lr, int kshift, int16_t *out_fixed, float *out_float, hipStream_t st);
// OpenCV's LR form after a side-0 left pass with sg_keys (DSX_LR_FORM_SGBM on the fused path): the floor
// and the ceiling of each sub-pixel disparity (fixed, the pass's x16 output kept in `fixed`) are tested
// against disp2 from the keys; a pixel is dropped when both land inside the image on a disp2 entry
// differing by more than max(lr, 1).  Writes out_fixed / out_float of the dropped pixels only.
hipError_t launch_lr_fixup_sgbm(const int16_t *fixed, const uint32_t *keys, int rows, int W, int m, int lr,
                                int kshift, int16_t *out_fixed, float *out_float, hipStream_t st);

size_t volume_smem_bytes(int TX, bool ssd, int Dp, int TPP, int W, bool conf = false);

// Semi-global aggregation (dsx_sgm.hip): one launch per path direction over the K1 volume.
struct SgmArgs {
    const uint16_t *C;  // [H][W][Dp] u16 SAD block costs (K1 output)
    uint32_t *S;        // [H][W][Dp] u32 path sums (written by the first direction, then +=)
    int H, W, D, Dp;
    int dx, dy;         // step direction of the path
    int P1, P2;
    uint32_t pads;      // S value for disparities >= D (never wins in K2)
};
hipError_t launch_sgm_path(const SgmArgs &a, bool first, hipStream_t st);

// All directions of a path set in one launch (dsx_sgm.hip, sgm_paths_all): every path writes its
// L_r (u16, exact while max cost + P2 < 65535) into its direction's [H][W][Dp] buffer; the K2
// variant (VolArgs.nsum) sums the buffers per slice.  Disparities >= D hold 0xFFFF.
struct SgmAllArgs {
    const uint16_t *C;  // [H][W][Dp] u16 SAD block costs (K1 output)
    uint16_t *L;        // ndir buffers of [H][W][Dp] u16, dir i at L + i * lstride
    size_t lstride;
    int H, W, D, Dp;
    int ndir;
    int dx[8], dy[8];
    int poff[9];        // first global path index of each direction (prefix sums)
    int P1, P2;
};
hipError_t launch_sgm_all(const SgmAllArgs &a, hipStream_t st);
int sgm_num_paths_host(int H, int W, int dx, int dy);

// Fast-mode epilogue (dsx_post.hip): crop + 3x3 median + optional depth.
struct PostArgs {
    const float *disp;  // H x W float disparity, row pitch in_pitch elements
    int64_t in_pitch;
    int H, W, crop;
    float *out_disp;   // H x (W - crop) or null
    float *out_depth;  // H x (W - crop) or null
    float fB, doffs, eps, max_depth;  // float32(f * B), float32(doffs), float32(eps), float32(max_depth)
    int has_max;
};
hipError_t launch_post_fast(const PostArgs &a, hipStream_t st);

// Launch options of the hole-filling march (dsx_inpaint.hip), carried by PostFullArgs too.
struct InpaintOpts {
    unsigned spin_limit = 0;            // grid-barrier spin bound of the persistent tail (0: default)
    int steps = -1;                     // step launches before the tail (-1: the previous call's count + 3)
    const void *status_key = nullptr;   // whose sticky timeout flag / step history (nullptr: the workspace)
};

// Full post-processing (speckles + outliers + median + depth), dsx_post.hip.
struct PostFullArgs {
    const float *disp;
    int64_t in_pitch;
    int H, W, crop;
    int max_speckle, max_diff16, apply_outliers, kernel;
    float thr;
    float *out_disp, *out_depth;
    float fB, doffs, eps, max_depth;
    int has_max;
    int fill_radius;  // > 0: hole filling between the outlier removal and the median: Telea (radius), or
    int fill_method;  // with DSX_FILL_NEAREST the iterated dilation (fill_radius = kernel_size)
    InpaintOpts fill_opts;  // status key (nullptr: the post-processing workspace), spin bound
    int tail_t1;      // post_tail writes the outlier-cleaned map to t1 instead of the median (set internally)
    // workspace views (set by launch_post_full)
    int *parent, *count, *root, *lsz;
    int16_t *v16;
    float *t0, *t1;
    // speckles of an int16 x16 map (launch_sgbm_post): in16 replaces disp, newv is the value that
    // marks removed / never-joining pixels (0 on the postprocess_disparity path)
    const int16_t *in16;
    int newv;
    int16_t *out16;
    // two-launch form (spk_tile + post_tail3): per-pixel 16-bit codes (the final x16 value, or
    // kSent: see `code` = the full 32-bit code), and the per-tile pending-node pool
    int16_t *code16;
    int *code, *pool;
    // the matcher's left-right check applied while the speckle pass loads the x16 map (the drop-in call
    // skips the lr_fixup launch): lr_keys != null -> A5' form (lr_form 0: lr_dstar = winner d or -1,
    // |key d - d| > lr_max drops the pixel) or OpenCV's form (1: floor / ceiling test, lr_dstar unused)
    const int16_t *lr_dstar;
    const uint32_t *lr_keys;
    int lr_form, lr_m, lr_max, lr_kshift;
    // diagnostics (DSX_POST_TIMELINE): per block 16 u64 - s_memrealtime after each phase, hw / xcc id
    uint64_t *tl_tile, *tl_tail;
};
size_t post_full_workspace(int H, int W, int crop);
// Optional per-launch hook (the handle's HIP-event timing of dsx_process_pair_device): before(name)
// right before a launch group, after() right after it.
struct LaunchHook {
    virtual void before(const char *name, hipStream_t st) = 0;
    virtual void after(hipStream_t st) = 0;
    virtual ~LaunchHook() = default;
};
// cv2.StereoSGBM::compute's own tail on an int16 x16 map: 3x3 median (BORDER_REPLICATE), then
// filterSpeckles(newVal, maxSpeckleSize, maxDiff) when max_speckle > 0.  Writes out16 and / or
// outf (= out16 / 16); `in` must not alias the outputs.
size_t sgbm_post_workspace(int H, int W);
hipError_t launch_sgbm_post(const int16_t *in, int H, int W, int newv, int max_speckle, int max_diff16, int16_t *out16,
                            float *outf, void *ws, hipStream_t st);
// The image-guided refinement hop of the chain (dsx_refine of dsx.h): between the hole filling and the
// median, on the cropped map.  guide: the uncropped H x W left image (read from column crop on).
struct RefineArgs {
    int type;  // kRefineNone | kRefineWmedian
    int radius, sigma, fill;
    const uint8_t *guide;
    int64_t guide_stride;
};
hipError_t launch_post_full(PostFullArgs a, void *ws, hipStream_t st, LaunchHook *hook = nullptr,
                            const RefineArgs *refine = nullptr);
// true when launch_post_full runs the two-launch speckle form (else the four-launch union-find)
bool post_full_two_launch(const PostFullArgs &a);

// Hole filling (dsx_inpaint.hip): fill_holes(method='inpaint') on d <= 0, Telea's march in
// arrival-time order (T-buckets, fixed-point sweeps).  Asynchronous: nothing is read back to the host.
size_t inpaint_workspace(int H, int W);
constexpr int kInpaintMaxW = 1 << 20;              // no row staging: only the pixel count is bounded
constexpr int64_t kInpaintMaxPixels = 1ll << 27;   // pop ranks (< 2 n) * 4 in 30 bits of the fill keys
hipError_t launch_inpaint(const float *in, int64_t pitch, int H, int W, int radius, float *out, void *ws, hipStream_t st,
                          const InpaintOpts &o = InpaintOpts{});
// 1 if a march with status key `key` (the caller's workspace, or a handle's) timed out (grid barrier
// or step cap) since the last call - its remaining holes stayed unfilled - and clears that flag; else 0
int inpaint_take_timeout(const void *key);
// the same over every key of the process (dsx_fill_holes_status)
int inpaint_take_timeout_any();
// drop the mapped status words of a key whose workspace is being freed
void inpaint_forget(const void *key);
void inpaint_forget_all();
bool inpaint_has_words();

// Hole filling by iterated dilation (dsx_nearest.hip): fill_holes(method='nearest') on d <= 0, k masked
// dilations with the ellipse footprint of radius k / 2.  Stateless, block barriers only.
constexpr int kNearestMaxK = 31;      // kernel_size bound: at most 31 footprint rows
constexpr int kNearestFusedMaxK = 5;  // the fused (all iterations in LDS) path's bound
constexpr int kNearestFused = 1, kNearestStep = 2;
constexpr int kFillInpaint = 0, kFillNearest = 1;  // PostFullArgs.fill_method (DSX_FILL_* of dsx.h)
// per-row half-widths of the footprint (hw[dy + r], -1: empty row); returns the row count 2 (k / 2) + 1,
// or -1 for k outside [0, kNearestMaxK] / cap too small.  Host only: the one C home of the ellipse rule.
int nearest_footprint(int k, int32_t *hw, int cap);
size_t nearest_workspace(int H, int W);  // the stepwise path's second buffer (k >= 2)
// path: kNearestFused (k <= kNearestFusedMaxK, ws unused) or kNearestStep (ws needed for k >= 2)
hipError_t launch_nearest(const float *in, int64_t pitch, int H, int W, int k, float *out, float *ws, int path,
                          hipStream_t st);

// Image-guided weighted median (dsx_wmedian.hip): out(p) = the weighted median of the valid (0 < d < inf)
// taps of p's (2 r + 1)^2 window, weights T[|G(p) - G(q)|] from the guide.  Stateless, one launch.
constexpr int kRefineNone = 0, kRefineWmedian = 1;  // DSX_REFINE_*
constexpr int kWmedianMinRadius = 1, kWmedianMaxRadius = 7;
constexpr int kWmedianMinSigma = 1, kWmedianMaxSigma = 64;
// T[k] = max(1, floor(256 exp(-k / sigma) + 0.5)) in doubles; -1 for sigma outside [1, 64] or a null array.
// Host only: the one C home of the weight rule.
int wmedian_weights(int sigma, uint16_t *out256);
// in: H x W floats, row pitch `pitch` elements; guide: H x W bytes, row stride gstride; out: contiguous, not in
hipError_t launch_wmedian(const float *in, int64_t pitch, int H, int W, const uint8_t *guide, int64_t gstride, int r,
                          int sigma, int fill, float *out, hipStream_t st);

// Birchfield-Tomasi block costs into K1's volume layout (dsx_bt.hip, oracle/bt_cost.py)
struct BtArgs {
    const uint2 *prepL, *prepR;  // bt_prep records of both views
    uint16_t *hs;                // horizontal sums [H][W][Dp]
    void *vol;                   // out: [H][W][Dp] u16, pads >= D
    int H, W, m, D, Dp, R;
    uint32_t padv;
};
size_t bt_workspace(int H, int W, int Dp);
hipError_t launch_bt_prep(const uint8_t *img, int64_t pitch, int H, int W, int ftz, uint2 *out, hipStream_t st);
// part 0: horizontal sums (bt_hsum), part 1: vertical sums into the volume (bt_vsum)
hipError_t launch_bt_volume(const BtArgs &a, int part, hipStream_t st);

// Census block costs into K1's volume layout (dsx_census.hip, depthestimation_amd/census.py)
constexpr int kCensus9x7 = 3, kCensus5x5 = 4;  // DSX_COST_CENSUS*: the window is the cost's name
constexpr int kCensusSeg = 16;                 // rows per census_volume segment (the sweep of DESIGN.md 4.3e)
struct CensusArgs {
    const uint8_t *src[2];  // view v (nviews of them, grid z), row stride `stride` bytes
    int64_t stride;
    void *dst[2];           // contiguous H x W codes: u64, or u32 (5x5 with out64 = 0)
    int nviews, H, W;
    int window;             // kCensus9x7 | kCensus5x5
    int out64;
};
struct CensusVolArgs {
    const void *codeL, *codeR;  // census_transform's planes (9x7: u64, 5x5: u32)
    void *vol;                  // out: [H][W][Dp] u16, pads >= D
    int H, W, m, D, Dp, R;
    int window;
    int seg;                    // rows per segment; 0: kCensusSeg
    uint32_t padv;
};
size_t census_code_bytes(int window);  // bytes per code inside the handle
hipError_t launch_census_transform(const CensusArgs &a, hipStream_t st);
hipError_t launch_census_volume(const CensusVolArgs &a, hipStream_t st);

// Rectification (dsx_rectify.hip): gray conversion fused with the fixed-point bilinear remap.
struct RectArgs {
    const uint8_t *img;  // Hs x Ws x channels (channels 1 or 3, BGR order), row stride in bytes
    int64_t stride;
    int Hs, Ws;
    const float *mapx, *mapy;  // H x W float32 maps (null: gray conversion only, output Hs x Ws)
    int H, W;
    uint8_t *out;              // H x W uint8, contiguous
};
hipError_t launch_rectify(const RectArgs &a, int channels, hipStream_t st);

// Area downscale (dsx_resize.hip): input.py resize_area (Pillow BOX, two u8 passes) on the device.
// (start, count, k) of each of the out_size outputs of one axis, in doubles on the host; -1 for
// out_size < 1, out_size > in_size or a null array.  Host only: the one C home of the window rule.
int resize_area_table(int in_size, int out_size, int32_t *start, int32_t *count, int32_t *coef);
// One launch on the current device; the tables come from a library-owned cache (8 shapes per device),
// uploaded on `st` at a shape's first use.  gray: 3 channels in, one gray byte per pixel out.
hipError_t launch_resize_area(const uint8_t *img, int64_t stride, int Hs, int Ws, int channels, int Ho, int Wo,
                              bool gray, uint8_t *out, int64_t out_stride, hipStream_t st);
bool resize_has_tables();
void resize_forget_all();  // frees every cached table (dsx_shutdown)

// Matcher prefilter and texture threshold (dsx_prefilter.hip; dsx_prefilter of dsx.h).
constexpr int kPrefNone = 0, kPrefXsobel = 1, kPrefMean = 2;  // DSX_PREFILTER_*
struct PrefilterArgs {
    const uint8_t *src[2];  // view v (nviews of them), frame f at src[v] + f * frame_stride
    int64_t stride, frame_stride;
    uint8_t *dst[2];        // view v, frame f at dst[v] + f * dframe, row pitch dpitch
    int64_t dpitch, dframe;
    int dwidth;             // writable bytes of an output row (W <= dwidth <= dpitch): rows whose
                            // start is 16-B aligned are written in 16-B stores up to dwidth
    int dal;                // set by the launcher: every output row starts 16-B aligned
    int nviews, nframes, H, W;
    int type, n, cap;       // kPrefXsobel | kPrefMean (window n, odd, 5..21); cap 1..63
};
hipError_t launch_prefilter(const PrefilterArgs &a, hipStream_t st);
// T = block x block sum of |P - cap| (clamped coordinates) over nframes prefiltered frames.  out_sum
// (u16, contiguous [nframes][H][W]) set: T is written; otherwise the pixels with T < thr get inv16 in
// out_fixed and invf in out_float (contiguous [nframes][H][W], either may be null).
struct TextureArgs {
    const uint8_t *pref;
    int64_t stride, frame_stride;
    int nframes, H, W, block, cap, thr;
    uint16_t *out_sum;
    int16_t *out_fixed;
    float *out_float;
    int inv16;
    float invf;
};
hipError_t launch_texture(const TextureArgs &a, hipStream_t st);



}  // namespace dsx
