/*
 * dsx.h - C-ABI of the MI355X stereo block-matching engine (libdsx.so).
 *
 * This is the drop-in boundary for the reference's hot path. In the reference
 * (mspaintenjoyer/DepthEstimation, Python) the path is a third-party matcher object:
 *
 *   depthlib/stereo_core.py:63-75   self.sgbm = cv2.StereoSGBM_create(minDisparity=..., ...)
 *   depthlib/stereo_core.py:231     disp_fixed = self.sgbm.compute(rectified_L, rectified_R)
 *   depthlib/stereo_core.py:232     return disp_fixed.astype(np.float32) / 16.0
 *
 * A reference-side binding (ctypes) maps
 *   cv2.StereoSGBM_create(...)  -> dsx_create()          (matcher construction)
 *   matcher.compute(L, R)       -> dsx_compute_host()     (int16 x16 fixed-point result)
 *   (device-resident callers)   -> dsx_compute_device()   (async, HIP stream)
 *   matcher lifetime (GC)       -> dsx_destroy()
 *
 * Plain C types only: pointers, sizes, int32/int64. No torch / HIP types in signatures
 * (streams are passed as void*). All functions return 0 on success or a negative
 * DSX_E* code; they never abort or throw across the ABI. dsx_last_error() returns a
 * thread-local message for the last failure on the calling thread.
 *
 * Threading: a handle is not thread-safe; use one handle per thread / GPU. Different
 * handles are independent. Every call does hipSetDevice(handle device) first.
 */
#ifndef DSX_H
#define DSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSX_VERSION 106 /* additive since 1.0.6 (layouts unchanged): dsx_block_min8_device (the fused SAD pass's
                           block minimum alone, for tests); dsx_upsample, dsx_default_upsample,
                           dsx_check_upsample, dsx_upsample_taps, dsx_upsample_x0, dsx_upsample_device
                           (joint bilateral upsampling of a downscaled run's map to the full-size frame);
                           dsx_temporal_params, dsx_default_temporal,
                           dsx_check_temporal, dsx_temporal_gains, dsx_tfilter_create, dsx_tfilter_set_params,
                           dsx_tfilter_reset, dsx_tfilter_destroy, dsx_tfilter_bytes, dsx_tfilter_run_device
                           (temporal disparity filter for video: motion-gated recursive average);
                           dsx_cloud, dsx_check_cloud,
                           dsx_reproject_device, dsx_point_cloud_workspace_bytes, dsx_point_cloud_device
                           (disparity -> XYZ, ordered point-cloud compaction);
                           dsx_confidence, dsx_default_confidence,
                           dsx_check_confidence, dsx_set_confidence, dsx_compute_conf_device, dsx_compute_conf_host
                           (matcher confidence map + threshold);
                           dsx_refine, dsx_default_refine, dsx_check_refine,
                           dsx_wmedian_weights, dsx_wmedian_device, dsx_postprocess_refine_device,
                           dsx_process_pair_refine_device (image-guided weighted median);
                           DSX_COST_CENSUS*, dsx_census_device, dsx_resize_area_*, dsx_fill_nearest_*,
                           dsx_postprocess_device,
                           dsx_prefilter, dsx_default_prefilter, dsx_check_prefilter, dsx_set_prefilter,
                           dsx_prefilter_device, dsx_texture_sum_device (matcher prefilter + texture threshold);
                           dsx_post_params.fill_method (a former reserved slot; 0 = as before);
                           1.0.6: hole filling in OpenCV's own arithmetic and exact queue order, dsx_fill_holes_release,
                           dsx_shutdown;
                           1.0.5: arrival-order hole filling, per-workspace / per-handle fill status, dsx_fill_opts;
                           1.0.4: dsx_params.in_flight; 1.0.3: dsx_process_pair_device, dsx_fill_holes_status */

#define DSX_OK 0
#define DSX_EINVAL (-1) /* bad argument (mirrors ValueError / cv2.error on bad input) */
#define DSX_EHIP (-2)   /* HIP runtime error */
#define DSX_ECOMM (-3)  /* RCCL (collective) error */
#define DSX_ENOMEM (-4) /* device allocation failed */

#define DSX_COST_SAD 0
#define DSX_COST_SSD 1
/* OpenCV SGBM's pixel cost (Birchfield-Tomasi on the prefilter_cap-clipped x-derivative plus the
 * raw intensity >> 2, cv2.StereoSGBM preFilterCap, stereo_core.py:63-75) summed over the same
 * block window; runs on the volume path (K1 replaced by the BT volume, then K2 / SGM). */
#define DSX_COST_BT 2
/* Census costs: the Hamming distance between local rank codes, invariant to any monotone intensity change
 * per window.  An addition of this build (as the prefilter is): parity with nothing outside this
 * repository is claimed.  The cost's name carries the window wx x wy: 9x7 (62 bits, the usual choice under
 * SGM) or 5x5 (24 bits).  With cx / cy the replicate clamp, rx = wx / 2, ry = wy / 2:
 *   code T(I)(x, y): the neighbours (i, j), j from -ry to ry (outer), i from -rx to rx (inner), the centre
 *       skipped, counted k = 0, 1, ...; bit k = 1 iff I(cx(x+i), cy(y+j)) < I(x, y) (strict); upper bits 0.
 *   block cost (the A5' window, block_size 1..15; 1 = the per-pixel Hamming cost used with SGM):
 *       C(x, y, d) = sum over |i|, |j| <= r of popcount(T_L[cy(y+j), cx(x+i)] xor T_R[cy(y+j), cx(x+i-m-d)])
 *       (the coordinates of the codes are clamped, not the codes' inputs); at most 225 * 62 = 13,950.
 * Everything after C is unchanged (WTA, uniqueness, both LR forms, sub-pixel, float modes, sgbm_post, SGM).
 * Like BT, census costs exist only as a volume: a handle with path FUSED runs the volume path (two
 * launches, census_transform and census_volume, replace K1), dsx_right_map_device returns DSX_EINVAL, and a
 * prefilter or a texture threshold with a census cost is DSX_EINVAL (census ranks intensities itself). */
#define DSX_COST_CENSUS9X7 3
#define DSX_COST_CENSUS5X5 4

#define DSX_FLOAT_FIXED 0    /* out_float = out_fixed / 16 (stereo_core.py:232 contract) */
#define DSX_FLOAT_PARABOLA 1 /* out_float = continuous parabola vertex (north-star 1e-3 path) */

/* Left-right check form (dsx_params.lr_form):
 *   DSX_LR_FORM_BM   : the right-view winner of every right pixel is the argmin over ALL costs
 *                      C(xr + m + d, d) (lowest d); valid band x in [m + D - 1, W - 1 + m]; the
 *                      check runs when disp12_max_diff >= 0 (SURVEY.md 8a row A5').
 *   DSX_LR_FORM_SGBM : cv2.StereoSGBM's own form (stereo_core.py:63-75): disp2 is built from the
 *                      unique LEFT winners only (minimum cost; equal costs: the largest x), each
 *                      sub-pixel disparity's floor and ceiling are tested and the pixel is dropped
 *                      only if both have a disp2 entry and both differ by more than disp12MaxDiff
 *                      (which is max(disp12_max_diff, 1): always on); valid band
 *                      x in [max(m + D, 0), W + min(m, 0)).  Runs on both paths: the volume path
 *                      in K2, the fused path as a separate left-pass build (each unique winner
 *                      offers its key by one atomicMin) + lr_fixup_sgbm. */
#define DSX_LR_FORM_BM 0
#define DSX_LR_FORM_SGBM 1

#define DSX_PATH_FUSED 0  /* cost computed in LDS, never written to HBM (default) */
#define DSX_PATH_VOLUME 1 /* K1 writes the [H][W][D] cost volume to HBM, K2 reduces it */

/* Semi-global aggregation over the SAD block costs: the path sets the
 * reference selects with sgbm_mode (stereo_core.py:55-61).  With aggregation != 0 the volume
 * path runs K1, one pass per direction into u32 path sums, then K2 on the sums. */
#define DSX_AGG_NONE 0
#define DSX_AGG_SGBM_3WAY 3 /* 'sgbm_3way': left->right, right->left, top->bottom          */
#define DSX_AGG_HH4 4       /* 'hh4'      : the 3-way set plus bottom->top                   */
#define DSX_AGG_SGBM 5      /* 'sgbm'     : the 3-way set plus the two top diagonals         */
#define DSX_AGG_HH 8        /* 'hh'       : all 8 neighbours                                 */

/* Matcher parameters. Field meaning follows StereoCore.sgbm_params
 * (depthlib/stereo_core.py:16-39) for the keys that exist there. */
typedef struct dsx_params {
    int32_t min_disp;         /* 'min_disp'          (stereo_core.py:17, cv2 minDisparity)    */
    int32_t num_disp;         /* 'num_disp'          (stereo_core.py:18, cv2 numDisparities)  */
    int32_t block_size;       /* 'block_size'        (stereo_core.py:19), odd, 1..15          */
    int32_t cost;             /* DSX_COST_SAD | _SSD | _BT | _CENSUS9X7 | _CENSUS5X5 (build key 'cost') */
    int32_t uniqueness_ratio; /* 'uniqueness_ratio'  (stereo_core.py:22), 0 disables, <100    */
    int32_t disp12_max_diff;  /* 'disp12_max_diff'   (stereo_core.py:20), <0 disables LR      */
    int32_t subpixel;         /* build key 'subpixel': 1 = 1/16-px parabola, 0 = integer      */
    int32_t float_mode;       /* DSX_FLOAT_FIXED | DSX_FLOAT_PARABOLA                          */
    int32_t path;             /* DSX_PATH_FUSED | DSX_PATH_VOLUME                              */
    int32_t timing;           /* 1 = record per-kernel HIP-event timings (dsx_kernel_times)   */
    int32_t grid_blocks;      /* 0 = one persistent block per resident slot; >0 forces the   */
                              /* persistent grid size (tests of the work partition)         */
    int32_t aggregation;      /* DSX_AGG_*: 0 = plain block matching (default); otherwise the */
                              /* SGM path set of 'sgbm_mode' (stereo_core.py:55-61), SAD only */
    int32_t p1, p2;           /* SGM penalties; <= 0 -> 8*bs^2 / 32*bs^2 (stereo_core.py:51-52) */
    int32_t prefilter_cap;    /* 'prefilter_cap'     (stereo_core.py:21), 1..63; DSX_COST_BT only */
    int32_t sgbm_post;        /* 1 = cv2.StereoSGBM::compute's own tail on the int16 map: 3x3     */
                              /* median, then filterSpeckles(newVal (min_disp-1)*16) when          */
                              /* speckle_window_size > 0; needs float_mode DSX_FLOAT_FIXED         */
    int32_t speckle_window_size; /* 'speckle_window_size' (stereo_core.py:23), >= 0              */
    int32_t speckle_range;    /* 'speckle_range'     (stereo_core.py:24), maxDiff = 16 * range   */
    int32_t lr_form;          /* DSX_LR_FORM_BM (default) | DSX_LR_FORM_SGBM                     */
    int32_t in_flight;        /* 1: the caller keeps other frames in flight on other handles and  */
                              /* streams (multigpu.DepthPipeline / HostPipeline): the fused pass  */
                              /* drops the balance that makes one frame's blocks finish together */
                              /* (priority bands, age weights) - the next frame fills the tail     */
    int32_t reserved[2];
} dsx_params;

typedef struct dsx_handle dsx_handle;

/* Library version (DSX_VERSION). */
int dsx_version(void);

/* Number of visible HIP devices. */
int dsx_device_count(int *n);

/* Fill *p with the defaults of StereoCore.sgbm_params (stereo_core.py:16-39) plus the build
 * keys: min 0, num 128, block 5, SAD, uniqueness 10, disp12 1, subpixel 1, fixed floats,
 * fused path, prefilter_cap 31, sgbm_post 0, speckle window 50 / range 2. */
void dsx_default_params(dsx_params *p);

/* Validate parameters without creating a handle (DSX_EINVAL + message if unsupported). */
int dsx_check_params(const dsx_params *p);

/* Create a matcher on `device` (replaces cv2.StereoSGBM_create, stereo_core.py:63-75). */
int dsx_create(int device, const dsx_params *p, dsx_handle **out);

/* Replace the parameters of an existing matcher (configure_sgbm -> _build_sgbm,
 * stereo_core.py:77-123). The parameters are validated first (DSX_EINVAL names the cause and the
 * handle keeps its old set; so does a switch to DSX_COST_BT or a census cost while a prefilter is set). The next
 * call grows every cached device buffer that the new set needs larger (e.g. the SGM buffer with the
 * direction count); a buffer may stay larger than needed. */
int dsx_set_params(dsx_handle *h, const dsx_params *p);

/* Matcher prefilter and texture threshold (cv2.StereoBM's preFilterType / preFilterSize / preFilterCap /
 * textureThreshold, in this build's own arithmetic; parity with OpenCV unpinned).  With c = cap, cx / cy the
 * replicate clamp into the image:
 *   DSX_PREFILTER_XSOBEL: P(x, y) = clip(Sx, -c, c) + c,
 *       Sx = 2 (I(x+1, y) - I(x-1, y)) + I(x+1, cy(y-1)) - I(x-1, cy(y-1)) + I(x+1, cy(y+1)) - I(x-1, cy(y+1));
 *       columns 0 and W-1 hold c.
 *   DSX_PREFILTER_MEAN (window n = size): S = sum of I(cx(x+i), cy(y+j)) over |i|, |j| <= n/2,
 *       mu = (S + n*n/2) / (n*n) (integer division), P = clip(I - mu, -c, c) + c.
 * P is uint8 in [0, 2c].  Both views are filtered into handle-owned buffers and the matcher runs on them
 * exactly as it runs on raw images (any SAD / SSD configuration; dsx_right_map_device too).
 *   texture_threshold t > 0 (needs a prefilter): T(x, y) = sum of |P_L(cx(x+i), cy(y+j)) - c| over the
 *       matcher's block window; a pixel with T < t gets the invalid value ((min_disp - 1) * 16; min_disp - 1
 *       in the float map) after uniqueness, sub-pixel and the LR check, before the sgbm_post tail.
 * DSX_COST_BT filters for itself: BT with a prefilter is DSX_EINVAL.  With type NONE and threshold 0
 * (the default) a handle runs no extra launch and owns no extra buffer. */
#define DSX_PREFILTER_NONE 0
#define DSX_PREFILTER_XSOBEL 1
#define DSX_PREFILTER_MEAN 2
typedef struct dsx_prefilter {
    int32_t type;              /* DSX_PREFILTER_*                                                   */
    int32_t size;              /* window of DSX_PREFILTER_MEAN: odd, 5..21 (checked for any filter)  */
    int32_t cap;               /* 1..63                                                             */
    int32_t texture_threshold; /* 0 (off) .. 65535                                                  */
    int32_t reserved[4];
} dsx_prefilter;

/* none, size 9, cap 31, threshold 0 */
void dsx_default_prefilter(dsx_prefilter *f);

/* Validate a prefilter, alone (p NULL) or against matcher parameters (no handle, no device). */
int dsx_check_prefilter(const dsx_params *p, const dsx_prefilter *f);

/* Set the handle's prefilter (NULL = off), validated against its current parameters; on error the
 * handle keeps its old set.  dsx_set_params in turn validates new parameters against the prefilter. */
int dsx_set_prefilter(dsx_handle *h, const dsx_prefilter *f);

/* The filter alone, for callers that filter themselves (stateless, asynchronous on hip_stream):
 * d_img uint8 H x W with row stride stride_bytes -> d_out uint8 H x W with row stride out_stride_bytes
 * (not d_img).  Any alignment; 16-B aligned rows take the wide loads / stores. */
int dsx_prefilter_device(const void *d_img, int32_t H, int32_t W, int64_t stride_bytes, const dsx_prefilter *f,
                         void *d_out, int64_t out_stride_bytes, void *hip_stream);

/* T of a prefiltered image: d_out_u16 contiguous uint16 H x W (at most 225 * 63 for a filtered image).
 * block_size odd, 1..15; cap 1..63.  Stateless, asynchronous on hip_stream. */
int dsx_texture_sum_device(const void *d_pref, int32_t H, int32_t W, int64_t stride_bytes, int32_t block_size,
                           int32_t cap, void *d_out_u16, void *hip_stream);

/* The census transform alone (stateless, asynchronous on hip_stream): d_img uint8 H x W with row stride
 * stride_bytes (any pitch and alignment) -> d_out_u64 contiguous uint64 H x W codes of the window named by
 * `cost` (DSX_COST_CENSUS9X7: 62 bits, DSX_COST_CENSUS5X5: 24 bits; the upper bits 0). */
int dsx_census_device(const void *d_img, int32_t H, int32_t W, int64_t stride_bytes, int32_t cost, void *d_out_u64,
                      void *hip_stream);

/* The fused SAD pass's block minimum in its packed-f16 form, alone (stateless, asynchronous on hip_stream; for
 * tests): d_blocks n 16-byte blocks of eight uint16 costs, each below 0x7C00 -> d_out_u32[i] = the minimum of block
 * i's eight costs, taken as the pass takes it (v_pk_minimum3_f16 of three words, integer minima of the rest). */
int dsx_block_min8_device(const void *d_blocks, int64_t n, void *d_out_u32, void *hip_stream);

/* Matcher confidence map and confidence threshold.  An addition of this build (as the prefilter and the
 * census costs are): parity with nothing outside this repository is claimed.
 * Let C(x, y, d), d in [0, D), be the costs the epilogue decides on (block costs of any `cost`, or SGM path
 * sums), b the lowest-d argmin, cb = C(b), and nm the minimum of C(d) over the real disparities with
 * |d - b| > 1 (the set the uniqueness test scans).  DSX_CONF_PEAK_RATIO is the uint8
 *   q = 255                        if that set is empty (D <= 2, or D = 3 with b = 1),
 *   q = 0                          if nm == 0 (then cb == 0: a perfect tie),
 *   q = 255 - (255 * cb) / nm      otherwise (integer division; cb <= nm, so q is in [0, 255]),
 *   q = 0                          outside the handle's valid band (lr_form BM: [m + D - 1, W - 1 + m];
 *                                  SGBM: [max(m + D, 0), W + min(m, 0))).
 * q describes the WTA decision alone: it does not depend on the uniqueness, LR, texture, sub-pixel or
 * sgbm_post outcomes.  Every in-band pixel that uniqueness_ratio u rejects has q <= 255 - (255 (100 - u)) / 100.
 *   threshold t in [0, 255], 0 = off: a pixel with q < t gets the invalid value ((min_disp - 1) * 16;
 *       min_disp - 1 in the float map) after the LR check of either form - it still takes part in the
 *       right-view winners and, for DSX_LR_FORM_SGBM, still offers its key - and before the texture mask
 *       and the sgbm_post tail.
 * The map comes from K2 of the volume path: a call that is handed a confidence output, and every call of a
 * handle whose threshold is > 0, runs the volume path also on a handle that otherwise runs the fused pass
 * (same disparities; the volume buffer is allocated on first need and such a call uses handle scratch).
 * The handle's other calls stay fused.  dsx_right_map_device is unaffected.  dsx_compute_device,
 * dsx_compute_batch_device and dsx_process_pair*_device honour the threshold and return no map. */
#define DSX_CONF_PEAK_RATIO 1
typedef struct dsx_confidence {
    int32_t type;      /* DSX_CONF_PEAK_RATIO */
    int32_t threshold; /* 0 (off) .. 255      */
    int32_t reserved[6];
} dsx_confidence;

/* PEAK_RATIO, threshold 0 */
void dsx_default_confidence(dsx_confidence *c);

/* Validate a confidence set, alone (p NULL) or against matcher parameters (no handle, no device). */
int dsx_check_confidence(const dsx_params *p, const dsx_confidence *c);

/* Set the handle's confidence set (NULL = default); on error the handle keeps its old set. */
int dsx_set_confidence(dsx_handle *h, const dsx_confidence *c);

/* dsx_compute_device / dsx_compute_host with the confidence map: d_out_conf / out_conf uint8 H x W,
 * contiguous.  With it NULL these are exactly dsx_compute_device / dsx_compute_host; otherwise at least one
 * of the three outputs is required (the host call needs no out_fixed then).  Argument errors are reported
 * before any HIP call. */
int dsx_compute_conf_device(dsx_handle *h, const void *dL, const void *dR, int32_t H, int32_t W, int64_t stride_bytes,
                            void *d_out_fixed, void *d_out_float, void *d_out_conf, void *hip_stream);
int dsx_compute_conf_host(dsx_handle *h, const uint8_t *L, const uint8_t *R, int32_t H, int32_t W, int64_t stride_bytes,
                          int16_t *out_fixed, float *out_float, uint8_t *out_conf);

/* Synchronous host-buffer compute (replaces matcher.compute, stereo_core.py:231).
 * L, R: uint8 H x W with row stride `stride_bytes` (>= W).  out_fixed: int16 H x W
 * (required, contiguous).  out_float: float32 H x W or NULL. */
int dsx_compute_host(dsx_handle *h, const uint8_t *L, const uint8_t *R, int32_t H, int32_t W,
                     int64_t stride_bytes, int16_t *out_fixed, float *out_float);

/* Asynchronous device-pointer compute on `hip_stream` (hipStream_t, NULL = default stream).
 * dL, dR: device uint8 H x W, row stride `stride_bytes`.  d_out_fixed (int16) and
 * d_out_float (float32) are contiguous H x W device buffers; either may be NULL but not
 * both.  No host synchronisation, no allocation when the size matches the cached one.
 * Calls on different streams through ONE handle are safe: a configuration that uses the handle's
 * scratch (LR check, volume path, BT or census cost, SGM, sgbm_post, a prefilter's filtered images) orders a call
 * on a new stream after the previous call's last kernel (stream wait on an event, no host wait); the
 * plain fused pass without a prefilter owns no scratch and runs concurrently.  Inputs and outputs
 * are the caller's: they must stay valid and unmodified until the work on hip_stream has completed. */
int dsx_compute_device(dsx_handle *h, const void *dL, const void *dR, int32_t H, int32_t W,
                       int64_t stride_bytes, void *d_out_fixed, void *d_out_float,
                       void *hip_stream);

/* Batched asynchronous compute of `nframes` frame pairs in ONE launch (video streams,
 * StereoDepthEstimatorVideo.py:69-147 frames handed over in groups): frame f's inputs start at
 * dL + f * frame_stride_bytes (same for dR); outputs are contiguous [nframes][H][W].  Same
 * results as nframes calls of dsx_compute_device; the persistent grid spreads the
 * (frame, strip, row) work, which amortises per-launch and per-run costs for small frames. */
int dsx_compute_batch_device(dsx_handle *h, int32_t nframes, const void *dL, const void *dR, int64_t frame_stride_bytes,
                             int32_t H, int32_t W, int64_t stride_bytes, void *d_out_fixed, void *d_out_float,
                             void *hip_stream);

/* Right-view winner map only (the LR check's dR, int16 H x W, -1 where the search range is
 * empty). Exposed for parity tests of the right pass. Async on hip_stream. */
int dsx_right_map_device(dsx_handle *h, const void *dL, const void *dR, int32_t H, int32_t W,
                         int64_t stride_bytes, void *d_out_dR, void *hip_stream);

/* Fast-mode epilogue on the device, replacing the host steps after the
 * matcher in StereoCore._process_pair with fast_mode=True (stereo_core.py:168-196):
 *   out_disp  = medianBlur(disp[:, crop:], 3)               (:168 crop by num_disp, :173 median,
 *                                                            replicated border of the cropped map)
 *   out_depth = f*B / (out_disp + doffs) where out_disp + doffs > eps, else +inf;
 *               clamped to max_depth when has_max_depth     (:186-196 -> disparity_to_depth :234-272)
 * d_disp: float32 H x W, row pitch `in_pitch` elements (>= W).  d_out_disp / d_out_depth: contiguous
 * float32 H x (W - crop); either may be NULL.  Scalars follow numpy-2 float32 rules (f*B, doffs,
 * eps, max_depth are rounded to float32), so results equal the host path bit for bit.
 * No handle: stateless, asynchronous on hip_stream. */
int dsx_postprocess_fast_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t crop,
                                void *d_out_disp, void *d_out_depth, double focal_length, double baseline,
                                double doffs, double eps, double max_depth, int32_t has_max_depth,
                                void *hip_stream);

/* Full post-processing on the device, replacing postprocess_disparity
 * (postprocess.py:120-171) as StereoCore._process_pair calls it without fast mode
 * (stereo_core.py:175-184) and with hole filling off (its default, stereo_core.py:38):
 *   speckle filter (x16 int16, max_speckle_size, max_diff) -> optional box-statistics outlier removal
 *   (kernel x kernel, threshold) -> 3x3 median -> optional depth (same scalars as
 *   dsx_postprocess_fast_device).  Input cropped by `crop` columns first (stereo_core.py:168).
 * d_workspace: >= dsx_postprocess_workspace_bytes(H, W, crop) bytes of device memory. Async. */
size_t dsx_postprocess_workspace_bytes(int32_t H, int32_t W, int32_t crop);
int dsx_postprocess_full_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t crop,
                                int32_t max_speckle_size, double max_diff, int32_t apply_outlier_removal,
                                double outlier_threshold, int32_t outlier_kernel, void *d_out_disp,
                                void *d_out_depth, double focal_length, double baseline, double doffs, double eps,
                                double max_depth, int32_t has_max_depth, void *d_workspace,
                                size_t workspace_bytes, void *hip_stream);

/* As dsx_postprocess_full_device, with hole filling (StereoCore hole_filling=True: fill_holes
 * method 'inpaint', postprocess.py:160-166, stereo_core.py:175-184) between the outlier removal and
 * the median when fill_radius > 0 (the reference passes fill_kernel 3, postprocess.py:165). Async. */
int dsx_postprocess_full_ex_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t crop,
                                   int32_t max_speckle_size, double max_diff, int32_t apply_outlier_removal,
                                   double outlier_threshold, int32_t outlier_kernel, int32_t fill_radius,
                                   void *d_out_disp, void *d_out_depth, double focal_length, double baseline,
                                   double doffs, double eps, double max_depth, int32_t has_max_depth,
                                   void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* fill_holes(disparity, method='inpaint', kernel_size=radius) on the device (postprocess.py:72-118,
 * cv2.inpaint INPAINT_TELEA on d <= 0) as OpenCV's inpaint.cpp does it (recalled): the outward march
 * over the known pixels within `radius` of a hole, then the inward march with Telea's float32 values,
 * OpenCV's normalised gradient term and + 0.5, both in the queue's exact (T, push order) order.  Equal
 * bit for bit to the sequential march (oracle/telea_cv.c) and the host restatement (postprocess.py
 * _telea_inpaint).  radius < 1 is taken as 1 (OpenCV clamps its range to [1, 100]).
 * d_disp: float32 H x W, row pitch `in_pitch` elements; d_out: contiguous float32 H x W; H * W < 2^27.
 * d_workspace: >= dsx_fill_holes_workspace_bytes(H, W).  Asynchronous on hip_stream: the march runs
 * as step launches (as many as the previous call on this workspace needed) plus one persistent
 * launch for any steps beyond them; nothing is read back to the host. */
size_t dsx_fill_holes_workspace_bytes(int32_t H, int32_t W);
int dsx_fill_holes_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t radius, void *d_out,
                          void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* fill_holes(disparity, method='nearest', kernel_size=k) on the device (postprocess.py:106-116): with
 * mask = d <= 0 taken from the input and r = k / 2, k times f <- where(mask, dilate(f, ellipse(r)), f);
 * every iteration reads only the previous one.  Taps outside the image are skipped (equal to the
 * host's replicated border for these footprints); values <= 0 take part in the max; holes further
 * than k * r from a valid pixel stay <= 0; k = 0 and k = 1 copy.  A float max only: bit-exact with the
 * host restatement (depthestimation_amd/postprocess.py fill_holes).  Stateless: no grid barrier, no
 * status flag, nothing to time out; calls on different streams are independent.
 *
 * dsx_fill_nearest_footprint (host only): the ellipse as per-row half-widths, halfwidths[dy + r] for
 *   dy in [-r, r] (-1: an empty row), by numpy's float64 rule (dy / r)^2 + (dx / r)^2 <= 1.0 (r = 0:
 *   the single pixel).  Writes 2 (k / 2) + 1 values and returns that count; DSX_EINVAL for
 *   kernel_size outside [0, 31], a NULL array or cap too small.
 * dsx_fill_nearest_device: d_disp float32 H x W, row pitch `in_pitch` elements; d_out contiguous
 *   float32 H x W, not d_disp.  path: DSX_NEAREST_AUTO, DSX_NEAREST_FUSED (all iterations of a tile
 *   in LDS, kernel_size <= DSX_NEAREST_FUSED_MAX, no workspace: d_workspace may be NULL) or
 *   DSX_NEAREST_STEPWISE (one launch per iteration, any kernel_size <= 31; for kernel_size >= 2 it
 *   needs >= dsx_fill_nearest_workspace_bytes(H, W) of workspace).  Auto is fused up to
 *   DSX_NEAREST_FUSED_MAX, stepwise beyond.  Asynchronous on hip_stream. */
#define DSX_NEAREST_AUTO 0
#define DSX_NEAREST_FUSED 1
#define DSX_NEAREST_STEPWISE 2
#define DSX_NEAREST_FUSED_MAX 5
int dsx_fill_nearest_footprint(int32_t kernel_size, int32_t *halfwidths, int32_t cap);
size_t dsx_fill_nearest_workspace_bytes(int32_t H, int32_t W);
int dsx_fill_nearest_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t kernel_size,
                            void *d_out, void *d_workspace, size_t workspace_bytes, int32_t path, void *hip_stream);

/* Launch shape of the march (tests and experiments; zero-initialised = the defaults). */
typedef struct dsx_fill_opts {
    uint32_t spin_limit; /* grid-barrier spin bound of the persistent launch (0: default, ~2 s)    */
    int32_t steps;       /* step launches before it: 0 adaptive, > 0 that many, < 0 none           */
    int32_t reserved[6];
} dsx_fill_opts;
int dsx_fill_holes_ex_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t radius, void *d_out,
                             void *d_workspace, size_t workspace_bytes, const dsx_fill_opts *opts, void *hip_stream);

/* Timeout reports.  A march whose persistent launch times out (a grid barrier, or the step bound)
 * leaves the holes of that call unfilled and raises a sticky flag that belongs to the caller's
 * workspace (dsx_fill_holes_device, dsx_fill_holes_ex_device, dsx_postprocess_full_ex_device) or to
 * the handle (dsx_process_pair_device).  The next hole-filling call with the same workspace / handle
 * fails with DSX_EHIP and clears it; so do these queries (DSX_OK when clear).  The march runs
 * asynchronously: the flag is known once the stream has passed that call.
 *   dsx_fill_holes_status_ws      - the workspace's flag
 *   dsx_fill_holes_status_handle  - the handle's flag (dsx_process_pair_device)
 *   dsx_fill_holes_status         - every flag of the process (reports and clears them all) */
int dsx_fill_holes_status_ws(const void *d_workspace);
int dsx_fill_holes_status_handle(dsx_handle *h);
int dsx_fill_holes_status(void);

/* Release the mapped host words (step history, timeout flag) kept for a workspace key: call it
 * before freeing or reusing a hole-filling workspace, so a new buffer at a recycled address does not
 * inherit the old one's flag (its pending flag is returned first, as dsx_fill_holes_status_ws).
 * Handles release theirs in dsx_destroy. */
int dsx_fill_holes_release(const void *d_workspace);

/* Process teardown: wait for every device, then free what the library keeps per process (the mapped
 * host words of every workspace key).  Python registers it with atexit; C callers call it before
 * exit() when no other thread uses the library.  Later calls re-create what they need. */
int dsx_shutdown(void);

/* The per-frame call of the drop-in path, StereoCore._process_pair on the device (stereo_core.py:
 * 162-200): compute_disparity (:165, the matcher with this handle's parameters, float = fixed / 16,
 * :232) -> crop [:, num_disp:] (:168) -> fast mode: 3x3 median (:171-173), or postprocess_disparity
 * (:175-184 -> postprocess.py:120-171: speckles, outliers, optional Telea hole filling, median) ->
 * disparity_to_depth (:186-196, :234-272) when has_depth.  One C-ABI call per frame; the handle owns
 * the float map and the post-processing workspace (no allocation when the size matches).  Per-kernel
 * times go to dsx_kernel_times when params.timing is set. */
#define DSX_POST_FAST 1 /* fast_mode=True:  crop + medianBlur(3)                        */
#define DSX_POST_FULL 2 /* fast_mode=False: crop + postprocess_disparity (the default)   */
#define DSX_FILL_INPAINT 0 /* fill_method 'inpaint': Telea's march (dsx_fill_holes_device)        */
#define DSX_FILL_NEAREST 1 /* fill_method 'nearest': iterated dilation (dsx_fill_nearest_device)  */
typedef struct dsx_post_params {
    double max_diff;           /* 1.0   (stereo_core.py:179)                                        */
    double outlier_threshold;  /* 2.5   (stereo_core.py:180)                                        */
    double focal_length;       /* sgbm_params['focal_length'] (used when has_depth)                 */
    double baseline;           /* sgbm_params['baseline']                                           */
    double doffs;              /* sgbm_params['doffs']                                              */
    double eps;                /* sgbm_params['min_disp'] (stereo_core.py:189: eps = min_disparity) */
    double max_depth;          /* sgbm_params['max_depth'] (used when has_max_depth)               */
    int32_t mode;              /* DSX_POST_FAST | DSX_POST_FULL                                     */
    int32_t max_speckle_size;  /* int(100 * downscale_factor) (stereo_core.py:178)                  */
    int32_t apply_outlier_removal; /* 1 (stereo_core.py:182)                                        */
    int32_t outlier_kernel;    /* 5 (postprocess.py:158 default kernel_size)                        */
    int32_t fill_radius;       /* 0, or 3 with hole_filling=True (postprocess.py:165 fill_kernel 3) */
    int32_t has_depth;         /* focal_length and baseline are set (stereo_core.py:186)            */
    int32_t has_max_depth;
    uint32_t fill_spin_limit;  /* hole filling's persistent-launch spin bound (0: default; tests)    */
    int32_t fill_steps;        /* hole filling's step launches: 0 adaptive, > 0 that many, < 0 none */
    int32_t fill_method;       /* DSX_FILL_INPAINT (0, Telea) | DSX_FILL_NEAREST: fill_radius is then the */
                               /* kernel_size of fill_holes(method='nearest'), 0..31                     */
    int32_t reserved[2];
} dsx_post_params;

/* dL, dR: device uint8 H x W (row stride `stride_bytes`), rectified.  d_out_disp / d_out_depth:
 * contiguous float32 H x (W - num_disp) device buffers (either may be NULL; depth is written only when
 * has_depth).  Needs float_mode DSX_FLOAT_FIXED.  Asynchronous on hip_stream. */
int dsx_process_pair_device(dsx_handle *h, const void *dL, const void *dR, int32_t H, int32_t W,
                            int64_t stride_bytes, const dsx_post_params *pp, void *d_out_disp,
                            void *d_out_depth, void *hip_stream);

/* The stand-alone post-processing chain with its parameters in a dsx_post_params (mode DSX_POST_FULL):
 * what dsx_postprocess_full_ex_device runs, plus fill_method (and fill_spin_limit / fill_steps for the
 * Telea march).  d_out_depth is written only when has_depth.  d_workspace: >=
 * dsx_postprocess_workspace_bytes(H, W, crop); it carries the Telea timeout flag, which 'nearest'
 * neither raises nor consults.  Asynchronous on hip_stream. */
int dsx_postprocess_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t crop,
                           const dsx_post_params *pp, void *d_out_disp, void *d_out_depth, void *d_workspace,
                           size_t workspace_bytes, void *hip_stream);

/* Image-guided refinement of the disparity map: a weighted median whose weights come from the intensity
 * similarity in the left rectified image, with optional filling of invalid pixels from their similar-looking
 * neighbours.  An addition of this build (as the prefilter and the census costs are): parity with nothing
 * outside this repository is claimed.  It gives the `left_image` that StereoCore._process_pair hands to
 * postprocess_disparity (stereo_core.py:175-184) a meaning.  With d the float32 H x W map, G the uint8 H x W
 * guide over the same pixels, r = radius, s = sigma:
 *   validity   a value is valid iff 0 < d < +inf (NaN, +-0, negatives and +inf are invalid);
 *   weights    T[k] = max(1, floor(256 exp(-k / s) + 0.5)), k = 0..255, in doubles on the host
 *              (dsx_wmedian_weights; the device never computes it);
 *   window     |i|, |j| <= r around p, taps outside the image skipped; N = its valid taps q (p included if
 *              valid), w_q = T[|G(p) - G(q)|], S = the sum of the w_q (<= 225 * 256);
 *   output     N empty, or d(p) invalid and fill == 0: out(p) = d(p), the input bits unchanged;
 *              otherwise the smallest v among the d_q with 2 * (sum of w_q over d_q <= v) >= S.
 * The output is always a bit pattern of the window: no arithmetic touches a disparity, so the device equals
 * the host restatement (depthestimation_amd/postprocess.py weighted_median_filter) bit for bit.  One
 * stateless launch: no workspace, no grid barrier, no status flag, nothing to time out.
 * In the chain (mode DSX_POST_FULL) it runs after the hole filling, if any, and before the 3x3 median; with
 * fill = 1 and hole filling off it is the hole filler.  DSX_POST_FAST ignores it, as it ignores hole filling. */
#define DSX_REFINE_NONE 0
#define DSX_REFINE_WMEDIAN 1
typedef struct dsx_refine {
    int32_t type;   /* DSX_REFINE_*                                            */
    int32_t radius; /* 1..7                                                    */
    int32_t sigma;  /* 1..64, in grey levels                                   */
    int32_t fill;   /* 0 | 1: invalid pixels take the median of their window   */
    int32_t reserved[4];
} dsx_refine;

/* none, radius 5, sigma 8, fill 1 */
void dsx_default_refine(dsx_refine *rf);

/* Validate a refinement (host only, no device).  Type NONE passes whatever the other fields hold. */
int dsx_check_refine(const dsx_refine *rf);

/* T for sigma in 1..64 into out256[0..255] (host only). */
int dsx_wmedian_weights(int32_t sigma, uint16_t *out256);

/* The filter alone.  d_disp: float32 H x W, row pitch `in_pitch` elements (any alignment; rows that are 16-byte
 * aligned take 16-byte loads); d_guide: uint8 H x W, row stride guide_stride_bytes (any alignment); rf: type
 * DSX_REFINE_WMEDIAN; d_out: contiguous float32 H x W, not d_disp.  H <= 1048560.  Stateless, asynchronous
 * on hip_stream; argument errors are reported before any HIP call. */
int dsx_wmedian_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, const void *d_guide,
                       int64_t guide_stride_bytes, const dsx_refine *rf, void *d_out, void *hip_stream);

/* dsx_postprocess_device with the refinement between the hole filling and the median.  d_guide: the
 * UNCROPPED uint8 H x W left image, row stride guide_stride_bytes; the chain reads it from column `crop` on.
 * rf NULL or type NONE: exactly dsx_postprocess_device (d_guide may be NULL).  No extra workspace. */
int dsx_postprocess_refine_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, int32_t crop,
                                  const dsx_post_params *pp, void *d_out_disp, void *d_out_depth, void *d_workspace,
                                  size_t workspace_bytes, void *hip_stream, const dsx_refine *rf, const void *d_guide,
                                  int64_t guide_stride_bytes);

/* dsx_process_pair_device with the refinement.  The guide is the caller's dL from column num_disp on: the raw
 * image, also when the handle has a prefilter set.  rf NULL or type NONE: exactly dsx_process_pair_device.
 * Reported under the name refine_wmedian by dsx_kernel_times. */
int dsx_process_pair_refine_device(dsx_handle *h, const void *dL, const void *dR, int32_t H, int32_t W,
                                   int64_t stride_bytes, const dsx_post_params *pp, void *d_out_disp,
                                   void *d_out_depth, void *hip_stream, const dsx_refine *rf);

/* Point-cloud output: a finished disparity map reprojected to metric XYZ, either organized (one point per
 * pixel) or compacted to the list of its valid points in row-major pixel order, with colours and pixel
 * indices.  An addition of this build (as the prefilter, the census costs and the refinement are): parity
 * with nothing outside this repository is claimed.  Stateless calls on a float32 H x W map d whose column 0
 * is image column x0 (the crop: num_disp for the maps of dsx_process_pair_device).  All values float32, every
 * operation correctly rounded, no FMA (host restatement: depthestimation_amd/pointcloud.py, equal bit for
 * bit, the count and the order included):
 *   fB  = (float)((double)focal_length * (double)baseline)      the depth map's own constant
 *   adj = d + doffs;  Z = fB / adj
 *   valid = adj > eps  and  0 < Z < +inf  and  (not has_max_depth or Z <= max_depth)     (NaN: invalid)
 *   s = Z / focal_length;  X = ((float)(x + x0) - cx) * s;  Y = ((float)y - cy) * s
 * Axes as cv2's: x right, y down, z forward.  Points beyond max_depth are dropped, not clamped as the depth
 * map clamps them; a valid point's Z has the depth map's bits wherever that depth is below max_depth.
 * Results in the denormal range are outside the contract. */
typedef struct dsx_cloud {
    double focal_length; /* pixels, > 0: doubles as in dsx_post_params, so that */
    double baseline;     /* metres, finite, != 0: fB is the depth map's own     */
    float cx, cy;      /* principal point in UNCROPPED image coordinates       */
    float doffs;        /* finite                                               */
    float eps;          /* finite (StereoCore passes min_disp)                  */
    float max_depth;    /* > 0 when has_max_depth                               */
    int32_t has_max_depth; /* 0 | 1                                             */
    int32_t x0;         /* >= 0: image column of the map's column 0             */
    int32_t reserved;
} dsx_cloud;

/* Validate a reprojection (host only, no device): focal_length > 0 and finite, baseline finite and != 0,
 * cx / cy / doffs / eps finite, has_max_depth 0 | 1 with max_depth > 0 (not NaN) when set, x0 >= 0. */
int dsx_check_cloud(const dsx_cloud *c);

/* The organized map.  d_disp: float32 H x W, row pitch `in_pitch` elements; d_xyz: contiguous float32
 * H x W x 3, all three components NaN at invalid pixels.  One launch, asynchronous on hip_stream.
 * H == 0 or W == 0: nothing to do.  H * W <= 2^31 - 1, x0 + W <= 2^31 - 1. */
int dsx_reproject_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, const dsx_cloud *c,
                         void *d_xyz, void *hip_stream);

/* Bytes of d_workspace for dsx_point_cloud_device: one int32 per tile of DSX_CLOUD_TILE consecutive pixels
 * (0 for an empty or invalid shape). */
#define DSX_CLOUD_TILE 2048
int64_t dsx_point_cloud_workspace_bytes(int32_t H, int32_t W);

/* The compact cloud: the valid points of d in row-major pixel order.
 *   d_points  float32 cap x 3 (X, Y, Z);  d_colors  uint8 cap x 3 RGB, or NULL;  d_index  int32 cap holding
 *   y * W + x (to gather confidence or anything else per point), or NULL;  d_count  one int32: the number N
 *   of valid points, always the true count - N > cap tells the caller that only the first cap points were
 *   written.  Nothing at or past cap is touched in any output.
 *   d_color  with d_colors: the UNCROPPED uint8 image H x (x0 + W) x channels on the same device, row pitch
 *   color_pitch_bytes (any alignment), read from column x0 on; channels 3: BGR, swapped to RGB; 1: gray,
 *   replicated; 0 (or d_colors NULL): no colours, d_color unused.
 * Three launches on hip_stream - per-tile counts (ballot + popcount), one block's exclusive scan of the tile
 * counts, and a scatter that recomputes the points, ranks them inside the tile (ballot + mbcnt) and writes them
 * into the tile's contiguous output range - with no block waiting on another, no atomics, no host
 * synchronisation.  H == 0 or W == 0 writes count 0 and launches nothing else (d_workspace may be NULL).
 * Argument errors (NULL or short arguments included) are DSX_EINVAL before any HIP call. */
int dsx_point_cloud_device(const void *d_disp, int32_t H, int32_t W, int64_t in_pitch, const dsx_cloud *c,
                           const void *d_color, int64_t color_pitch_bytes, int32_t channels, void *d_points,
                           void *d_colors, void *d_index, int64_t cap, void *d_count, void *d_workspace,
                           int64_t workspace_bytes, void *hip_stream);

/* Temporal disparity filter for video: a motion-gated recursive average with a temporal hole filler.  An
 * addition of this build (as the prefilter, the census costs, the refinement and the point cloud are): parity
 * with nothing outside this repository is claimed.  The one stage here that carries STATE from frame to frame;
 * the state lives in an opaque filter object (dsx_tfilter), not in a matcher handle.
 * Inputs per frame: d, the finished float32 H x W disparity map (what dsx_process_pair_device or the
 * post-processing chain returns; row pitch in elements, any alignment), and G, the uint8 guide over the same
 * pixels (the left rectified image from column num_disp on - the raw image, also when a prefilter is set; row
 * stride in bytes, any alignment).
 * State per pixel: S float32 filtered disparity; n uint8 age (0: no state); h uint8 count of consecutive held
 * frames; P the previous frame's guide.
 * Gains: A[n] = (float)(1.0 / (n + 1)), n = 1..max_age, in doubles on the host (dsx_temporal_gains; the device
 * never computes them).
 * Rule, with r = motion_radius, cx / cy the replicate clamp, all disparity arithmetic float32, every operation
 * correctly rounded, no FMA:
 *   v      = 0 < d < +inf                      (NaN, +-0, negatives and +inf are invalid: the refinement's rule)
 *   M      = sum over |i|, |j| <= r of |G(cx(x+i), cy(y+j)) - P(cx(x+i), cy(y+j))|       (<= 25 * 255)
 *   static = there is a previous frame  and  M <= motion_threshold * (2r + 1)^2
 *   v and static and n > 0 and |d - S| <= max_diff:
 *            S' = S + (d - S) * A[n];  n' = min(n + 1, max_age);  h' = 0;  out = S'
 *   else v:  S' = d;  n' = 1;  h' = 0;  out = d (the input bits)
 *   else static and n > 0 and h < hold:
 *            out = S;  S and n kept;  h' = h + 1                               (the temporal hole filler)
 *   else:    out = d (the input bits unchanged);  S' = 0;  n' = 0;  h' = 0
 *   then P <- G.
 * The first frame, the first frame after a reset and the first frame after a shape change have no previous
 * frame: out = d and the state is initialised from d.  Host restatement: depthestimation_amd/temporal.py,
 * equal bit for bit on every frame. */
#define DSX_TEMPORAL_NONE 0
#define DSX_TEMPORAL_RECURSIVE 1
typedef struct dsx_temporal_params {
    int32_t type;             /* DSX_TEMPORAL_*                                                    */
    int32_t max_age;          /* 1..64 (4): the average covers at most max_age + 1 frames           */
    float max_diff;           /* finite, > 0, pixels (1.0): a larger step restarts the average      */
    int32_t motion_radius;    /* 0..2 (1)                                                          */
    int32_t motion_threshold; /* 0..255 grey levels per tap (6)                                    */
    int32_t hold;             /* 0..255 frames (2): how long a static pixel's hole shows its state  */
    int32_t reserved[6];
} dsx_temporal_params;

/* recursive, max_age 4, max_diff 1.0, radius 1, threshold 6, hold 2 */
void dsx_default_temporal(dsx_temporal_params *t);

/* Validate a parameter set (host only, no device).  Type NONE passes whatever the other fields hold. */
int dsx_check_temporal(const dsx_temporal_params *t);

/* A[1..max_age] into out[1..max_age], out[0] = 0 (host only); out holds max_age + 1 floats.  Returns the
 * count max_age + 1; DSX_EINVAL for max_age outside 1..64 or a NULL array. */
int dsx_temporal_gains(int32_t max_age, float *out);

/* The filter object: it owns the state planes (S, n, h, and two guide planes - the window reads the
 * neighbours' P while the frame's own G becomes the next P, so the guide state is double-buffered and the
 * parity is kept here on the host) and the gain table.  A shape change reallocates and resets; otherwise no
 * call allocates.  Not thread-safe: one caller at a time.
 *   dsx_tfilter_create      type must be DSX_TEMPORAL_RECURSIVE
 *   dsx_tfilter_set_params  waits for the filter's last launch, replaces the set and resets the state; on
 *                           error the filter keeps its old set
 *   dsx_tfilter_reset       the next frame has no previous frame (no device work)
 *   dsx_tfilter_bytes       device bytes held */
typedef struct dsx_tfilter dsx_tfilter;
int dsx_tfilter_create(int device, const dsx_temporal_params *t, dsx_tfilter **out);
int dsx_tfilter_set_params(dsx_tfilter *f, const dsx_temporal_params *t);
int dsx_tfilter_reset(dsx_tfilter *f);
int dsx_tfilter_bytes(dsx_tfilter *f, int64_t *bytes);
int dsx_tfilter_destroy(dsx_tfilter *f);

/* One frame: one launch, asynchronous on hip_stream.  d_disp float32 H x W, row pitch in_pitch elements;
 * d_guide uint8 H x W, row stride guide_stride_bytes; d_out_disp contiguous float32 H x W, which may be d_disp
 * itself when in_pitch == W (every output reads only its own pixel of d).  Rows of d_disp, d_out_disp and
 * d_out_depth that are all 16-byte aligned take 16-byte loads and stores; any other pitch or alignment takes
 * the scalar-per-pixel path.  With d_out_depth non-NULL (contiguous float32 H x W) the same launch writes the
 * depth of out by the depth map's own rule (dsx_postprocess_fast_device: fB = (float)(focal_length * baseline),
 * adj = out + doffs, adj > eps ? fB / adj : +inf, clamped to max_depth when has_max_depth); without it the
 * seven depth scalars are ignored.  H <= 524280.  H == 0 or W == 0: nothing to do.
 * Frames are filtered in the order of the host's calls: a call on a different stream than the previous one is
 * ordered behind the previous call's kernel by a stream wait on an event, with no host wait (as
 * dsx_compute_device orders the users of a handle's scratch), so one filter serves a pipeline that keeps several
 * frames in flight on several streams.  Argument errors are DSX_EINVAL before any HIP call. */
#define DSX_TEMPORAL_TILE_W 256 /* pixels of a row per block: 64 lanes x 4 consecutive pixels */
#define DSX_TEMPORAL_TILE_H 8   /* rows per block                                              */
int dsx_tfilter_run_device(dsx_tfilter *f, const void *d_disp, int32_t H, int32_t W, int64_t in_pitch,
                           const void *d_guide, int64_t guide_stride_bytes, void *d_out_disp, void *d_out_depth,
                           double focal_length, double baseline, double doffs, double eps, double max_depth,
                           int32_t has_max_depth, void *hip_stream);

/* Full-resolution output for downscaled runs: joint bilateral upsampling.  An addition of this build (as the
 * prefilter, the census costs, the refinement, the point cloud and the temporal filter are): parity with nothing
 * outside this repository is claimed.  A run with an input downscale matches at h x Wl pixels; this stage brings
 * its finished map back to the H x W frame the caller holds, guided by that frame, in one stateless launch.
 * Inputs:
 *   d  the finished low-resolution float32 map, h x w, row pitch in elements; its column 0 is low-resolution
 *      image column x0 (the crop: num_disp for the maps of the chain), so x0 + w == Wl;
 *   g  the low-resolution uint8 guide, h x Wl, UNCROPPED, row stride in bytes, any alignment: the raw left image
 *      the matcher ran on, also when a prefilter is set;
 *   G  the full-size uint8 guide, H x W x ch, ch 1 or 3, row stride in bytes, any alignment.  For ch = 3 the
 *      kernel forms the gray value itself, (c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14 in memory order (the
 *      formula of dsx_rectify_device / dsx_resize_area_device); no full-size gray image is written anywhere.
 *   1 <= h <= H, 1 <= Wl <= W, H, W <= 32768.
 * Geometry, per axis with hi-res size I and low-res size O <= I, in integers only:
 *   near(X)    = ((2X + 1) O) div (2 I): the low-res pixel whose cell contains hi-res centre X (<= O - 1);
 *   tap        k = near(X) + t - r, t = 0..2r;  n = |(2X + 1) O - (2k + 1) I|;
 *   tent       a(X, t) = max(0, 64 - ((64 n + (r + 1) I) div (2 (r + 1) I)))      (the centre tap's is > 0);
 *   X0         = max(0, ceil((2 W x0 - Wl) / (2 Wl))): the smallest X with near_x(X) >= x0.
 * The output covers hi-res columns X0 .. W - 1 and all H rows: H x (W - X0), contiguous.  W - X0 <= 0 or w = 0:
 * nothing to do.
 * Per output pixel P = (X, Y), r = radius:
 *   window     y = near_y(Y) + j - r, x = near_x(X) + i - r, j outer and i inner, each 0..2r; taps with y outside
 *              [0, h) or x - x0 outside [0, w) are skipped;
 *   validity   a tap is valid iff 0 < d(y, x - x0) < +inf (the refinement's rule);
 *   weight     W_q = a_x(X, i) a_y(Y, j) T[|G(P) - g(y, x)|] <= 2^20, T the refinement's table
 *              dsx_wmedian_weights(sigma), built on the host;
 *   selection  S = the sum of W_q over the valid taps; m = the smallest valid tap value v with
 *              2 (sum of W_q over d_q <= v) >= S;
 *   average    float32, every operation correctly rounded, no FMA: over the valid taps with |d_q - m| <= max_diff
 *              in window order num <- num + ((float)W_q * d_q); den = the integer sum of their W_q, converted
 *              once; a = num / den (the selected tap itself has W_q >= 1, so den >= 1);
 *   outputs    out_disp(P) = a * sx, sx = (float)((double)W / (double)Wl): full-size pixels;
 *              out_depth(P) = the depth of the UNSCALED a by the depth map's own rule (dsx_postprocess_fast_device:
 *              fB = (float)(focal_length * baseline), adj = a + doffs, adj > eps ? fB / adj : +inf, clamped to
 *              max_depth) - metric depth does not depend on the resolution, so the scalars are the
 *              low-resolution calibration's;
 *   no valid tap: out_disp(P) = the bits of d(near_y(Y), near_x(X) - x0) unchanged - invalid by construction,
 *              unscaled - and the depth rule applied to that value.
 * Host restatement: depthestimation_amd/upsample.py joint_upsample, equal bit for bit. */
#define DSX_UPSAMPLE_NONE 0
#define DSX_UPSAMPLE_JOINT 1
typedef struct dsx_upsample {
    int32_t type;   /* DSX_UPSAMPLE_* (JOINT)                                                   */
    int32_t radius; /* 1..3 (1): the window is (2 radius + 1)^2 low-resolution taps              */
    int32_t sigma;  /* 1..64 grey levels (8)                                                    */
    float max_diff; /* finite, > 0, LOW-RESOLUTION pixels (1.0): the gate of the average around m */
    int32_t reserved[4];
} dsx_upsample;

/* joint, radius 1, sigma 8, max_diff 1.0 */
void dsx_default_upsample(dsx_upsample *u);

/* Validate a parameter set (host only, no device).  Type NONE passes whatever the other fields hold. */
int dsx_check_upsample(const dsx_upsample *u);

/* The integer geometry of one axis (host only): near[X] and tent[X * (2 radius + 1) + t] for X = 0..in_size - 1
 * (in_size the hi-res size I, out_size the low-res size O).  DSX_EINVAL unless 1 <= out_size <= in_size <= 32768,
 * radius in 1..3 and both arrays non-NULL. */
int dsx_upsample_taps(int32_t in_size, int32_t out_size, int32_t radius, int32_t *near, int32_t *tent);

/* X0 of the geometry above (host only); DSX_EINVAL unless 1 <= Wl <= W <= 32768 and 0 <= x0 <= Wl. */
int32_t dsx_upsample_x0(int32_t W, int32_t Wl, int32_t x0);

/* The launch.  d_out_disp / d_out_depth: contiguous float32 H x (W - X0); d_out_depth NULL: no depth, and the
 * seven depth scalars are ignored.  Output rows that are 16-byte aligned (W - X0 a multiple of 4, aligned bases)
 * take 16-byte stores, any other shape the scalar path.  Stateless: one launch, asynchronous on hip_stream, no
 * workspace, no grid barrier, no status flag.  Argument errors are DSX_EINVAL before any HIP call: NULL arguments,
 * Wl > W, h > H, x0 < 0, x0 + w != Wl, pitches or strides too small, channels other than 1 or 3,
 * d_out_disp == d_disp. */
#define DSX_UPSAMPLE_TILE_W 256 /* output pixels of a row per block: 64 lanes x 4 consecutive pixels */
#define DSX_UPSAMPLE_TILE_H 8   /* output rows per block                                             */
int dsx_upsample_device(const void *d_disp, int32_t h, int32_t w, int64_t in_pitch, int32_t x0, const void *d_guide_lo,
                        int32_t Wl, int64_t guide_lo_stride_bytes, const void *d_guide, int32_t H, int32_t W,
                        int32_t channels, int64_t guide_stride_bytes, const dsx_upsample *params, void *d_out_disp,
                        void *d_out_depth, double focal_length, double baseline, double doffs, double eps,
                        double max_depth, int32_t has_max_depth, void *hip_stream);

/* Per-frame rectification on the device, replacing cv2.cvtColor(BGR2GRAY)
 * + cv2.remap(INTER_LINEAR) of rectify.py:183-186 (cached-maps path) and stereo_core.py:155-159:
 * d_img: uint8 Hs x Ws x channels (channels 1 or 3, BGR), row stride `stride_bytes`;
 * d_mapx, d_mapy: float32 H x W maps (initUndistortRectifyMap CV_32FC1 semantics), or both NULL
 *   for the gray conversion alone (then H, W must equal Hs, Ws);
 * d_out: uint8 H x W.  Fixed-point bilinear (1/32 px, 15-bit weights), border 0.  Async. */
int dsx_rectify_device(const void *d_img, int32_t Hs, int32_t Ws, int64_t stride_bytes, int32_t channels,
                       const float *d_mapx, const float *d_mapy, int32_t H, int32_t W, void *d_out,
                       void *hip_stream);

/* The input downscale on the device, replacing cv2.resize(INTER_AREA) of input.py:38-43,63-67 and
 * threaded_stereo.py:45-47 in the arithmetic of this project's host step (input.py resize_area, Pillow's
 * BOX resampling), bit for bit.  Per axis, input size I and output size O <= I:
 *   scale = I / O, fs = max(scale, 1), sup = fs / 2, ss = 1 / fs (doubles);  output o has centre
 *   c = (o + 0.5) scale and the taps x in [int(c - sup + 0.5), int(c + sup + 0.5)) clipped to [0, I) with
 *   -0.5 < (x - c + 0.5) ss <= 0.5: `count` contiguous taps from `start`, coef k = int(2^22 / count + 0.5);
 *   out = min(255, (2^21 + k * sum of the taps) >> 22).
 * The horizontal pass runs first and rounds to uint8, the vertical pass runs on those values; an axis
 * with O == I is the identity.
 *
 * dsx_resize_area_table (host only, no device): fills out_size entries of start / count / coef by the rule
 *   above.  DSX_EINVAL for out_size < 1, out_size > in_size or a NULL array.
 * dsx_resize_area_device: d_img uint8 Hs x Ws x channels (1 or 3), row stride `stride_bytes`; d_out uint8
 *   Ho x Wo x channels with row stride `out_stride_bytes`, or with gray_out = 1 (channels = 3 only)
 *   Ho x Wo gray: (c0 * 1868 + c1 * 9617 + c2 * 4899 + 8192) >> 14 of the rounded uint8 channel values,
 *   the gray formula of dsx_rectify_device (resize, then gray).  1 <= Ho <= Hs, 1 <= Wo <= Ws (no
 *   upscaling), Ho <= 262140.  One launch; integer arithmetic only on the device.  The tables of a
 *   (Hs, Ws, Ho, Wo) are built on the host and kept by the library per device (8 shapes per device, the
 *   least recently used dropped; freed by dsx_shutdown): a shape's first call uploads them on hip_stream
 *   and waits for that copy, later calls allocate nothing and are asynchronous on hip_stream.
 *   Thread-safe; runs on the device that owns d_img.  Argument errors are reported before any HIP call. */
int dsx_resize_area_table(int32_t in_size, int32_t out_size, int32_t *start, int32_t *count, int32_t *coef);
int dsx_resize_area_device(const void *d_img, int32_t Hs, int32_t Ws, int64_t stride_bytes, int32_t channels,
                           int32_t Ho, int32_t Wo, int32_t gray_out, void *d_out, int64_t out_stride_bytes,
                           void *hip_stream);

/* Per-kernel timings accumulated since the last reset (params.timing = 1): names are
 * written as a ';'-separated list into `names` (capacity `names_cap`), average ms per
 * launch into ms[i], launch counts into counts[i]; *n = number of kernels. */
int dsx_kernel_times(dsx_handle *h, char *names, int names_cap, float *ms, int *counts, int cap,
                     int *n);
int dsx_reset_times(dsx_handle *h);

/* Device bytes currently held by the handle's buffer cache: the host-call staging images and
 * outputs, the prefiltered images, the LR keys and left winners, the cost volume, the BT records, the census codes,
 * the SGM sums of either form, the sgbm_post input and workspace, and dsx_process_pair_device's maps and workspace.
 * Buffers kept from an earlier parameter set count until a shape or geometry change frees them. */
int dsx_workspace_bytes(dsx_handle *h, int64_t *bytes);

/* Destroy the matcher and free its device buffers. */
int dsx_destroy(dsx_handle *h);

/* Thread-local message of the last error on this thread ("" if none). */
const char *dsx_last_error(void);

/* ---- single-process multi-GPU collectives ----
 * The frame-sharded video path (StereoDepthEstimatorVideo.py:69-147 fed by
 * ThreadedStereoCapture, threaded_stereo.py:49-80) has one exchange: the calibration block
 * (stereo_core.py:26-37 keys; optionally the rectification maps of rectify.py:49-73) sent
 * once from the root GPU before the first frame.  A process driving several GPUs from
 * threads creates one RCCL communicator per device (ncclCommInitAll) and broadcasts over
 * xGMI.  RCCL is loaded lazily (dlopen), so these are the only entry points that need it. */
typedef struct dsx_comm dsx_comm;

/* One communicator per device in devs[0..ndev) (distinct, visible).  DSX_ECOMM if RCCL is
 * unavailable or ncclCommInitAll fails. */
int dsx_comm_init_all(int ndev, const int *devs, dsx_comm **out);

/* Number of devices in the communicator. */
int dsx_comm_size(dsx_comm *c, int *n);

/* Broadcast `bytes` from dev_bufs[root] into dev_bufs[i] on every device i (device pointers
 * in communicator order).  Synchronous: orders after prior work on each device, returns once
 * every copy has landed. */
int dsx_bcast(dsx_comm *c, void *const *dev_bufs, size_t bytes, int root);

/* Destroy the communicators and their streams (NULL is a no-op). */
int dsx_comm_destroy(dsx_comm *c);

#ifdef __cplusplus
}
#endif
#endif /* DSX_H */
