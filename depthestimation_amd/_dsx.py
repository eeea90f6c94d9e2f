"""ctypes binding of libdsx.so (the C-ABI declared in include/dsx.h).

The library is built in-tree (``depthestimation_amd/libdsx.so``, see ``__graft_entry__.build``).
There is no CPU fallback: if the library cannot be loaded, or no HIP device is present when a
matcher is first used, the product raises ``RuntimeError`` (the reference equally fails hard
when cv2's native matcher is unavailable: ``import cv2`` at depthlib/stereo_core.py:1).
"""
from __future__ import annotations

import atexit
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSX_LIB", os.path.join(_HERE, "libdsx.so"))

DSX_OK = 0
DSX_EINVAL = -1
DSX_EHIP = -2
DSX_ECOMM = -3
DSX_ENOMEM = -4

COST = {"sad": 0, "ssd": 1, "bt": 2, "census9x7": 3, "census5x5": 4}  # include/dsx.h DSX_COST_*
CENSUS_WINDOW = {"census9x7": (9, 7), "census5x5": (5, 5)}  # (wx, wy) of the census costs
FLOAT_MODE = {"fixed": 0, "parabola": 1}
PATH = {"fused": 0, "volume": 1}
# SGM path sets by the reference's sgbm_mode names (stereo_core.py:55-61), include/dsx.h DSX_AGG_*
AGGREGATION = {None: 0, "none": 0, "sgbm_3way": 3, "hh4": 4, "sgbm": 5, "hh": 8}

# Every symbol include/dsx.h declares (checked by tests/test_abi.py against the header).
EXPORTS = (
    "dsx_version", "dsx_device_count", "dsx_default_params", "dsx_check_params", "dsx_create",
    "dsx_set_params", "dsx_compute_host", "dsx_compute_device", "dsx_compute_batch_device", "dsx_right_map_device",
    "dsx_postprocess_fast_device", "dsx_postprocess_workspace_bytes", "dsx_postprocess_full_device",
    "dsx_postprocess_full_ex_device", "dsx_fill_holes_workspace_bytes", "dsx_fill_holes_device",
    "dsx_rectify_device", "dsx_fill_holes_status", "dsx_process_pair_device", "dsx_fill_holes_ex_device",
    "dsx_fill_holes_status_ws", "dsx_fill_holes_status_handle", "dsx_fill_holes_release", "dsx_shutdown",
    "dsx_kernel_times", "dsx_reset_times", "dsx_workspace_bytes", "dsx_destroy", "dsx_last_error",
    "dsx_comm_init_all", "dsx_comm_size", "dsx_bcast", "dsx_comm_destroy",
    "dsx_fill_nearest_footprint", "dsx_fill_nearest_workspace_bytes", "dsx_fill_nearest_device",
    "dsx_postprocess_device", "dsx_resize_area_table", "dsx_resize_area_device",
    "dsx_default_prefilter", "dsx_check_prefilter", "dsx_set_prefilter", "dsx_prefilter_device",
    "dsx_texture_sum_device", "dsx_census_device",
    "dsx_default_refine", "dsx_check_refine", "dsx_wmedian_weights", "dsx_wmedian_device",
    "dsx_postprocess_refine_device", "dsx_process_pair_refine_device",
    "dsx_default_confidence", "dsx_check_confidence", "dsx_set_confidence", "dsx_compute_conf_device",
    "dsx_compute_conf_host",
    "dsx_check_cloud", "dsx_reproject_device", "dsx_point_cloud_workspace_bytes", "dsx_point_cloud_device",
    "dsx_default_temporal", "dsx_check_temporal", "dsx_temporal_gains", "dsx_tfilter_create",
    "dsx_tfilter_set_params", "dsx_tfilter_reset", "dsx_tfilter_bytes", "dsx_tfilter_destroy",
    "dsx_tfilter_run_device",
    "dsx_default_upsample", "dsx_check_upsample", "dsx_upsample_taps", "dsx_upsample_x0", "dsx_upsample_device",
    "dsx_block_min8_device",
)


LR_FORM = {"bm": 0, "sgbm": 1}  # DSX_LR_FORM_* (include/dsx.h)


class DsxParams(ctypes.Structure):
    _fields_ = [
        ("min_disp", ctypes.c_int32),
        ("num_disp", ctypes.c_int32),
        ("block_size", ctypes.c_int32),
        ("cost", ctypes.c_int32),
        ("uniqueness_ratio", ctypes.c_int32),
        ("disp12_max_diff", ctypes.c_int32),
        ("subpixel", ctypes.c_int32),
        ("float_mode", ctypes.c_int32),
        ("path", ctypes.c_int32),
        ("timing", ctypes.c_int32),
        ("grid_blocks", ctypes.c_int32),
        ("aggregation", ctypes.c_int32),
        ("p1", ctypes.c_int32),
        ("p2", ctypes.c_int32),
        ("prefilter_cap", ctypes.c_int32),
        ("sgbm_post", ctypes.c_int32),
        ("speckle_window_size", ctypes.c_int32),
        ("speckle_range", ctypes.c_int32),
        ("lr_form", ctypes.c_int32),
        ("in_flight", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 2),
    ]


PREFILTER = {"none": 0, "xsobel": 1, "mean": 2}  # DSX_PREFILTER_* (include/dsx.h)


class DsxPrefilter(ctypes.Structure):
    """dsx_prefilter (include/dsx.h): the matcher prefilter and the texture threshold."""
    _fields_ = [
        ("type", ctypes.c_int32),
        ("size", ctypes.c_int32),
        ("cap", ctypes.c_int32),
        ("texture_threshold", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 4),
    ]


CONFIDENCE = {"peak_ratio": 1}  # DSX_CONF_* (include/dsx.h)


class DsxConfidence(ctypes.Structure):
    """dsx_confidence (include/dsx.h): the matcher's confidence measure and its threshold."""
    _fields_ = [
        ("type", ctypes.c_int32),
        ("threshold", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 6),
    ]


REFINE = {"none": 0, "wmedian": 1}  # DSX_REFINE_* (include/dsx.h)


class DsxRefine(ctypes.Structure):
    """dsx_refine (include/dsx.h): the image-guided weighted median of the post-processing chain."""
    _fields_ = [
        ("type", ctypes.c_int32),
        ("radius", ctypes.c_int32),
        ("sigma", ctypes.c_int32),
        ("fill", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 4),
    ]


CLOUD_TILE = 2048  # DSX_CLOUD_TILE: pixels per block of the point-cloud compaction


class DsxCloud(ctypes.Structure):
    """dsx_cloud (include/dsx.h): the reprojection of a disparity map to XYZ."""
    _fields_ = [
        ("focal_length", ctypes.c_double),
        ("baseline", ctypes.c_double),
        ("cx", ctypes.c_float),
        ("cy", ctypes.c_float),
        ("doffs", ctypes.c_float),
        ("eps", ctypes.c_float),
        ("max_depth", ctypes.c_float),
        ("has_max_depth", ctypes.c_int32),
        ("x0", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


TEMPORAL = {"none": 0, "recursive": 1}  # DSX_TEMPORAL_* (include/dsx.h)
TEMPORAL_TILE = (256, 8)  # (DSX_TEMPORAL_TILE_W, DSX_TEMPORAL_TILE_H): pixels per block of the temporal filter


class DsxTemporalParams(ctypes.Structure):
    """dsx_temporal_params (include/dsx.h): the temporal disparity filter."""
    _fields_ = [
        ("type", ctypes.c_int32),
        ("max_age", ctypes.c_int32),
        ("max_diff", ctypes.c_float),
        ("motion_radius", ctypes.c_int32),
        ("motion_threshold", ctypes.c_int32),
        ("hold", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 6),
    ]


UPSAMPLE = {"none": 0, "joint": 1}  # DSX_UPSAMPLE_* (include/dsx.h)
UPSAMPLE_TILE = (256, 8)  # (DSX_UPSAMPLE_TILE_W, DSX_UPSAMPLE_TILE_H): output pixels per block of the upsampling


class DsxUpsample(ctypes.Structure):
    """dsx_upsample (include/dsx.h): the joint bilateral upsampling of a downscaled run's map."""
    _fields_ = [
        ("type", ctypes.c_int32),
        ("radius", ctypes.c_int32),
        ("sigma", ctypes.c_int32),
        ("max_diff", ctypes.c_float),
        ("reserved", ctypes.c_int32 * 4),
    ]


POST_MODE = {"fast": 1, "full": 2}  # DSX_POST_* (include/dsx.h)
FILL_METHOD = {"inpaint": 0, "nearest": 1}  # DSX_FILL_* (fill_holes' method names, postprocess.py:72-118)
NEAREST_PATH = {"auto": 0, "fused": 1, "stepwise": 2}  # DSX_NEAREST_*
NEAREST_FUSED_MAX = 5  # DSX_NEAREST_FUSED_MAX


class DsxPostParams(ctypes.Structure):
    """dsx_post_params (include/dsx.h): the post-processing of StereoCore._process_pair."""
    _fields_ = [
        ("max_diff", ctypes.c_double),
        ("outlier_threshold", ctypes.c_double),
        ("focal_length", ctypes.c_double),
        ("baseline", ctypes.c_double),
        ("doffs", ctypes.c_double),
        ("eps", ctypes.c_double),
        ("max_depth", ctypes.c_double),
        ("mode", ctypes.c_int32),
        ("max_speckle_size", ctypes.c_int32),
        ("apply_outlier_removal", ctypes.c_int32),
        ("outlier_kernel", ctypes.c_int32),
        ("fill_radius", ctypes.c_int32),
        ("has_depth", ctypes.c_int32),
        ("has_max_depth", ctypes.c_int32),
        ("fill_spin_limit", ctypes.c_uint32),
        ("fill_steps", ctypes.c_int32),
        ("fill_method", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 2),
    ]


class DsxFillOpts(ctypes.Structure):
    """dsx_fill_opts (include/dsx.h): launch shape of the hole-filling march (tests, experiments)."""
    _fields_ = [
        ("spin_limit", ctypes.c_uint32),
        ("steps", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 6),
    ]


_lib = None
_lock = threading.Lock()


def _bind(lib):
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    P = ctypes.POINTER(DsxParams)
    F = ctypes.POINTER(DsxPrefilter)
    RF = ctypes.POINTER(DsxRefine)
    CF = ctypes.POINTER(DsxConfidence)
    PP = ctypes.POINTER(DsxPostParams)
    CL = ctypes.POINTER(DsxCloud)
    TP = ctypes.POINTER(DsxTemporalParams)
    dbl = ctypes.c_double
    UP = ctypes.POINTER(DsxUpsample)
    i32p = ctypes.POINTER(i32)
    sig = {
        "dsx_default_upsample": (None, [UP]),
        "dsx_check_upsample": (ctypes.c_int, [UP]),
        "dsx_upsample_taps": (ctypes.c_int, [i32, i32, i32, i32p, i32p]),
        "dsx_upsample_x0": (i32, [i32, i32, i32]),
        "dsx_upsample_device": (ctypes.c_int, [vp, i32, i32, i64, i32, vp, i32, i64, vp, i32, i32, i32, i64, UP, vp, vp,
                                                dbl, dbl, dbl, dbl, dbl, i32, vp]),
        "dsx_default_temporal": (None, [TP]),
        "dsx_check_temporal": (ctypes.c_int, [TP]),
        "dsx_temporal_gains": (ctypes.c_int, [i32, ctypes.POINTER(ctypes.c_float)]),
        "dsx_tfilter_create": (ctypes.c_int, [ctypes.c_int, TP, ctypes.POINTER(vp)]),
        "dsx_tfilter_set_params": (ctypes.c_int, [vp, TP]),
        "dsx_tfilter_reset": (ctypes.c_int, [vp]),
        "dsx_tfilter_bytes": (ctypes.c_int, [vp, ctypes.POINTER(i64)]),
        "dsx_tfilter_destroy": (ctypes.c_int, [vp]),
        "dsx_tfilter_run_device": (ctypes.c_int, [vp, vp, i32, i32, i64, vp, i64, vp, vp, dbl, dbl, dbl, dbl, dbl, i32,
                                                   vp]),
        "dsx_check_cloud": (ctypes.c_int, [CL]),
        "dsx_reproject_device": (ctypes.c_int, [vp, i32, i32, i64, CL, vp, vp]),
        "dsx_point_cloud_workspace_bytes": (i64, [i32, i32]),
        "dsx_point_cloud_device": (ctypes.c_int, [vp, i32, i32, i64, CL, vp, i64, i32, vp, vp, vp, i64, vp, vp, i64,
                                                   vp]),
        "dsx_default_confidence": (None, [CF]),
        "dsx_check_confidence": (ctypes.c_int, [P, CF]),
        "dsx_set_confidence": (ctypes.c_int, [vp, CF]),
        "dsx_compute_conf_device": (ctypes.c_int, [vp, vp, vp, i32, i32, i64, vp, vp, vp, vp]),
        "dsx_compute_conf_host": (ctypes.c_int, [vp, vp, vp, i32, i32, i64, vp, vp, vp]),
        "dsx_default_refine": (None, [RF]),
        "dsx_check_refine": (ctypes.c_int, [RF]),
        "dsx_wmedian_weights": (ctypes.c_int, [i32, ctypes.POINTER(ctypes.c_uint16)]),
        "dsx_wmedian_device": (ctypes.c_int, [vp, i32, i32, i64, vp, i64, RF, vp, vp]),
        "dsx_postprocess_refine_device": (ctypes.c_int, [vp, i32, i32, i64, i32, PP, vp, vp, vp, ctypes.c_size_t, vp,
                                                          RF, vp, i64]),
        "dsx_process_pair_refine_device": (ctypes.c_int, [vp, vp, vp, i32, i32, i64, PP, vp, vp, vp, RF]),
        "dsx_default_prefilter": (None, [F]),
        "dsx_check_prefilter": (ctypes.c_int, [P, F]),
        "dsx_set_prefilter": (ctypes.c_int, [vp, F]),
        "dsx_prefilter_device": (ctypes.c_int, [vp, i32, i32, i64, F, vp, i64, vp]),
        "dsx_texture_sum_device": (ctypes.c_int, [vp, i32, i32, i64, i32, i32, vp, vp]),
        "dsx_census_device": (ctypes.c_int, [vp, i32, i32, i64, i32, vp, vp]),
        "dsx_block_min8_device": (ctypes.c_int, [vp, i64, vp, vp]),
        "dsx_version": (ctypes.c_int, []),
        "dsx_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
        "dsx_default_params": (None, [P]),
        "dsx_check_params": (ctypes.c_int, [P]),
        "dsx_create": (ctypes.c_int, [ctypes.c_int, P, ctypes.POINTER(vp)]),
        "dsx_set_params": (ctypes.c_int, [vp, P]),
        "dsx_compute_host": (ctypes.c_int, [vp, vp, vp, i32, i32, i64, vp, vp]),
        "dsx_compute_device": (ctypes.c_int, [vp, vp, vp, i32, i32, i64, vp, vp, vp]),
        "dsx_compute_batch_device": (ctypes.c_int, [vp, i32, vp, vp, i64, i32, i32, i64, vp, vp, vp]),
        "dsx_right_map_device": (ctypes.c_int, [vp, vp, vp, i32, i32, i64, vp, vp]),
        "dsx_postprocess_workspace_bytes": (ctypes.c_size_t, [i32, i32, i32]),
        "dsx_postprocess_full_device": (ctypes.c_int, [vp, i32, i32, i64, i32, i32, ctypes.c_double, i32,
                                                        ctypes.c_double, i32, vp, vp, ctypes.c_double,
                                                        ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                                        ctypes.c_double, i32, vp, ctypes.c_size_t, vp]),
        "dsx_postprocess_full_ex_device": (ctypes.c_int, [vp, i32, i32, i64, i32, i32, ctypes.c_double, i32,
                                                           ctypes.c_double, i32, i32, vp, vp, ctypes.c_double,
                                                           ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                                           ctypes.c_double, i32, vp, ctypes.c_size_t, vp]),
        "dsx_fill_holes_workspace_bytes": (ctypes.c_size_t, [i32, i32]),
        "dsx_fill_holes_device": (ctypes.c_int, [vp, i32, i32, i64, i32, vp, vp, ctypes.c_size_t, vp]),
        "dsx_fill_nearest_footprint": (ctypes.c_int, [i32, ctypes.POINTER(ctypes.c_int32), i32]),
        "dsx_fill_nearest_workspace_bytes": (ctypes.c_size_t, [i32, i32]),
        "dsx_fill_nearest_device": (ctypes.c_int, [vp, i32, i32, i64, i32, vp, vp, ctypes.c_size_t, i32, vp]),
        "dsx_postprocess_device": (ctypes.c_int, [vp, i32, i32, i64, i32, ctypes.POINTER(DsxPostParams), vp, vp, vp,
                                                   ctypes.c_size_t, vp]),
        "dsx_rectify_device": (ctypes.c_int, [vp, i32, i32, i64, i32, vp, vp, i32, i32, vp, vp]),
        "dsx_resize_area_table": (ctypes.c_int, [i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        "dsx_resize_area_device": (ctypes.c_int, [vp, i32, i32, i64, i32, i32, i32, i32, vp, i64, vp]),
        "dsx_postprocess_fast_device": (ctypes.c_int, [vp, i32, i32, i64, i32, vp, vp, ctypes.c_double,
                                                        ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                                        ctypes.c_double, i32, vp]),
        "dsx_fill_holes_status": (ctypes.c_int, []),
        "dsx_fill_holes_status_ws": (ctypes.c_int, [vp]),
        "dsx_fill_holes_status_handle": (ctypes.c_int, [vp]),
        "dsx_fill_holes_release": (ctypes.c_int, [vp]),
        "dsx_shutdown": (ctypes.c_int, []),
        "dsx_fill_holes_ex_device": (ctypes.c_int, [vp, i32, i32, i64, i32, vp, vp, ctypes.c_size_t,
                                                     ctypes.POINTER(DsxFillOpts), vp]),
        "dsx_process_pair_device": (ctypes.c_int, [vp, vp, vp, i32, i32, i64, ctypes.POINTER(DsxPostParams), vp, vp,
                                                    vp]),
        "dsx_kernel_times": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                             ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
        "dsx_reset_times": (ctypes.c_int, [vp]),
        "dsx_workspace_bytes": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int64)]),
        "dsx_destroy": (ctypes.c_int, [vp]),
        "dsx_last_error": (ctypes.c_char_p, []),
        "dsx_comm_init_all": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(vp)]),
        "dsx_comm_size": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int)]),
        "dsx_bcast": (ctypes.c_int, [vp, ctypes.POINTER(vp), ctypes.c_size_t, ctypes.c_int]),
        "dsx_comm_destroy": (ctypes.c_int, [vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    return lib


def lib():
    """Load (once) and return the ctypes handle of libdsx.so; RuntimeError if unavailable."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"libdsx.so not found at {LIB_PATH}: build it with "
                        "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback)")
                try:
                    _lib = _bind(ctypes.CDLL(LIB_PATH))
                except OSError as e:  # pragma: no cover - depends on the image
                    raise RuntimeError(f"cannot load {LIB_PATH}: {e}") from e
                # free the per-process mapped host words before the HIP runtime's own exit-time
                # teardown runs (atexit handlers of the interpreter run before the C library's)
                atexit.register(_lib.dsx_shutdown)
    return _lib


def last_error() -> str:
    msg = lib().dsx_last_error()
    return msg.decode() if msg else ""


def check(rc: int, what: str = "dsx") -> None:
    """Map a DSX_E* code onto the reference's error behaviour: ValueError for bad arguments
    (stereo_core.py:106-109 raises ValueError for bad params), RuntimeError otherwise."""
    if rc == DSX_OK:
        return
    msg = f"{what}: {last_error() or 'error ' + str(rc)}"
    if rc == DSX_EINVAL:
        raise ValueError(msg)
    if rc == DSX_ENOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def default_params() -> DsxParams:
    p = DsxParams()
    lib().dsx_default_params(ctypes.byref(p))
    return p


def make_params(min_disp=0, num_disp=128, block_size=5, cost="sad", uniqueness_ratio=10,
                disp12_max_diff=1, subpixel=True, float_mode="fixed", path="fused",
                timing=False, grid_blocks=0, aggregation=None, p1=0, p2=0, prefilter_cap=31,
                sgbm_post=False, speckle_window_size=50, speckle_range=2, lr_form="bm",
                in_flight=False) -> DsxParams:
    p = default_params()
    p.min_disp = int(min_disp)
    p.num_disp = int(num_disp)
    p.block_size = int(block_size)
    if cost not in COST:
        raise ValueError(f"cost must be one of {list(COST)}")
    p.cost = COST[cost]
    p.uniqueness_ratio = int(uniqueness_ratio)
    p.disp12_max_diff = int(disp12_max_diff)
    p.subpixel = int(bool(subpixel))
    if float_mode not in FLOAT_MODE:
        raise ValueError(f"float_mode must be one of {list(FLOAT_MODE)}")
    p.float_mode = FLOAT_MODE[float_mode]
    if path not in PATH:
        raise ValueError(f"path must be one of {list(PATH)}")
    p.path = PATH[path]
    p.timing = int(bool(timing))
    p.grid_blocks = int(grid_blocks)
    if aggregation not in AGGREGATION:
        raise ValueError(f"aggregation must be one of {[k for k in AGGREGATION if k]}")
    p.aggregation = AGGREGATION[aggregation]
    p.p1 = int(p1)
    p.p2 = int(p2)
    p.prefilter_cap = int(prefilter_cap)
    p.sgbm_post = int(bool(sgbm_post))
    p.speckle_window_size = int(speckle_window_size)
    p.speckle_range = int(speckle_range)
    if lr_form not in LR_FORM:
        raise ValueError(f"lr_form must be one of {list(LR_FORM)}")
    p.lr_form = LR_FORM[lr_form]
    p.in_flight = int(bool(in_flight))
    return p


def make_prefilter(prefilter_type="none", prefilter_size=9, prefilter_cap=31, texture_threshold=0) -> DsxPrefilter:
    f = DsxPrefilter()
    lib().dsx_default_prefilter(ctypes.byref(f))
    if prefilter_type not in PREFILTER:
        raise ValueError(f"prefilter_type must be one of {list(PREFILTER)}")
    f.type = PREFILTER[prefilter_type]
    f.size = int(prefilter_size)
    f.cap = int(prefilter_cap)
    f.texture_threshold = int(texture_threshold)
    return f


def make_confidence(confidence_threshold=0) -> DsxConfidence:
    """dsx_confidence from the matcher keyword; ValueError for a non-integer or a value outside [0, 255]."""
    c = DsxConfidence()
    lib().dsx_default_confidence(ctypes.byref(c))
    if isinstance(confidence_threshold, bool) or int(confidence_threshold) != confidence_threshold:
        raise ValueError("confidence_threshold must be an integer in [0, 255]")
    c.threshold = int(confidence_threshold)
    check(lib().dsx_check_confidence(None, ctypes.byref(c)), "dsx_check_confidence")
    return c


def make_refine(refine="none", refine_radius=5, refine_sigma=8, refine_fill=True) -> DsxRefine:
    """dsx_refine from the post-processing keywords; ValueError for an unknown name or a value out of range."""
    rf = DsxRefine()
    lib().dsx_default_refine(ctypes.byref(rf))
    if refine is None:
        refine = "none"
    if refine not in REFINE:
        raise ValueError(f"refine must be one of {list(REFINE)}, got {refine!r}")
    rf.type = REFINE[refine]
    if int(refine_sigma) != refine_sigma:
        raise ValueError("refine_sigma must be an integer in [1, 64]")
    rf.radius = int(refine_radius)
    rf.sigma = int(refine_sigma)
    rf.fill = int(bool(refine_fill))
    check(lib().dsx_check_refine(ctypes.byref(rf)), "dsx_check_refine")
    return rf


def make_cloud(focal_length, baseline, cx, cy, doffs=0.0, eps=1e-6, max_depth=None, x0=0) -> DsxCloud:
    """dsx_cloud from the reprojection keywords; ValueError for a value dsx_check_cloud refuses."""
    if focal_length is None or baseline is None:
        raise ValueError("a point cloud needs focal_length and baseline")
    if isinstance(x0, bool) or int(x0) != x0:
        raise ValueError("x0 must be an integer >= 0")
    c = DsxCloud()
    c.focal_length, c.baseline, c.cx, c.cy = float(focal_length), float(baseline), float(cx), float(cy)
    c.doffs, c.eps = float(doffs or 0.0), float(eps)
    c.max_depth = float(max_depth) if max_depth is not None else 0.0
    c.has_max_depth = int(max_depth is not None)
    c.x0 = int(x0)
    check(lib().dsx_check_cloud(ctypes.byref(c)), "dsx_check_cloud")
    return c


def make_temporal(temporal="recursive", max_age=4, max_diff=1.0, motion_radius=1, motion_threshold=6,
                  hold=2) -> DsxTemporalParams:
    """dsx_temporal_params from the filter's keywords; ValueError for an unknown name or a value
    dsx_check_temporal refuses."""
    t = DsxTemporalParams()
    lib().dsx_default_temporal(ctypes.byref(t))
    if temporal is None:
        temporal = "none"
    if temporal not in TEMPORAL:
        raise ValueError(f"temporal must be one of {list(TEMPORAL)}, got {temporal!r}")
    t.type = TEMPORAL[temporal]
    for name, v in (("max_age", max_age), ("motion_radius", motion_radius), ("motion_threshold", motion_threshold),
                    ("hold", hold)):
        if isinstance(v, bool) or int(v) != v or abs(int(v)) > 1 << 30:
            raise ValueError(f"temporal {name} must be an integer")
        setattr(t, name, int(v))
    try:
        t.max_diff = float(max_diff)
    except (TypeError, ValueError, OverflowError) as e:
        raise ValueError("temporal max_diff must be a finite number > 0") from e
    check(lib().dsx_check_temporal(ctypes.byref(t)), "dsx_check_temporal")
    return t


def make_upsample(upsample="joint", radius=1, sigma=8, max_diff=1.0) -> DsxUpsample:
    """dsx_upsample from the stage's keywords; ValueError for an unknown name or a value dsx_check_upsample
    refuses."""
    u = DsxUpsample()
    lib().dsx_default_upsample(ctypes.byref(u))
    if upsample is None:
        upsample = "none"
    if upsample not in UPSAMPLE:
        raise ValueError(f"upsample must be one of {list(UPSAMPLE)}, got {upsample!r}")
    u.type = UPSAMPLE[upsample]
    for name, v in (("radius", radius), ("sigma", sigma)):
        if isinstance(v, bool) or int(v) != v or abs(int(v)) > 1 << 30:
            raise ValueError(f"upsample {name} must be an integer")
        setattr(u, name, int(v))
    try:
        u.max_diff = float(max_diff)
    except (TypeError, ValueError, OverflowError) as e:
        raise ValueError("upsample max_diff must be a finite number > 0") from e
    check(lib().dsx_check_upsample(ctypes.byref(u)), "dsx_check_upsample")
    return u


def check_prefilter(p, f: DsxPrefilter) -> None:
    """Validate a prefilter against matcher parameters (``p`` None: the filter's own ranges)."""
    check(lib().dsx_check_prefilter(None if p is None else ctypes.byref(p), ctypes.byref(f)), "dsx_check_prefilter")


def check_params(p: DsxParams) -> None:
    check(lib().dsx_check_params(ctypes.byref(p)), "dsx_check_params")


def device_count() -> int:
    n = ctypes.c_int(0)
    check(lib().dsx_device_count(ctypes.byref(n)), "dsx_device_count")
    return n.value
