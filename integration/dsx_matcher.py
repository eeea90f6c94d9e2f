# depthlib/dsx_matcher.py - the reference-side binding of libdsx.so (include/dsx.h).
#
# This is the file a depthlib maintainer drops into the reference as depthlib/dsx_matcher.py
# (option B).  It replaces the object depthlib/stereo_core.py:63-75 builds with
# cv2.StereoSGBM_create and calls at stereo_core.py:231 (matcher.compute(L, R) -> int16 x16), and
# depends on nothing but ctypes, numpy and libdsx.so.  tests/test_integration_stub.py checks its
# struct layout against include/dsx.h (CPU) and its results against the oracle (GPU).
import ctypes
import os

import numpy as np


class _Params(ctypes.Structure):
    # field order and types of dsx_params (include/dsx.h)
    _fields_ = [(n, ctypes.c_int32) for n in (
        "min_disp", "num_disp", "block_size", "cost", "uniqueness_ratio", "disp12_max_diff",
        "subpixel", "float_mode", "path", "timing", "grid_blocks", "aggregation", "p1", "p2",
        "prefilter_cap", "sgbm_post", "speckle_window_size", "speckle_range", "lr_form", "in_flight")] + [("reserved", ctypes.c_int32 * 2)]


class _Prefilter(ctypes.Structure):
    # dsx_prefilter (include/dsx.h)
    _fields_ = [(n, ctypes.c_int32) for n in ("type", "size", "cap", "texture_threshold")] + [
        ("reserved", ctypes.c_int32 * 4)]


class _Confidence(ctypes.Structure):
    # dsx_confidence (include/dsx.h): type DSX_CONF_PEAK_RATIO = 1, threshold 0..255
    _fields_ = [("type", ctypes.c_int32), ("threshold", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]


# preFilterType names -> DSX_PREFILTER_* (this build's own arithmetic, see include/dsx.h)
PREFILTERS = {None: 0, "none": 0, "xsobel": 1, "mean": 2}

# cost names -> DSX_COST_* (the census costs are this build's addition: Hamming distance of 9x7 / 5x5 codes)
COSTS = {"sad": 0, "ssd": 1, "bt": 2, "census9x7": 3, "census5x5": 4}

# sgbm_mode names (stereo_core.py:55-61) -> DSX_AGG_* (semi-global aggregation over SAD costs)
SGBM_MODES = {"sgbm_3way": 3, "hh4": 4, "sgbm": 5, "hh": 8}

_lib = ctypes.CDLL(os.environ.get("DSX_LIB", "libdsx.so"))
_vp, _P = ctypes.c_void_p, ctypes.POINTER(_Params)
_lib.dsx_default_params.argtypes = [_P]
_lib.dsx_default_params.restype = None
_lib.dsx_check_params.argtypes = [_P]
_lib.dsx_create.argtypes = [ctypes.c_int, _P, ctypes.POINTER(_vp)]
_lib.dsx_compute_host.argtypes = [_vp, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _vp, _vp]
_lib.dsx_destroy.argtypes = [_vp]
_lib.dsx_last_error.restype = ctypes.c_char_p
_lib.dsx_set_prefilter.argtypes = [_vp, ctypes.POINTER(_Prefilter)]
_lib.dsx_set_confidence.argtypes = [_vp, ctypes.POINTER(_Confidence)]
_lib.dsx_compute_conf_host.argtypes = [_vp, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _vp, _vp, _vp]


def make_params(minDisparity=0, numDisparities=128, blockSize=5, disp12MaxDiff=1, uniquenessRatio=10,
                cost=0, sgbm_mode=None, P1=0, P2=0, preFilterCap=31):
    # cost: 0 SAD, 1 SSD, 2 BT (OpenCV SGBM's Birchfield-Tomasi pixel cost on the preFilterCap-clipped
    # x-derivative plus intensity), 3 / 4 census 9x7 / 5x5 - or a name of COSTS
    cost = COSTS[cost] if isinstance(cost, str) else cost
    p = _Params()
    _lib.dsx_default_params(ctypes.byref(p))
    p.min_disp, p.num_disp, p.block_size = minDisparity, numDisparities, blockSize
    p.disp12_max_diff, p.uniqueness_ratio, p.cost = disp12MaxDiff, uniquenessRatio, cost
    p.prefilter_cap = preFilterCap
    if sgbm_mode is not None:
        p.aggregation, p.p1, p.p2 = SGBM_MODES[sgbm_mode], P1, P2
    if _lib.dsx_check_params(ctypes.byref(p)) != 0:
        raise ValueError(_lib.dsx_last_error().decode())
    return p


class DsxStereoMatcher:
    """cv2.StereoMatcher-compatible: compute(L, R) -> int16 H x W disparity x16, invalid (min_disp - 1) * 16."""

    def __init__(self, minDisparity=0, numDisparities=128, blockSize=5, disp12MaxDiff=1,
                 uniquenessRatio=10, cost=0, device=0, sgbm_mode=None, P1=0, P2=0, preFilterCap=31,
                 preFilterType=None, preFilterSize=9, textureThreshold=0, confidenceThreshold=0,
                 **_sgbm_only_keys):
        # preFilterType 'xsobel' | 'mean' (cv2.StereoBM's keyword names): both views are filtered on the
        # device before the SAD / SSD search, cap preFilterCap; textureThreshold > 0 needs one
        p = make_params(minDisparity, numDisparities, blockSize, disp12MaxDiff, uniquenessRatio, cost,
                        sgbm_mode, P1, P2, preFilterCap)
        # confidenceThreshold t in 1..255: pixels whose peak-ratio confidence is below t become invalid
        # (this build's addition; the matcher then runs its volume path)
        if isinstance(confidenceThreshold, bool) or int(confidenceThreshold) != confidenceThreshold or \
                not 0 <= confidenceThreshold <= 255:
            raise ValueError("confidenceThreshold must be an integer in [0, 255]")
        self._h = _vp()
        if _lib.dsx_create(device, ctypes.byref(p), ctypes.byref(self._h)) != 0:
            self._h = None
            raise RuntimeError(_lib.dsx_last_error().decode())
        if PREFILTERS[preFilterType] or textureThreshold:
            f = _Prefilter(PREFILTERS[preFilterType], preFilterSize, preFilterCap, textureThreshold)
            if _lib.dsx_set_prefilter(self._h, ctypes.byref(f)) != 0:
                msg = _lib.dsx_last_error().decode()
                _lib.dsx_destroy(self._h)
                self._h = None
                raise ValueError(msg)
        if confidenceThreshold:
            c = _Confidence(1, int(confidenceThreshold))
            if _lib.dsx_set_confidence(self._h, ctypes.byref(c)) != 0:
                msg = _lib.dsx_last_error().decode()
                _lib.dsx_destroy(self._h)
                self._h = None
                raise ValueError(msg)

    def compute_with_confidence(self, left, right):
        """(int16 x16 disparity, uint8 peak-ratio confidence: 255 = no rival, 0 = a tie or outside the band)."""
        L = np.ascontiguousarray(left, np.uint8)
        R = np.ascontiguousarray(right, np.uint8)
        if L.shape != R.shape or L.ndim != 2:
            raise ValueError("left/right must be uint8 H x W of the same size")
        out, conf = np.empty(L.shape, np.int16), np.empty(L.shape, np.uint8)
        if _lib.dsx_compute_conf_host(self._h, L.ctypes.data, R.ctypes.data, L.shape[0], L.shape[1],
                                      L.strides[0], out.ctypes.data, None, conf.ctypes.data) != 0:
            raise RuntimeError(_lib.dsx_last_error().decode())
        return out, conf

    def compute(self, left, right):
        L = np.ascontiguousarray(left, np.uint8)
        R = np.ascontiguousarray(right, np.uint8)
        if L.shape != R.shape or L.ndim != 2:
            raise ValueError("left/right must be uint8 H x W of the same size")
        out = np.empty(L.shape, np.int16)
        if _lib.dsx_compute_host(self._h, L.ctypes.data, R.ctypes.data, L.shape[0], L.shape[1],
                                 L.strides[0], out.ctypes.data, None) != 0:
            raise RuntimeError(_lib.dsx_last_error().decode())
        return out

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.dsx_destroy(self._h)
            self._h = None
