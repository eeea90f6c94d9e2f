"""HipBlockMatcher: the MI355X replacement for the matcher object the reference builds with
``cv2.StereoSGBM_create`` (depthlib/stereo_core.py:63-75) and calls as
``self.sgbm.compute(rectified_L, rectified_R)`` (stereo_core.py:231).

``compute`` keeps cv2's ``StereoMatcher.compute`` contract: two uint8 H x W arrays of the same
size -> int16 H x W disparity x16 (4 fractional bits), invalid = (min_disp - 1) * 16, so
``StereoCore.compute_disparity``'s ``/ 16.0`` and ``_process_pair``'s crop apply unchanged.
Mismatched inputs raise ValueError (cv2 raises cv2.error there).

Device-resident callers use ``compute_device`` with torch tensors (or raw device pointers) on a
HIP stream; nothing is copied through the host.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _dsx


def _ptr(t):
    """Device pointer of a torch tensor (or an int already)."""
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


def _device_index(t):
    i = t.get_device()  # one call (the per-frame checks below run on every launch)
    return i if i >= 0 else 0


def _fill_method(name) -> int:
    """DSX_FILL_* of fill_holes' method name (postprocess.py:72-118); ValueError for any other."""
    if name not in _dsx.FILL_METHOD:
        raise ValueError(f"fill method must be one of {list(_dsx.FILL_METHOD)}, got {name!r}")
    return _dsx.FILL_METHOD[name]


_DTYPES = {}


def _dt(name):
    """torch dtype object for "torch.<name>" (cached: identity tests instead of str() per call)."""
    d = _DTYPES.get(name)
    if d is None:
        import torch
        d = _DTYPES[name] = getattr(torch, name.split(".")[-1])
    return d


def _check_inputs_on(dev, *ts):
    """Device tensors handed to a handle must live on the handle's GPU (the kernels read them
    through raw pointers on that device)."""
    for t in ts:
        if not t.is_cuda:
            raise ValueError("compute_device needs device tensors (use compute() for host arrays)")
        if _device_index(t) != dev:
            raise ValueError(f"tensor on cuda:{_device_index(t)} but the matcher runs on cuda:{dev}")


def _check_out(t, shape, dtype_name, dev, name):
    """Caller-owned output: a contiguous device tensor of the exact shape and dtype on the handle's
    device (raw int pointers are the caller's responsibility and pass unchecked)."""
    if t is None or isinstance(t, int):
        return
    if not hasattr(t, "data_ptr") or not getattr(t, "is_cuda", False):
        raise ValueError(f"{name} must be a device tensor (or a raw device pointer)")
    if t.dtype is not _dt(dtype_name):
        raise ValueError(f"{name} must be {dtype_name.split('.')[-1]}, got {str(t.dtype).split('.')[-1]}")
    if t.shape != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if _device_index(t) != dev:
        raise ValueError(f"{name} on cuda:{_device_index(t)} but the matcher runs on cuda:{dev}")


class HipBlockMatcher:
    """Block matcher (SAD / SSD / BT / census costs) running on one HIP device (one handle per thread / GPU)."""

    def __init__(self, min_disp=0, num_disp=128, block_size=5, cost="sad", uniqueness_ratio=10,
                 disp12_max_diff=1, subpixel=True, float_mode="fixed", path="fused", device=0,
                 timing=False, grid_blocks=0, aggregation=None, p1=0, p2=0, prefilter_cap=31,
                 sgbm_post=False, speckle_window_size=50, speckle_range=2, lr_form="bm", in_flight=False,
                 prefilter_type="none", prefilter_size=9, texture_threshold=0, confidence_threshold=0):
        """``confidence_threshold`` t in [0, 255] (0: off) invalidates the pixels whose peak-ratio confidence
        (depthestimation_amd/confidence.py; ``compute(..., out_confidence=)`` returns the map) is below t,
        after the LR check.  A matcher with t > 0, and any call that asks for the map, runs the volume path.

        ``prefilter_type`` 'xsobel' | 'mean' filters both views on the device before the search
        (``prefilter_cap`` is its cap, ``prefilter_size`` the window of 'mean'); ``texture_threshold`` > 0
        then invalidates the pixels whose filtered block has less texture (depthestimation_amd/prefilter.py
        restates both).  The defaults ('none', 0) run no extra kernel."""
        self.device = int(device)
        self._params = _dsx.make_params(min_disp, num_disp, block_size, cost, uniqueness_ratio,
                                        disp12_max_diff, subpixel, float_mode, path, timing,
                                        grid_blocks, aggregation, p1, p2, prefilter_cap, sgbm_post,
                                        speckle_window_size, speckle_range, lr_form, in_flight)
        _dsx.check_params(self._params)  # validates on the host, no device needed
        self._prefilter = _dsx.make_prefilter(prefilter_type, prefilter_size, prefilter_cap, texture_threshold)
        _dsx.check_prefilter(self._params, self._prefilter)
        self._confidence = _dsx.make_confidence(confidence_threshold)
        self._h = None
        self._cfg = dict(min_disp=min_disp, num_disp=num_disp, block_size=block_size, cost=cost,
                         uniqueness_ratio=uniqueness_ratio, disp12_max_diff=disp12_max_diff,
                         subpixel=subpixel, float_mode=float_mode, path=path, timing=timing,
                         grid_blocks=grid_blocks, aggregation=aggregation, p1=p1, p2=p2,
                         prefilter_cap=prefilter_cap, sgbm_post=sgbm_post,
                         speckle_window_size=speckle_window_size, speckle_range=speckle_range, lr_form=lr_form,
                         in_flight=in_flight, prefilter_type=prefilter_type, prefilter_size=prefilter_size,
                         texture_threshold=texture_threshold, confidence_threshold=confidence_threshold)

    _CONFIDENCE_DEFAULTS = {"confidence_threshold": 0}
    _PREFILTER_DEFAULTS = {"prefilter_type": "none", "prefilter_size": 9, "texture_threshold": 0}
    _PREFILTER_KEYS = tuple(_PREFILTER_DEFAULTS)

    @classmethod
    def _split_cfg(cls, cfg):
        """(dsx_params, dsx_prefilter) of a configuration dict."""
        base = {k: v for k, v in cfg.items() if k not in cls._PREFILTER_KEYS and k not in cls._CONFIDENCE_DEFAULTS}
        params = _dsx.make_params(**base)
        pre = _dsx.make_prefilter(cfg["prefilter_type"], cfg["prefilter_size"], cfg["prefilter_cap"],
                                  cfg["texture_threshold"])
        return params, pre

    # -- lifetime ---------------------------------------------------------------------------
    def _handle(self):
        if self._h is None:
            L = _dsx.lib()
            n = _dsx.device_count()
            if n == 0:
                raise RuntimeError("HipBlockMatcher: no HIP device visible (the engine has no CPU fallback)")
            h = ctypes.c_void_p()
            _dsx.check(L.dsx_create(self.device, ctypes.byref(self._params), ctypes.byref(h)), "dsx_create")
            if self._prefilter.type != _dsx.PREFILTER["none"]:
                rc = L.dsx_set_prefilter(h, ctypes.byref(self._prefilter))
                if rc != _dsx.DSX_OK:
                    L.dsx_destroy(h)
                    _dsx.check(rc, "dsx_set_prefilter")
            if self._confidence.threshold:
                rc = L.dsx_set_confidence(h, ctypes.byref(self._confidence))
                if rc != _dsx.DSX_OK:
                    L.dsx_destroy(h)
                    _dsx.check(rc, "dsx_set_confidence")
            self._h = h
        return self._h

    def close(self):
        if self._h is not None:
            _dsx.lib().dsx_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - GC timing
        try:
            self.close()
        except Exception:
            pass

    @property
    def params(self) -> dict:
        """The constructor keywords of this matcher.  The prefilter keys are reported once any of them
        is off its default ('none', 9, 0), so a matcher without a prefilter reports the set it always
        did; ``prefilter_params`` reports them always.  ``confidence_threshold`` follows the same rule."""
        cfg = dict(self._cfg)
        if cfg["confidence_threshold"] == self._CONFIDENCE_DEFAULTS["confidence_threshold"]:
            del cfg["confidence_threshold"]
        if all(cfg[k] == d for k, d in self._PREFILTER_DEFAULTS.items()):
            for k in self._PREFILTER_DEFAULTS:
                del cfg[k]
        return cfg

    @property
    def prefilter_params(self) -> dict:
        """{'prefilter_type', 'prefilter_size', 'prefilter_cap', 'texture_threshold'} in effect."""
        return {k: self._cfg[k] for k in ("prefilter_type", "prefilter_size", "prefilter_cap", "texture_threshold")}

    def set_params(self, **kw):
        """Replace parameters of this matcher (dsx_set_params; configure_sgbm -> _build_sgbm,
        stereo_core.py:77-123): ``kw`` is merged into ``params``, validated on the host like the
        constructor does, and handed to the existing handle, which keeps its cached buffers and grows
        them on the next call where needed.  With no handle yet the set is only stored.  Any error
        raises ValueError and leaves the matcher as it was.  ``device`` cannot change."""
        unknown = sorted(set(kw) - set(self._cfg))
        if unknown:
            raise ValueError(f"set_params: unknown parameter(s) {unknown}; known: {sorted(self._cfg)}")
        cfg = dict(self._cfg, **kw)
        try:
            params, pre = self._split_cfg(cfg)
        except (TypeError, OverflowError) as e:
            raise ValueError(f"set_params: {e}") from e
        _dsx.check_params(params)
        _dsx.check_prefilter(params, pre)
        conf = _dsx.make_confidence(cfg["confidence_threshold"])
        if self._h is not None:
            L = _dsx.lib()

            def set_p():
                rc = L.dsx_set_params(self._h, ctypes.byref(params))
                if rc != _dsx.DSX_OK:
                    raise ValueError(f"dsx_set_params: {_dsx.last_error() or 'error ' + str(rc)}")

            def set_f():
                rc = L.dsx_set_prefilter(self._h, ctypes.byref(pre))
                if rc != _dsx.DSX_OK:
                    raise ValueError(f"dsx_set_prefilter: {_dsx.last_error() or 'error ' + str(rc)}")

            # each setter validates against the other's current value, and the pair was validated
            # together above: a filter that goes off leaves first (the new cost may be 'bt'), one that
            # comes on or changes arrives after the parameters it was checked with
            for step in ((set_f, set_p) if pre.type == _dsx.PREFILTER["none"] else (set_p, set_f)):
                step()
            # the confidence set was validated above and depends on no other parameter
            rc = L.dsx_set_confidence(self._h, ctypes.byref(conf))
            if rc != _dsx.DSX_OK:
                raise ValueError(f"dsx_set_confidence: {_dsx.last_error() or 'error ' + str(rc)}")
        self._params, self._prefilter, self._confidence, self._cfg = params, pre, conf, cfg

    # -- cv2.StereoMatcher-style getters (cv2 names used by depthlib docs) --------------------
    def getMinDisparity(self):
        return self._cfg["min_disp"]

    def getNumDisparities(self):
        return self._cfg["num_disp"]

    def getBlockSize(self):
        return self._cfg["block_size"]

    def getUniquenessRatio(self):
        return self._cfg["uniqueness_ratio"]

    def getDisp12MaxDiff(self):
        return self._cfg["disp12_max_diff"]

    # -- compute ----------------------------------------------------------------------------
    @staticmethod
    def _as_gray(a, name):
        a = np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError(f"{name} must be a uint8 H x W (grayscale, rectified) array")
        if a.strides[1] != 1:
            a = np.ascontiguousarray(a)
        return a

    def compute(self, left, right, out_float=None, out_confidence=None):
        """cv2 StereoMatcher.compute contract (stereo_core.py:231): int16 H x W, x16.  ``out_confidence``:
        a contiguous uint8 H x W array that takes the peak-ratio confidence map (dsx_compute_conf_host)."""
        L = self._as_gray(left, "left")
        R = self._as_gray(right, "right")
        if L.shape != R.shape:
            raise ValueError("left and right images must have the same size")
        if L.strides[0] != R.strides[0]:
            L = np.ascontiguousarray(L)
            R = np.ascontiguousarray(R)
        H, W = L.shape
        out = np.empty((H, W), np.int16)
        fptr = None
        if out_float is not None:
            if out_float.shape != (H, W) or out_float.dtype != np.float32 or not out_float.flags.c_contiguous:
                raise ValueError("out_float must be a contiguous float32 H x W array")
            fptr = out_float.ctypes.data
        if out_confidence is not None:
            if not isinstance(out_confidence, np.ndarray) or out_confidence.shape != (H, W) or \
                    out_confidence.dtype != np.uint8 or not out_confidence.flags.c_contiguous:
                raise ValueError("out_confidence must be a contiguous uint8 H x W array")
            rc = _dsx.lib().dsx_compute_conf_host(self._handle(), L.ctypes.data, R.ctypes.data, H, W, L.strides[0],
                                                  out.ctypes.data, fptr, out_confidence.ctypes.data)
            _dsx.check(rc, "dsx_compute_conf_host")
            return out
        rc = _dsx.lib().dsx_compute_host(self._handle(), L.ctypes.data, R.ctypes.data, H, W, L.strides[0],
                                         out.ctypes.data, fptr)
        _dsx.check(rc, "dsx_compute_host")
        return out

    def compute_device(self, left, right, out_fixed=None, out_float=None, stream=None, stride=None,
                       out_confidence=None):
        """Async device compute. ``left``/``right``: uint8 CUDA/HIP tensors (H x W, unit column
        stride) or (ptr, H, W) tuples.  Outputs are caller-owned contiguous device buffers;
        ``out_confidence`` (uint8 H x W) takes the peak-ratio confidence map (dsx_compute_conf_device)."""
        if isinstance(left, tuple):
            lp, H, W = left
            rp = right[0] if isinstance(right, tuple) else _ptr(right)
            st = W if stride is None else stride
        else:
            if left.dtype != right.dtype or left.shape != right.shape or left.dim() != 2:
                raise ValueError("left and right must be uint8 H x W tensors of the same shape")
            ls, rs = left.stride(), right.stride()
            if left.dtype is not _dt("torch.uint8") or ls[1] != 1 or rs[1] != 1 or ls[0] != rs[0]:
                raise ValueError("inputs must be uint8 with unit column stride and equal row strides")
            _check_inputs_on(self.device, left, right)
            H, W = left.shape
            lp, rp, st = left.data_ptr(), right.data_ptr(), ls[0]
        if out_fixed is None and out_float is None and out_confidence is None:
            raise ValueError("at least one of out_fixed / out_float is required")
        _check_out(out_fixed, (H, W), "torch.int16", self.device, "out_fixed")
        _check_out(out_float, (H, W), "torch.float32", self.device, "out_float")
        _check_out(out_confidence, (H, W), "torch.uint8", self.device, "out_confidence")
        if stream is None:
            sptr = None
        elif isinstance(stream, int):
            sptr = stream
        else:
            sptr = stream.cuda_stream
        if out_confidence is not None:
            rc = _dsx.lib().dsx_compute_conf_device(self._handle(), lp, rp, H, W, st, _ptr(out_fixed), _ptr(out_float),
                                                    _ptr(out_confidence), sptr)
            _dsx.check(rc, "dsx_compute_conf_device")
            return
        rc = _dsx.lib().dsx_compute_device(self._handle(), lp, rp, H, W, st, _ptr(out_fixed), _ptr(out_float), sptr)
        _dsx.check(rc, "dsx_compute_device")

    def compute_batch_device(self, left, right, out_fixed=None, out_float=None, stream=None):
        """One launch over N frame pairs: ``left``/``right`` uint8 HIP tensors N x H x W (unit
        column stride, equal strides); outputs contiguous N x H x W.  Equals N compute_device calls."""
        if left.dim() != 3 or left.shape != right.shape or left.stride() != right.stride():
            raise ValueError("left and right must be N x H x W tensors of the same shape and strides")
        if str(left.dtype) != "torch.uint8" or str(right.dtype) != "torch.uint8" or left.stride(2) != 1:
            raise ValueError("inputs must be uint8 device tensors with unit column stride")
        _check_inputs_on(self.device, left, right)
        N, H, W = left.shape
        if out_fixed is None and out_float is None:
            raise ValueError("at least one of out_fixed / out_float is required")
        _check_out(out_fixed, (N, H, W), "torch.int16", self.device, "out_fixed")
        _check_out(out_float, (N, H, W), "torch.float32", self.device, "out_float")
        sptr = None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
        rc = _dsx.lib().dsx_compute_batch_device(self._handle(), N, left.data_ptr(), right.data_ptr(), left.stride(0),
                                                 H, W, left.stride(1), _ptr(out_fixed), _ptr(out_float), sptr)
        _dsx.check(rc, "dsx_compute_batch_device")

    def process_pair_device(self, left, right, fast_mode=False, max_speckle_size=100, max_diff=1.0,
                            apply_outlier_removal=True, outlier_threshold=2.5, outlier_kernel=5, fill_radius=0,
                            focal_length=None, baseline=None, doffs=0.0, eps=1e-6, max_depth=None, out_disp=None,
                            out_depth=None, stream=None, fill_spin_limit=0, fill_steps=0, fill_method="inpaint",
                            refine="none", refine_radius=5, refine_sigma=8, refine_fill=True):
        """StereoCore._process_pair (stereo_core.py:162-200) in ONE C-ABI call
        (dsx_process_pair_device): matcher -> crop [:, num_disp:] -> fast-mode median or
        postprocess_disparity (speckles, outliers, hole filling when ``fill_radius`` > 0: Telea with
        ``fill_method`` 'inpaint', the iterated dilation with 'nearest', where ``fill_radius`` is the
        kernel_size; median) -> depth when focal length and baseline are given.  ``left``/``right``: uint8 HIP
        tensors H x W (unit column stride, equal row strides).  Returns float32 HIP tensors
        (disparity H x (W - num_disp), depth or None); asynchronous on ``stream``.

        ``refine`` 'wmedian' (dsx_process_pair_refine_device) runs the image-guided weighted median
        (postprocess.weighted_median_filter; ``refine_radius`` 1..7, ``refine_sigma`` 1..64, ``refine_fill``)
        after the hole filling and before the median, guided by the raw ``left`` from column num_disp on;
        fast mode ignores it.  Per call, like every other post parameter."""
        import torch
        rf = _dsx.make_refine(refine, refine_radius, refine_sigma, refine_fill)
        if left.dtype != right.dtype or left.shape != right.shape or left.dim() != 2:
            raise ValueError("left and right must be uint8 H x W tensors of the same shape")
        if str(left.dtype) != "torch.uint8" or left.stride(1) != 1 or right.stride(1) != 1 or \
                left.stride(0) != right.stride(0):
            raise ValueError("inputs must be uint8 with unit column stride and equal row strides")
        _check_inputs_on(self.device, left, right)
        H, W = left.shape
        Wc = max(W - int(self._cfg["num_disp"]), 0)
        want_depth = focal_length is not None and baseline is not None
        if out_disp is None:
            out_disp = torch.empty((H, Wc), dtype=torch.float32, device=left.device)
        if want_depth and out_depth is None:
            out_depth = torch.empty((H, Wc), dtype=torch.float32, device=left.device)
        _check_out(out_disp, (H, Wc), "torch.float32", self.device, "out_disp")
        if want_depth:
            _check_out(out_depth, (H, Wc), "torch.float32", self.device, "out_depth")
        pp = _dsx.DsxPostParams()
        pp.mode = _dsx.POST_MODE["fast" if fast_mode else "full"]
        pp.max_speckle_size = int(max_speckle_size)
        pp.max_diff = float(max_diff)
        pp.apply_outlier_removal = int(bool(apply_outlier_removal))
        pp.outlier_threshold = float(outlier_threshold)
        pp.outlier_kernel = int(outlier_kernel)
        pp.fill_radius = int(fill_radius)
        pp.has_depth = int(want_depth)
        pp.focal_length = float(focal_length or 0.0)
        pp.baseline = float(baseline or 0.0)
        pp.doffs = float(doffs or 0.0)
        pp.eps = float(eps)
        pp.max_depth = float(max_depth or 0.0)
        pp.has_max_depth = int(max_depth is not None)
        pp.fill_spin_limit = int(fill_spin_limit)
        pp.fill_steps = int(fill_steps)
        pp.fill_method = _fill_method(fill_method)
        sptr = None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
        if rf.type:
            rc = _dsx.lib().dsx_process_pair_refine_device(self._handle(), left.data_ptr(), right.data_ptr(), H, W,
                                                           left.stride(0), ctypes.byref(pp), _ptr(out_disp),
                                                           _ptr(out_depth) if want_depth else None, sptr,
                                                           ctypes.byref(rf))
            _dsx.check(rc, "dsx_process_pair_refine_device")
            return out_disp, (out_depth if want_depth else None)
        rc = _dsx.lib().dsx_process_pair_device(self._handle(), left.data_ptr(), right.data_ptr(), H, W,
                                                left.stride(0), ctypes.byref(pp), _ptr(out_disp),
                                                _ptr(out_depth) if want_depth else None, sptr)
        _dsx.check(rc, "dsx_process_pair_device")
        return out_disp, (out_depth if want_depth else None)

    def fill_status(self):
        """Raise RuntimeError if this handle's hole filling (process_pair_device with fill_radius > 0)
        timed out since the last check (dsx_fill_holes_status_handle): that frame's holes were left
        unfilled.  Call it once the stream has passed the frame; the condition is cleared."""
        if self._h is not None:
            _dsx.check(_dsx.lib().dsx_fill_holes_status_handle(self._h), "hole filling")

    def right_map_device(self, left, right, out_dR, stream=None):
        """Right-view winner map dR (int16 H x W, -1 where the search range is empty)."""
        if left.dim() != 2 or left.shape != right.shape or left.stride(0) != right.stride(0):
            raise ValueError("left and right must be H x W tensors of the same shape and row stride")
        if str(left.dtype) != "torch.uint8" or str(right.dtype) != "torch.uint8" or left.stride(1) != 1 \
                or right.stride(1) != 1:
            raise ValueError("inputs must be uint8 with unit column stride")
        _check_inputs_on(self.device, left, right)
        H, W = left.shape
        _check_out(out_dR, (H, W), "torch.int16", self.device, "out_dR")
        if out_dR is None:
            raise ValueError("out_dR is required")
        sptr = None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
        rc = _dsx.lib().dsx_right_map_device(self._handle(), left.data_ptr(), right.data_ptr(), H, W,
                                             left.stride(0), _ptr(out_dR), sptr)
        _dsx.check(rc, "dsx_right_map_device")

    # -- timing -----------------------------------------------------------------------------
    def kernel_times(self) -> dict:
        """{kernel name: (avg ms per launch, launches)} recorded with HIP events (timing=True)."""
        cap = 16
        names = ctypes.create_string_buffer(1024)
        ms = (ctypes.c_float * cap)()
        cnt = (ctypes.c_int * cap)()
        n = ctypes.c_int(0)
        rc = _dsx.lib().dsx_kernel_times(self._handle(), names, 1024, ms, cnt, cap, ctypes.byref(n))
        _dsx.check(rc, "dsx_kernel_times")
        keys = names.value.decode().split(";") if n.value else []
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(keys[:cap])}

    def reset_times(self):
        _dsx.check(_dsx.lib().dsx_reset_times(self._handle()), "dsx_reset_times")

    def workspace_bytes(self) -> int:
        b = ctypes.c_int64(0)
        _dsx.check(_dsx.lib().dsx_workspace_bytes(self._handle(), ctypes.byref(b)), "dsx_workspace_bytes")
        return b.value


def postprocess_fast_device(disp, crop, focal_length=None, baseline=None, doffs=0.0, eps=1e-6, max_depth=None,
                            out_disp=None, out_depth=None, stream=None):
    """Fast-mode epilogue on the device (dsx_postprocess_fast_device; stereo_core.py:168-196):
    crop ``[:, crop:]`` -> 3x3 median (cv2.medianBlur semantics) -> depth when focal length and
    baseline are given.  ``disp``: float32 H x W HIP tensor (unit column stride).  Returns
    (disp_cropped, depth or None) as HIP tensors."""
    import torch

    if disp.dtype != torch.float32 or disp.dim() != 2 or disp.stride(1) != 1 or not disp.is_cuda:
        raise ValueError("disp must be a float32 H x W device tensor with unit column stride")
    H, W = disp.shape
    Wc = max(W - int(crop), 0)
    if out_disp is None:
        out_disp = torch.empty((H, Wc), dtype=torch.float32, device=disp.device)
    want_depth = focal_length is not None and baseline is not None
    if want_depth and out_depth is None:
        out_depth = torch.empty((H, Wc), dtype=torch.float32, device=disp.device)
    sptr = None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
    rc = _dsx.lib().dsx_postprocess_fast_device(
        disp.data_ptr(), H, W, disp.stride(0), int(crop), _ptr(out_disp) if Wc else None,
        _ptr(out_depth) if (want_depth and Wc) else None, float(focal_length or 0.0), float(baseline or 0.0),
        float(doffs or 0.0), float(eps), float(max_depth or 0.0), int(max_depth is not None), sptr)
    _dsx.check(rc, "dsx_postprocess_fast_device")
    return out_disp, (out_depth if want_depth else None)


def prefilter_device(img, prefilter_type="xsobel", prefilter_size=9, prefilter_cap=31, out=None, stream=None):
    """The matcher prefilter alone on the device (dsx_prefilter_device; host restatement
    depthestimation_amd/prefilter.py): ``img`` uint8 H x W HIP tensor (unit column stride, any row stride
    or offset) -> uint8 H x W in [0, 2 * prefilter_cap]."""
    import torch

    if img.dtype != torch.uint8 or img.dim() != 2 or not img.is_cuda or img.stride(1) != 1:
        raise ValueError("img must be a uint8 H x W device tensor with unit column stride")
    f = _dsx.make_prefilter(prefilter_type, prefilter_size, prefilter_cap, 0)
    H, W = img.shape
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=img.device)
    elif out.dtype != torch.uint8 or out.shape != (H, W) or out.stride(1) != 1 or out.device != img.device:
        raise ValueError("out must be a uint8 H x W tensor with unit column stride on the input's device")
    if H == 0 or W == 0:
        return out
    rc = _dsx.lib().dsx_prefilter_device(img.data_ptr(), H, W, img.stride(0), ctypes.byref(f), out.data_ptr(),
                                         out.stride(0), _stream_ptr(stream))
    _dsx.check(rc, "dsx_prefilter_device")
    return out


def census_device(img, cost="census9x7", out=None, stream=None):
    """The census transform alone on the device (dsx_census_device; host restatement
    depthestimation_amd/census.py ``census_transform``): ``img`` uint8 H x W HIP tensor (unit column stride,
    any row stride or offset) -> int64 H x W codes of the window ``cost`` names ('census9x7': 62 bits,
    'census5x5': 24 bits)."""
    import torch

    if cost not in _dsx.CENSUS_WINDOW:
        raise ValueError(f"cost must be one of {list(_dsx.CENSUS_WINDOW)}, got {cost!r}")
    if img.dtype != torch.uint8 or img.dim() != 2 or not img.is_cuda or img.stride(1) != 1:
        raise ValueError("img must be a uint8 H x W device tensor with unit column stride")
    H, W = img.shape
    if out is None:
        out = torch.empty((H, W), dtype=torch.int64, device=img.device)
    elif out.dtype != torch.int64 or out.shape != (H, W) or not out.is_contiguous() or out.device != img.device:
        raise ValueError("out must be a contiguous int64 H x W tensor on the input's device")
    if H == 0 or W == 0:
        return out
    rc = _dsx.lib().dsx_census_device(img.data_ptr(), H, W, img.stride(0), _dsx.COST[cost], out.data_ptr(),
                                      _stream_ptr(stream))
    _dsx.check(rc, "dsx_census_device")
    return out


def texture_sum_device(pref, block_size, cap=31, stream=None):
    """T of a prefiltered image on the device (dsx_texture_sum_device): the block_size x block_size sum
    of |P - cap| with clamped coordinates, int32 H x W HIP tensor (the kernel's uint16 values)."""
    import torch

    if pref.dtype != torch.uint8 or pref.dim() != 2 or not pref.is_cuda or pref.stride(1) != 1:
        raise ValueError("pref must be a uint8 H x W device tensor with unit column stride")
    H, W = pref.shape
    out = torch.empty((H, W), dtype=torch.int16, device=pref.device)
    if H and W:
        rc = _dsx.lib().dsx_texture_sum_device(pref.data_ptr(), H, W, pref.stride(0), int(block_size), int(cap),
                                               out.data_ptr(), _stream_ptr(stream))
        _dsx.check(rc, "dsx_texture_sum_device")
    if stream is None:
        return out.to(torch.int32) & 0xFFFF
    st = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=pref.device)
    with torch.cuda.stream(st):  # the widening follows the kernel on its stream
        return out.to(torch.int32) & 0xFFFF


def rectify_device(img, mapx=None, mapy=None, out=None, stream=None):
    """BGR->gray fused with the fixed-point bilinear remap on the device (dsx_rectify_device;
    rectify.py:183-186 + stereo_core.py:155-159).  ``img``: uint8 H x W x 3 (BGR) or H x W HIP
    tensor; ``mapx``/``mapy``: float32 HIP maps (None: gray conversion only).  Returns uint8."""
    import torch

    if img.dtype != torch.uint8 or not img.is_cuda or img.dim() not in (2, 3):
        raise ValueError("img must be a uint8 H x W (x 3) device tensor")
    ch = 1 if img.dim() == 2 else img.shape[2]
    if ch not in (1, 3) or img.stride(-1) != 1 or (ch == 3 and img.stride(1) != 3):
        raise ValueError("img must be gray or packed 3-channel with unit element stride")
    Hs, Ws = img.shape[0], img.shape[1]
    if mapx is None:
        if ch == 1:
            return img if out is None else out.copy_(img)
        H, W = Hs, Ws
    else:
        if mapx.dtype != torch.float32 or mapx.shape != mapy.shape or not mapx.is_contiguous() or not mapy.is_contiguous():
            raise ValueError("maps must be contiguous float32 tensors of the same shape")
        H, W = mapx.shape
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=img.device)
    sptr = None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
    rc = _dsx.lib().dsx_rectify_device(img.data_ptr(), Hs, Ws, img.stride(0), ch,
                                       None if mapx is None else mapx.data_ptr(),
                                       None if mapy is None else mapy.data_ptr(), H, W, out.data_ptr(), sptr)
    _dsx.check(rc, "dsx_rectify_device")
    return out


def _keep_until_done(t, stream):
    """A workspace tensor dropped when the call returns is handed back to torch's caching
    allocator at once; when the kernels run on another stream than torch's current one, mark it
    used there so the block is not reused before they finish."""
    import torch
    if stream is None:
        return
    st = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=t.device)
    if st.cuda_stream != torch.cuda.current_stream(t.device).cuda_stream:
        t.record_stream(st)


def postprocess_full_device(disp, crop, max_speckle_size=50, max_diff=1.0, apply_outlier_removal=True,
                            outlier_threshold=3.0, outlier_kernel=5, focal_length=None, baseline=None, doffs=0.0,
                            eps=1e-6, max_depth=None, stream=None, apply_hole_filling=False, fill_kernel=3,
                            workspace=None, fill_method="inpaint", guide=None, refine="none", refine_radius=5,
                            refine_sigma=8, refine_fill=True):
    """postprocess_disparity (postprocess.py:120-171) + depth on the device
    (dsx_postprocess_device): speckles -> outliers -> hole filling when
    ``apply_hole_filling`` (``fill_method`` 'inpaint': Telea with radius ``fill_kernel``; 'nearest':
    ``fill_kernel`` masked dilations, stateless) -> 3x3 median -> depth, all enqueued on ``stream``
    without host synchronisation.  ``disp``: float32 H x W HIP tensor.
    Returns (disp_cropped, depth or None) as HIP tensors.  ``workspace``: a ``FillWorkspace`` (default:
    one per device and stream), whose flag ``fill_holes_status(workspace)`` reports a timed-out fill.

    ``refine`` 'wmedian' (dsx_postprocess_refine_device): the image-guided weighted median between the hole
    filling and the median, with ``guide`` the UNCROPPED uint8 H x W left image on ``disp``'s device (unit
    column stride; read from column ``crop`` on)."""
    import torch

    method = _fill_method(fill_method)
    rf = _dsx.make_refine(refine, refine_radius, refine_sigma, refine_fill)
    if rf.type:
        if guide is None:
            raise ValueError("refine needs guide (the uncropped left image on the device)")
        if guide.dtype != torch.uint8 or guide.dim() != 2 or guide.stride(1) != 1 or guide.device != disp.device \
                or guide.shape != disp.shape:
            raise ValueError("guide must be a uint8 device tensor of disp's shape with unit column stride")
    if disp.dtype != torch.float32 or disp.dim() != 2 or disp.stride(1) != 1 or not disp.is_cuda:
        raise ValueError("disp must be a float32 H x W device tensor with unit column stride")
    H, W = disp.shape
    Wc = max(W - int(crop), 0)
    out_disp = torch.empty((H, Wc), dtype=torch.float32, device=disp.device)
    want_depth = focal_length is not None and baseline is not None
    out_depth = torch.empty((H, Wc), dtype=torch.float32, device=disp.device) if want_depth else None
    if Wc == 0:
        return out_disp, out_depth
    L = _dsx.lib()
    nbytes = L.dsx_postprocess_workspace_bytes(H, W, int(crop))
    wsobj = workspace if workspace is not None else default_workspace(disp.device, stream, "post")
    ws = wsobj.get(nbytes, disp.device, stream)
    sptr = _stream_ptr(stream)
    pp = _dsx.DsxPostParams()
    pp.mode = _dsx.POST_MODE["full"]
    pp.max_speckle_size = int(max_speckle_size)
    pp.max_diff = float(max_diff)
    pp.apply_outlier_removal = int(bool(apply_outlier_removal))
    pp.outlier_threshold = float(outlier_threshold)
    pp.outlier_kernel = int(outlier_kernel)
    pp.fill_radius = int(fill_kernel) if apply_hole_filling else 0
    pp.fill_method = method
    pp.has_depth = int(want_depth)
    pp.focal_length = float(focal_length or 0.0)
    pp.baseline = float(baseline or 0.0)
    pp.doffs = float(doffs or 0.0)
    pp.eps = float(eps)
    pp.max_depth = float(max_depth or 0.0)
    pp.has_max_depth = int(max_depth is not None)
    if rf.type:
        rc = L.dsx_postprocess_refine_device(disp.data_ptr(), H, W, disp.stride(0), int(crop), ctypes.byref(pp),
                                             out_disp.data_ptr(), out_depth.data_ptr() if want_depth else None,
                                             ws.data_ptr(), nbytes, sptr, ctypes.byref(rf), guide.data_ptr(),
                                             guide.stride(0))
        _dsx.check(rc, "dsx_postprocess_refine_device")
    else:
        rc = L.dsx_postprocess_device(disp.data_ptr(), H, W, disp.stride(0), int(crop), ctypes.byref(pp),
                                      out_disp.data_ptr(), out_depth.data_ptr() if want_depth else None,
                                      ws.data_ptr(), nbytes, sptr)
        _dsx.check(rc, "dsx_postprocess_device")
    _keep_until_done(ws, stream)
    return out_disp, out_depth


def wmedian_device(disp, guide, radius=5, sigma=8, fill=True, out=None, stream=None):
    """The image-guided weighted median alone on the device (dsx_wmedian_device; host restatement
    postprocess.weighted_median_filter, equal bit for bit).  ``disp``: float32 H x W HIP tensor, ``guide``:
    uint8 H x W HIP tensor (both unit column stride, any row stride or offset); ``out`` must not be
    ``disp``.  Stateless, asynchronous on ``stream``; returns the contiguous float32 H x W result."""
    import torch

    if disp.dtype != torch.float32 or disp.dim() != 2 or disp.stride(1) != 1 or not disp.is_cuda:
        raise ValueError("disp must be a float32 H x W device tensor with unit column stride")
    if guide is None:
        raise ValueError("guide is required (a uint8 H x W device tensor)")
    if guide.dtype != torch.uint8 or guide.shape != disp.shape or guide.device != disp.device or \
            (guide.dim() == 2 and guide.shape[1] > 1 and guide.stride(1) != 1):
        raise ValueError("guide must be a uint8 tensor of disp's shape on its device with unit column stride")
    rf = _dsx.make_refine("wmedian", radius, sigma, fill)
    H, W = disp.shape
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=disp.device)
    elif out is disp or (hasattr(out, "data_ptr") and H and W and out.data_ptr() == disp.data_ptr()):
        raise ValueError("out must not be disp (every window reads its neighbours' inputs)")
    elif out.shape != (H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != disp.device:
        raise ValueError("out must be a contiguous float32 H x W tensor on the input's device")
    if H == 0 or W == 0:
        return out
    rc = _dsx.lib().dsx_wmedian_device(disp.data_ptr(), H, W, max(disp.stride(0), W), guide.data_ptr(),
                                       max(guide.stride(0), W), ctypes.byref(rf), out.data_ptr(), _stream_ptr(stream))
    _dsx.check(rc, "dsx_wmedian_device")
    return out


def _cloud_args(disp, focal_length, baseline, principal_point, doffs, eps, max_depth, x0):
    """The checks the two point-cloud calls share: (H, W, dsx_cloud)."""
    import torch

    if not hasattr(disp, "dtype") or disp.dtype != torch.float32 or disp.dim() != 2 or not disp.is_cuda or \
            (disp.shape[1] > 1 and disp.stride(1) != 1):
        raise ValueError("disp must be a float32 H x W device tensor with unit column stride")
    H, W = disp.shape
    if isinstance(x0, bool) or int(x0) != x0 or int(x0) < 0:
        raise ValueError("x0 must be an integer >= 0")
    if principal_point is None:
        cx, cy = (int(x0) + W - 1) / 2.0, (H - 1) / 2.0  # the centre of the uncropped image
    else:
        cx, cy = principal_point
    return H, W, _dsx.make_cloud(focal_length, baseline, cx, cy, doffs, eps, max_depth, x0)


def reproject_device(disp, focal_length, baseline, principal_point=None, doffs=0.0, eps=1e-6, max_depth=None, x0=0,
                     out=None, stream=None):
    """The organized cloud on the device (dsx_reproject_device; host restatement
    pointcloud.reproject_disparity, equal bit for bit): float32 H x W disparity tensor (unit column stride, any
    row stride) whose column 0 is image column ``x0`` -> contiguous float32 H x W x 3, NaN at invalid pixels.
    ``principal_point``: (cx, cy) in uncropped image coordinates, None for the image centre.  One launch,
    asynchronous on ``stream``."""
    import torch

    H, W, c = _cloud_args(disp, focal_length, baseline, principal_point, doffs, eps, max_depth, x0)
    if out is None:
        out = torch.empty((H, W, 3), dtype=torch.float32, device=disp.device)
    elif out.shape != (H, W, 3) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != disp.device:
        raise ValueError("out must be a contiguous float32 H x W x 3 tensor on the input's device")
    if H == 0 or W == 0:
        return out
    rc = _dsx.lib().dsx_reproject_device(disp.data_ptr(), H, W, max(disp.stride(0), W), ctypes.byref(c),
                                         out.data_ptr(), _stream_ptr(stream))
    _dsx.check(rc, "dsx_reproject_device")
    return out


def point_cloud_device(disp, focal_length, baseline, principal_point=None, doffs=0.0, eps=1e-6, max_depth=None, x0=0,
                       colors=None, capacity=None, out_points=None, out_colors=None, out_index=None, stream=None,
                       sync=True):
    """The compact cloud on the device (dsx_point_cloud_device; host restatement pointcloud.point_cloud, equal
    bit for bit, count and order included): the valid points of ``disp`` in row-major pixel order.

    ``disp``: float32 H x W HIP tensor (unit column stride, any row stride) whose column 0 is image column
    ``x0``.  ``colors``: the UNCROPPED uint8 image on the same device, H x (x0 + W) x 3 BGR or H x (x0 + W) gray
    (packed pixels, any row stride or offset), read from column ``x0`` on; None: no colours.  ``capacity``: room
    in the outputs, in points (None: H * W); ``out_points`` (float32 capacity x 3), ``out_colors`` (uint8
    capacity x 3) and ``out_index`` (int32 capacity) may be the caller's; ``out_index=False`` writes no index
    (d_index NULL) and returns None in its place.

    ``sync=True`` waits, reads the count N and returns ``(points[:N], colors[:N] or None, index[:N])``;
    ValueError when N exceeds the capacity.  ``sync=False`` never touches the host: it returns the
    full-capacity tensors and the int32 count tensor ``(points, colors or None, index, count)``; the count is
    always the true N, only the first ``capacity`` points are written.  Three launches on ``stream``.

    Stream order: the outputs and the count are allocated on torch's current stream and written on ``stream``
    (only the workspace is marked with ``record_stream``), as in ``wmedian_device``.  With ``sync=False`` on a
    stream other than torch's current one the caller orders its later use of the returned tensors after
    ``stream`` (an event, ``wait_stream``) and keeps them alive until it has finished."""
    import torch

    H, W, c = _cloud_args(disp, focal_length, baseline, principal_point, doffs, eps, max_depth, x0)
    dev = disp.device
    if capacity is None:
        capacity = H * W
    if isinstance(capacity, bool) or int(capacity) != capacity or int(capacity) < 0:
        raise ValueError("capacity must be an integer >= 0")
    cap = int(capacity)
    ch = 0
    if colors is not None:
        ok = hasattr(colors, "dtype") and colors.dtype == torch.uint8 and colors.device == dev and \
            colors.dim() in (2, 3) and tuple(colors.shape[:2]) == (H, c.x0 + W)
        if ok and colors.dim() == 3:
            ok = colors.shape[2] == 3 and colors.stride(2) == 1 and colors.stride(1) == 3
        elif ok:
            ok = colors.shape[1] <= 1 or colors.stride(1) == 1
        if not ok:
            raise ValueError("colors must be a uint8 H x (x0 + W) gray or H x (x0 + W) x 3 BGR tensor on disp's "
                             "device with packed pixels")
        ch = 3 if colors.dim() == 3 else 1

    def own(t, shape, dtype, name):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if not hasattr(t, "data_ptr") or t.shape != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous {str(dtype).split('.')[-1]} tensor of shape {tuple(shape)} "
                             "on the input's device")
        return t

    points = own(out_points, (cap, 3), torch.float32, "out_points")
    cols = own(out_colors, (cap, 3), torch.uint8, "out_colors") if ch else None
    index = None if out_index is False else own(out_index, (cap,), torch.int32, "out_index")
    count = torch.empty(1, dtype=torch.int32, device=dev)
    L = _dsx.lib()
    nbytes = int(L.dsx_point_cloud_workspace_bytes(H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    rc = L.dsx_point_cloud_device(disp.data_ptr() if H and W else None, H, W, max(disp.stride(0), W), ctypes.byref(c),
                                  colors.data_ptr() if ch and H and W else None,
                                  max(colors.stride(0), (c.x0 + W) * ch) if ch else 0, ch,
                                  points.data_ptr() if cap else None, cols.data_ptr() if ch and cap else None,
                                  index.data_ptr() if cap and index is not None else None, cap, count.data_ptr(),
                                  None if ws is None else ws.data_ptr(), nbytes, _stream_ptr(stream))
    _dsx.check(rc, "dsx_point_cloud_device")
    if ws is not None:
        _keep_until_done(ws, stream)
    if not sync:
        return points, cols, index, count
    if stream is not None:
        st = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=dev)
        st.synchronize()
    n = int(count.item())
    if n > cap:
        raise ValueError(f"the cloud has {n} points but the outputs have room for {cap} (capacity)")
    return points[:n], None if cols is None else cols[:n], None if index is None else index[:n]


def fill_holes_status(workspace=None):
    """Raise RuntimeError if a hole-filling march timed out since the last check (its remaining
    holes were left unfilled); the condition is cleared.  ``workspace``: a ``FillWorkspace`` (its
    own flag, dsx_fill_holes_status_ws); None: every flag of the process (dsx_fill_holes_status)."""
    L = _dsx.lib()
    if workspace is not None and workspace.take_pending():
        _dsx.check(_dsx.DSX_EHIP, "hole filling: the persistent march timed out (on this workspace's previous "
                                  "buffer); the holes of that call were left unfilled")
    rc = L.dsx_fill_holes_status() if workspace is None else L.dsx_fill_holes_status_ws(workspace.ptr)
    _dsx.check(rc, "hole filling")


class FillWorkspace:
    """Device workspace of the hole-filling march on one device, grown on demand.  It carries the
    march's timeout flag and step history (both keyed by the workspace in the library), so calls
    that share one report to it: ``fill_holes_status(ws)``.  One stream at a time.

    When the buffer is replaced (a larger frame, another device) the old key is released in the
    library (``dsx_fill_holes_release``, after the device has finished with it) and a timeout it still
    held is kept here, so ``fill_holes_status(ws)`` reports it (a new buffer at a recycled
    address must not inherit the old flag, and the old flag must not be lost)."""

    def __init__(self, device=None):
        self.device = device
        self.buf = None
        self._pending = False

    def _release(self):
        if self.buf is None:
            return
        import torch
        torch.cuda.synchronize(self.buf.device)  # the device may still write the key's mapped words
        if _dsx.lib().dsx_fill_holes_release(self.buf.data_ptr()) != _dsx.DSX_OK:
            self._pending = True

    def get(self, nbytes, device, stream=None):
        import torch
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            if self.buf is not None:
                self._release()
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self.buf

    def take_pending(self) -> bool:
        p, self._pending = self._pending, False
        return p

    def close(self):
        """Release the buffer and its key in the library (a pending timeout stays reportable)."""
        self._release()
        self.buf = None

    @property
    def ptr(self):
        return None if self.buf is None else self.buf.data_ptr()


_fill_ws = {}
_FILL_WS_MAX = 8  # default workspaces kept (per (kind, device, stream)); the least recently used is closed


def _stream_ptr(stream):
    return None if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)


def default_workspace(device, stream, kind="fill"):
    """The workspace shared by the ``kind`` calls ("fill": fill_holes_device, "post":
    postprocess_full_device) on one (device, stream): a stable key for the library's step history
    and timeout flag.  At most ``_FILL_WS_MAX`` are kept (hundreds of MB each at 1080p); callers that use
    many streams should pass their own ``FillWorkspace``."""
    import torch
    key = (kind, device.index, _stream_ptr(stream) or torch.cuda.current_stream(device).cuda_stream)
    ws = _fill_ws.pop(key, None)
    if ws is None:
        ws = FillWorkspace(device)
        while len(_fill_ws) >= _FILL_WS_MAX:  # bounded: callers cycling through many streams
            _fill_ws.pop(next(iter(_fill_ws))).close()
    _fill_ws[key] = ws  # most recently used last
    return ws


def fill_holes_device(disp, radius=5, out=None, stream=None, workspace=None, spin_limit=0, steps=0,
                      method="inpaint", path=0):
    """fill_holes(disparity, method=method, kernel_size=radius) on the device (postprocess.py:72-118).
    'inpaint' (dsx_fill_holes_ex_device): Telea inpainting of the pixels <= 0 in cv2.inpaint's
    arrival-time order, equal to the host restatement (postprocess._telea_inpaint).  'nearest'
    (dsx_fill_nearest_device): ``radius`` is the kernel_size k - k masked dilations with the ellipse
    of radius k // 2, equal to the host ``fill_holes(method='nearest')``; stateless (no workspace
    object, no status flag); ``path`` 0 auto, 1 fused (k <= 5), 2 stepwise; ``out`` must not be ``disp``.
    ``disp``: float32 H x W HIP tensor (unit column stride).  Asynchronous on ``stream``; returns the
    filled float32 H x W tensor.  ``workspace``: a ``FillWorkspace`` (default: one per device and
    stream).  ``spin_limit`` / ``steps``: dsx_fill_opts (tests: force a timeout / the persistent
    launch)."""
    import torch

    method = _fill_method(method)
    if disp.dtype != torch.float32 or disp.dim() != 2 or disp.stride(1) != 1 or not disp.is_cuda:
        raise ValueError("disp must be a float32 H x W device tensor with unit column stride")
    H, W = disp.shape
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=disp.device)
    elif out.shape != (H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != disp.device:
        raise ValueError("out must be a contiguous float32 H x W tensor on the input's device")
    if H == 0 or W == 0:
        return out
    L = _dsx.lib()
    if method == _dsx.FILL_METHOD["nearest"]:
        k, path = int(radius), int(path)
        stepwise = path == _dsx.NEAREST_PATH["stepwise"] or (path == _dsx.NEAREST_PATH["auto"]
                                                             and k > _dsx.NEAREST_FUSED_MAX)
        nbytes = L.dsx_fill_nearest_workspace_bytes(H, W) if stepwise and k >= 2 else 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=disp.device) if nbytes else None
        rc = L.dsx_fill_nearest_device(disp.data_ptr(), H, W, disp.stride(0), k, out.data_ptr(),
                                       None if ws is None else ws.data_ptr(), nbytes, path, _stream_ptr(stream))
        _dsx.check(rc, "dsx_fill_nearest_device")
        if ws is not None:
            _keep_until_done(ws, stream)
        return out
    nbytes = L.dsx_fill_holes_workspace_bytes(H, W)
    wsobj = workspace if workspace is not None else default_workspace(disp.device, stream, "fill")
    ws = wsobj.get(nbytes, disp.device, stream)
    opts = _dsx.DsxFillOpts()
    opts.spin_limit = int(spin_limit)
    opts.steps = int(steps)
    rc = L.dsx_fill_holes_ex_device(disp.data_ptr(), H, W, disp.stride(0), int(radius), out.data_ptr(), ws.data_ptr(),
                                    nbytes, ctypes.byref(opts), _stream_ptr(stream))
    _dsx.check(rc, "dsx_fill_holes_ex_device")
    _keep_until_done(ws, stream)
    return out


class TemporalFilterDevice:
    """The temporal disparity filter on one HIP device (dsx_tfilter, include/dsx.h; host restatement
    depthestimation_amd/temporal.py ``TemporalFilter``, equal bit for bit on every frame): a motion-gated
    recursive average of the finished disparity maps of a video with a temporal hole filler.  The object owns
    the state (filtered disparity, age, hold count, previous guide); a frame of another shape reallocates and
    resets it.  Frames are filtered in the order of the ``run`` calls whatever their streams: the library
    orders a call on another stream behind the previous call's kernel (an event, no host wait), so one object
    serves a pipeline with several frames in flight.  One caller at a time."""

    def __init__(self, device=0, max_age=4, max_diff=1.0, motion_radius=1, motion_threshold=6, hold=2):
        self.device = int(device)
        self._params = _dsx.make_temporal("recursive", max_age, max_diff, motion_radius, motion_threshold, hold)
        self._f = None

    def _filter(self):
        if self._f is None:
            if _dsx.device_count() == 0:
                raise RuntimeError("TemporalFilterDevice: no HIP device visible (the engine has no CPU fallback)")
            f = ctypes.c_void_p()
            _dsx.check(_dsx.lib().dsx_tfilter_create(self.device, ctypes.byref(self._params), ctypes.byref(f)),
                       "dsx_tfilter_create")
            self._f = f
        return self._f

    def set_params(self, max_age=4, max_diff=1.0, motion_radius=1, motion_threshold=6, hold=2):
        """Replace the parameters (dsx_tfilter_set_params); the state is reset."""
        t = _dsx.make_temporal("recursive", max_age, max_diff, motion_radius, motion_threshold, hold)
        if self._f is not None:
            _dsx.check(_dsx.lib().dsx_tfilter_set_params(self._f, ctypes.byref(t)), "dsx_tfilter_set_params")
        self._params = t

    def reset(self):
        """The next frame has no previous frame."""
        if self._f is not None:
            _dsx.check(_dsx.lib().dsx_tfilter_reset(self._f), "dsx_tfilter_reset")

    def state_bytes(self) -> int:
        b = ctypes.c_int64(0)
        _dsx.check(_dsx.lib().dsx_tfilter_bytes(self._filter(), ctypes.byref(b)), "dsx_tfilter_bytes")
        return b.value

    def run(self, disp, guide, out=None, focal_length=None, baseline=None, doffs=0.0, eps=1e-6, max_depth=None,
            out_depth=None, stream=None):
        """One frame, asynchronous on ``stream`` (dsx_tfilter_run_device).  ``disp``: float32 H x W HIP tensor,
        ``guide``: uint8 H x W HIP tensor over the same pixels (both unit column stride, any row stride or
        offset: the pitched view ``left[:, num_disp:]`` is fine).  ``out``: a contiguous float32 H x W tensor,
        which may be ``disp`` itself when that is contiguous; None allocates one.  With ``focal_length`` and
        ``baseline`` the same launch writes the depth of the filtered map (``StereoCore.disparity_to_depth``,
        bit for bit).  Returns (out, depth or None)."""
        import torch

        if not hasattr(disp, "dtype") or disp.dtype != torch.float32 or disp.dim() != 2 or not disp.is_cuda or \
                (disp.shape[1] > 1 and disp.stride(1) != 1):
            raise ValueError("disp must be a float32 H x W device tensor with unit column stride")
        if not hasattr(guide, "dtype") or guide.dtype != torch.uint8 or guide.shape != disp.shape or \
                guide.device != disp.device or (guide.shape[1] > 1 and guide.stride(1) != 1):
            raise ValueError("guide must be a uint8 tensor of disp's shape on its device with unit column stride")
        _check_inputs_on(self.device, disp, guide)
        H, W = disp.shape
        if out is None:
            out = torch.empty((H, W), dtype=torch.float32, device=disp.device)
        _check_out(out, (H, W), "torch.float32", self.device, "out")
        want_depth = focal_length is not None and baseline is not None
        if want_depth and out_depth is None:
            out_depth = torch.empty((H, W), dtype=torch.float32, device=disp.device)
        if want_depth:
            _check_out(out_depth, (H, W), "torch.float32", self.device, "out_depth")
        if H == 0 or W == 0:
            return out, (out_depth if want_depth else None)
        rc = _dsx.lib().dsx_tfilter_run_device(
            self._filter(), disp.data_ptr(), H, W, max(disp.stride(0), W) if H > 1 else W, guide.data_ptr(),
            max(guide.stride(0), W) if H > 1 else W, _ptr(out), _ptr(out_depth) if want_depth else None,
            float(focal_length or 0.0), float(baseline or 0.0), float(doffs or 0.0), float(eps),
            float(max_depth or 0.0), int(max_depth is not None), _stream_ptr(stream))
        _dsx.check(rc, "dsx_tfilter_run_device")
        return out, (out_depth if want_depth else None)

    def close(self):
        if self._f is not None:
            _dsx.lib().dsx_tfilter_destroy(self._f)
            self._f = None

    def __del__(self):  # pragma: no cover - GC timing
        try:
            self.close()
        except Exception:
            pass


def joint_upsample_device(disp, x0, guide_lo, guide, radius=1, sigma=8, max_diff=1.0, focal_length=None,
                          baseline=None, doffs=0.0, eps=1e-6, max_depth=None, out=None, out_depth=None, stream=None):
    """The joint bilateral upsampling of a downscaled run's map on the device (dsx_upsample_device; host
    restatement upsample.joint_upsample, equal bit for bit).  ``disp``: the finished float32 h x w HIP tensor whose
    column 0 is low-resolution column ``x0``; ``guide_lo``: the uncropped uint8 h x Wl low-resolution image the
    matcher ran on (Wl = x0 + w); ``guide``: the full-size uint8 frame, H x W or H x W x 3 (the kernel forms the
    gray value).  All with unit element stride along a row, any row stride or offset.  Returns ``(out, depth)``:
    contiguous float32 H x (W - X0) tensors, the disparity in full-size pixels and, with ``focal_length`` and
    ``baseline`` (the low-resolution calibration), the metric depth written by the same launch; else None.
    Stateless, asynchronous on ``stream``."""
    import torch

    if not hasattr(disp, "dtype") or disp.dtype != torch.float32 or disp.dim() != 2 or not disp.is_cuda or \
            (disp.shape[1] > 1 and disp.stride(1) != 1):
        raise ValueError("disp must be a float32 h x w device tensor with unit column stride")
    if not hasattr(guide_lo, "dtype") or guide_lo.dtype != torch.uint8 or guide_lo.dim() != 2 or \
            guide_lo.device != disp.device or guide_lo.shape[0] != disp.shape[0] or \
            (guide_lo.shape[1] > 1 and guide_lo.stride(1) != 1):
        raise ValueError("guide_lo must be a uint8 h x Wl tensor on disp's device with unit column stride")
    if not hasattr(guide, "dtype") or guide.dtype != torch.uint8 or guide.dim() not in (2, 3) or \
            guide.device != disp.device or (guide.dim() == 3 and guide.shape[2] not in (1, 3)):
        raise ValueError("guide must be a uint8 H x W or H x W x 3 tensor on disp's device")
    ch = 1 if guide.dim() == 2 else int(guide.shape[2])
    H, W = int(guide.shape[0]), int(guide.shape[1])
    if guide.dim() == 3 and (guide.stride(2) != 1 or (W > 1 and guide.stride(1) != ch)):
        raise ValueError("guide must have its channels interleaved (unit element stride along a row)")
    if guide.dim() == 2 and W > 1 and guide.stride(1) != 1:
        raise ValueError("guide must have unit column stride")
    h, w = int(disp.shape[0]), int(disp.shape[1])
    Wl, x0 = int(guide_lo.shape[1]), int(x0)
    if x0 < 0 or x0 + w != Wl:
        raise ValueError("disp must cover the low-resolution columns x0 .. Wl - 1 (x0 + w == Wl)")
    if not (1 <= h <= H <= 32768 and 1 <= Wl <= W <= 32768):
        raise ValueError("shapes must satisfy 1 <= h <= H <= 32768 and 1 <= Wl <= W <= 32768")
    up = _dsx.make_upsample("joint", radius, sigma, max_diff)
    X0 = _dsx.lib().dsx_upsample_x0(W, Wl, x0)
    _dsx.check(min(X0, 0), "dsx_upsample_x0")
    dev = _device_index(disp)
    shape = (H, W - X0)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=disp.device)
    _check_out(out, shape, "torch.float32", dev, "out")
    want_depth = focal_length is not None and baseline is not None
    if want_depth and out_depth is None:
        out_depth = torch.empty(shape, dtype=torch.float32, device=disp.device)
    if want_depth:
        _check_out(out_depth, shape, "torch.float32", dev, "out_depth")
    if w == 0 or shape[1] == 0:
        return out, (out_depth if want_depth else None)
    rc = _dsx.lib().dsx_upsample_device(
        disp.data_ptr(), h, w, max(disp.stride(0), w) if h > 1 else w, x0, guide_lo.data_ptr(), Wl,
        max(guide_lo.stride(0), Wl) if h > 1 else Wl, guide.data_ptr(), H, W, ch,
        max(guide.stride(0), W * ch) if H > 1 else W * ch, ctypes.byref(up), _ptr(out),
        _ptr(out_depth) if want_depth else None, float(focal_length or 0.0), float(baseline or 0.0),
        float(doffs or 0.0), float(eps), float(max_depth or 0.0), int(max_depth is not None), _stream_ptr(stream))
    _dsx.check(rc, "dsx_upsample_device")
    return out, (out_depth if want_depth else None)
