"""StereoCore - host-side mirror of depthlib/stereo_core.py with the MI355X block matcher.

Same class, method names, parameter dict, validation and error behaviour as the reference
(depthlib/stereo_core.py:7-293). The one seam that changes is the matcher object:
``_build_sgbm`` (stereo_core.py:44-75) builds a :class:`HipBlockMatcher` (libdsx.so, C-ABI in
include/dsx.h) instead of ``cv2.StereoSGBM_create``, and ``compute_disparity``
(stereo_core.py:212-232) calls its ``compute`` with the same cv2 contract (int16 x16 -> /16).

Keys added to ``sgbm_params`` (accepted by ``configure_sgbm`` like the reference's own keys):
  'cost'     : 'sad' | 'ssd' | 'bt' | 'census9x7' | 'census5x5'
                                      (block cost; north_star SAD/SSD; 'bt' is OpenCV SGBM's
                                       Birchfield-Tomasi pixel cost on the 'prefilter_cap'-clipped
                                       x-derivative plus intensity, summed over the same block; the
                                       census costs are this build's addition (census.py): the Hamming
                                       distance of 9x7 (62-bit) or 5x5 (24-bit) rank codes, invariant to
                                       gain and shading, the usual pixel cost under 'aggregation': 'sgm'
                                       with 'block_size' 1.  'prefilter_type' and 'texture_threshold' are
                                       refused with a census cost: census ranks intensities itself)
  'sgbm_post': bool                   (False; True runs cv2.StereoSGBM::compute's own tail on the
                                       int16 map: 3x3 median, then filterSpeckles with
                                       'speckle_window_size' / 'speckle_range' and newVal
                                       (min_disp - 1) * 16)
  'subpixel' : bool                   (1/16-px parabola refinement, on by default)
  'device'   : int                    (HIP device of the matcher)
  'lr_form'  : 'bm' | 'sgbm'          ('bm', the default: the A5' right-view argmin over every cost;
                                       'sgbm': cv2.StereoSGBM's own check - disp2 from the unique left
                                       winners, floor / ceiling test, disp12MaxDiff >= 1, its valid
                                       band [max(min_disp + num_disp, 0), W + min(min_disp, 0));
                                       runs on the volume path)
  'aggregation': 'none' | 'sgm'       ('none', the default, is the north-star block matching;
                                       'sgm' adds semi-global aggregation over the SAD costs with
                                       the path set of 'sgbm_mode' and P1 = 8 bs^2, P2 = 32 bs^2 as
                                       _build_sgbm derives them, stereo_core.py:51-61)
  'fill_method': 'inpaint' | 'nearest' (with 'hole_filling': fill_holes' method, postprocess.py:72-118.
                                       'inpaint', the default and the reference's choice, is Telea's
                                       march; 'nearest' is the iterated dilation - bounded, stateless,
                                       nothing to time out, and fast enough for video)
  'prefilter_type': 'none' | 'xsobel' | 'mean'  ('none', the default: raw intensities.  cv2.StereoBM's
                                       prefilter in this build's arithmetic (prefilter.py): both views are
                                       filtered on the device before the SAD / SSD search, which makes it
                                       usable on cameras of unequal exposure or shading; 'prefilter_cap' is
                                       the cap, 'prefilter_size' (odd, 5..21) the window of 'mean')
  'texture_threshold': int            (0 = off; > 0 needs a prefilter: pixels whose filtered block sums
                                       less than this much |P - cap| become invalid)
  'refine': 'none' | 'wmedian'         ('none', the default.  'wmedian': the image-guided weighted median of
                                       postprocess.weighted_median_filter after the hole filling, if any,
                                       and before the median, guided by the left rectified image - the
                                       `left_image` the reference passes and never reads.  It thins the
                                       fattened foreground at depth edges and, with 'refine_fill' (True),
                                       fills invalid pixels from similar-looking neighbours: one stateless
                                       launch, fast enough for video.  'refine_radius' 1..7 (5),
                                       'refine_sigma' 1..64 grey levels (8).  Ignored in fast mode, as
                                       'hole_filling' is)
  'confidence': bool                  (False.  True: ``_process_pair`` and ``process_pair_device`` also keep
                                       the matcher's peak-ratio confidence map (confidence.py; uint8, 255 =
                                       no rival, 0 = a tie or outside the valid band), cropped like the
                                       disparity, in ``confidence_map`` - a numpy array on the host, a
                                       tensor on the device.  The map comes from the volume path's K2, so a
                                       SAD / SSD core pays that path for it; return values are unchanged)
  'confidence_threshold': int         (0 = off; t in 1..255: pixels of confidence below t become invalid
                                       after the LR check, before the texture mask and 'sgbm_post' - holes
                                       for the fillers and 'refine' to close from trusted neighbours)
  'principal_point': (cx, cy) | None  (None.  The principal point of the left rectified image in uncropped
                                       pixel coordinates, scaled by downscale_factor like 'focal_length'; used
                                       by ``point_cloud`` (pointcloud.py: disparity -> XYZ + RGB).  None: with
                                       a full calibration the rectification's own P1, else the image centre)
  'temporal': 'none' | 'recursive'    ('none', the default.  'recursive': the temporal disparity filter of temporal.py
                                       behind the mode's tail (fast and full mode alike) - a motion-gated
                                       recursive average of the finished maps of consecutive frames that also
                                       holds a static pixel's last value over short holes, guided by the raw
                                       left rectified image.  It removes the frame-to-frame flicker of block
                                       matching on video; the state lives in this core (``reset_temporal()``
                                       forgets it, as any ``configure_sgbm`` and any change of the frame's
                                       shape do), so frames must arrive in order.  'temporal_max_age' 1..64 (4),
                                       'temporal_max_diff' > 0 px (1.0), 'temporal_motion_radius' 0..2 (1),
                                       'temporal_motion_threshold' 0..255 grey levels per tap (6),
                                       'temporal_hold' 0..255 frames (2))
  'upsample': 'none' | 'joint'        ('none', the default.  'joint': full-resolution output for downscaled runs -
                                       the joint bilateral upsampling of upsample.py.  It runs only in calls that
                                       carry ``input_scale`` != 1 (``estimate_depth`` / ``estimate_depth_device``, and
                                       through them the facades with ``device_downscale=True`` and
                                       ``DepthPipeline(input_scale=...)``), behind the mode's tail and behind the
                                       temporal filter, which keeps working and keeping its state at low resolution:
                                       one launch reads the finished low-resolution map, the low-resolution left
                                       image and the full-size left frame and writes ``disparity_map`` in full-size
                                       pixels and ``depth_map``, both H x (W - X0) with X0 = upsample.upsample_x0(W,
                                       Wl, num_disp).  Without ``input_scale`` the key is ignored, as fast mode
                                       ignores 'hole_filling': there is no full-size frame.  With a full calibration
                                       the call raises ValueError: rectification runs after the downscale, so the
                                       full-size frame is not rectified and cannot guide.  ``confidence_map`` stays
                                       low-resolution; ``point_cloud`` after an upsampled frame raises ValueError
                                       (its intrinsics and crop are the low-resolution ones).  'upsample_radius'
                                       1..3 (1), 'upsample_sigma' 1..64 grey levels (8), 'upsample_max_diff' > 0
                                       low-resolution px (1.0))
Keys of the reference that have no block-matching meaning are kept, validated and reported
but do not change the result: 'prefilter_cap' unless 'cost' is 'bt' or a prefilter is set, 'speckle_window_size' /
'speckle_range' unless 'sgbm_post' is set, and 'sgbm_mode' / P1 / P2 while 'aggregation' is 'none'
(SURVEY.md 8a A5').  cost='bt' + aggregation='sgm' + lr_form='sgbm' + sgbm_post=True is this build's
closest form of the reference's cv2.StereoSGBM.

There is no CPU fallback: without libdsx.so or a HIP device ``compute_disparity`` raises.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from .input import resize_area, resize_area_device
from .matcher import (HipBlockMatcher, TemporalFilterDevice, default_workspace, fill_holes_status, joint_upsample_device,
                      postprocess_fast_device, point_cloud_device, postprocess_full_device, rectify_device)
from .pointcloud import point_cloud as host_point_cloud
from .postprocess import median_blur3, postprocess_disparity
from .temporal import TemporalFilter, check_temporal
from .upsample import check_upsample, joint_upsample
from .rectify import RectificationCache, rectified_principal_point, rectify_images, to_grayscale_bgr

_SGBM_MODES = ("sgbm", "hh", "sgbm_3way", "hh4")
_CALIBRATION_KEYS = ('cam_matrix_L', 'cam_matrix_R', 'baseline', 'image_width', 'image_height')


def _valid_principal_point(pp) -> bool:
    """Two finite numbers (cx, cy)."""
    try:
        return len(pp) == 2 and all(not isinstance(v, (bool, np.bool_)) and np.isfinite(float(v)) for v in pp)
    except (TypeError, ValueError):
        return False


class _HostView:
    """A device tensor handed out as a numpy array on first read (estimate_depth's stored
    rectified images: copied back over PCIe only if the caller looks at them)."""

    __slots__ = ("t",)

    def __init__(self, t):
        self.t = t


class _TemporalState:
    """The temporal filter of one StereoCore: the parameters, the host restatement (the host path) and the
    device object (the device routes), each created on first use.  Shallow copies of a core share it, so the
    per-slot copies of a ``multigpu.DepthPipeline`` filter one sequence."""

    def __init__(self, **kw):
        self.kw = kw
        self.host = None
        self.dev = None

    def host_filter(self) -> TemporalFilter:
        if self.host is None:
            self.host = TemporalFilter(**self.kw)
        return self.host

    def device_filter(self, device: int) -> TemporalFilterDevice:
        if self.dev is not None and self.dev.device != device:
            self.dev.close()
            self.dev = None
        if self.dev is None:
            self.dev = TemporalFilterDevice(device=device, **self.kw)
        return self.dev

    def reset(self) -> None:
        if self.host is not None:
            self.host.reset()
        if self.dev is not None:
            self.dev.reset()

    def close(self) -> None:
        if self.dev is not None:
            self.dev.close()
        self.host = self.dev = None


class StereoCore:
    """Handles common stereo operations (stereo_core.py:7)."""

    # left_rectified / right_rectified (stereo_core.py:289-291): plain attributes, except that
    # estimate_depth's device pipeline stores them as lazy host views
    @property
    def left_rectified(self):
        v = self.__dict__.get("_left_rect")
        if isinstance(v, _HostView):
            v = self.__dict__["_left_rect"] = v.t.cpu().numpy()
        return v

    @left_rectified.setter
    def left_rectified(self, v):
        self.__dict__["_left_rect"] = v

    @property
    def right_rectified(self):
        v = self.__dict__.get("_right_rect")
        if isinstance(v, _HostView):
            v = self.__dict__["_right_rect"] = v.t.cpu().numpy()
        return v

    @right_rectified.setter
    def right_rectified(self, v):
        self.__dict__["_right_rect"] = v

    def __init__(self, downscale_factor=1.0, fast_mode=False) -> None:
        self.downscale_factor = downscale_factor
        self.fast_mode = fast_mode
        self.sgbm = None
        self._rect_cache = RectificationCache()
        self._dev_maps = None  # (host maps dict id, device, (map1_L, map2_L, map1_R, map2_R) on the device)
        # stereo_core.py:16-39 defaults, then the build keys
        self.sgbm_params = {
            'min_disp': 0,
            'num_disp': 128,
            'block_size': 5,
            'disp12_max_diff': 1,
            'prefilter_cap': 31,
            'uniqueness_ratio': 10,
            'speckle_window_size': 50,
            'speckle_range': 2,
            'sgbm_mode': 'sgbm_3way',
            'focal_length': None,
            'baseline': None,
            'doffs': 0.0,
            'max_depth': None,
            'cam_matrix_L': None,
            'cam_matrix_R': None,
            'image_width': None,
            'image_height': None,
            'dist_coeff_L': None,
            'dist_coeff_R': None,
            'rotation': None,
            'translation': None,
            'hole_filling': False,
            'cost': 'sad',
            'subpixel': True,
            'device': 0,
            'aggregation': 'none',
            'sgbm_post': False,
            'lr_form': 'bm',
            'fill_method': 'inpaint',
            'prefilter_type': 'none',
            'prefilter_size': 9,
            'texture_threshold': 0,
            'refine': 'none',
            'refine_radius': 5,
            'refine_sigma': 8,
            'refine_fill': True,
            'confidence': False,
            'confidence_threshold': 0,
            'principal_point': None,
            'temporal': 'none',
            'temporal_max_age': 4,
            'temporal_max_diff': 1.0,
            'temporal_motion_radius': 1,
            'temporal_motion_threshold': 6,
            'temporal_hold': 2,
            'upsample': 'none',
            'upsample_radius': 1,
            'upsample_sigma': 8,
            'upsample_max_diff': 1.0,
        }
        self._temporal = None
        self._upsampled = False  # the last frame's maps are full-size (point_cloud refuses them)
        self._pp_cache = None  # (calibration key, (cx, cy) of the left rectified image)
        self.confidence_map = None
        self._build_sgbm()
        self.disparity_map = None
        self.depth_map = None

    # -- matcher -------------------------------------------------------------------------
    def _build_sgbm(self):
        """stereo_core.py:44-75 -> HipBlockMatcher. P1/P2 and the mode are recorded for
        reporting and drive the optional SGM aggregation ('aggregation': 'sgm')."""
        p = self.sgbm_params
        if p.get('aggregation', 'none') not in ('none', 'sgm'):
            raise ValueError("Invalid parameter value for 'aggregation': expected 'none' or 'sgm'")
        if p.get('fill_method', 'inpaint') not in ('inpaint', 'nearest'):
            raise ValueError("Invalid parameter value for 'fill_method': expected 'inpaint' or 'nearest'")
        if p.get('refine', 'none') not in ('none', 'wmedian'):
            raise ValueError("Invalid parameter value for 'refine': expected 'none' or 'wmedian'")
        r, sg = p.get('refine_radius', 5), p.get('refine_sigma', 8)
        if isinstance(r, bool) or int(r) != r or not 1 <= int(r) <= 7:
            raise ValueError("Invalid parameter value for 'refine_radius': expected an integer in [1, 7]")
        if isinstance(sg, bool) or int(sg) != sg or not 1 <= int(sg) <= 64:
            raise ValueError("Invalid parameter value for 'refine_sigma': expected an integer in [1, 64]")
        if not isinstance(p.get('confidence', False), (bool, np.bool_)):
            raise ValueError("Invalid parameter value for 'confidence': expected a bool")
        t = p.get('confidence_threshold', 0)
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)) or \
                int(t) != t or not 0 <= int(t) <= 255:
            raise ValueError("Invalid parameter value for 'confidence_threshold': expected an integer in [0, 255]")
        if p.get('principal_point') is not None and not _valid_principal_point(p['principal_point']):
            raise ValueError("Invalid parameter value for 'principal_point': expected None or two finite numbers")
        if p.get('temporal', 'none') not in ('none', 'recursive'):
            raise ValueError("Invalid parameter value for 'temporal': expected 'none' or 'recursive'")
        tkw = self._temporal_kwargs()
        for key, (lo, hi) in (('max_age', (1, 64)), ('motion_radius', (0, 2)), ('motion_threshold', (0, 255)),
                              ('hold', (0, 255))):
            try:
                check_temporal(**{key: tkw[key]})
            except ValueError:
                raise ValueError(f"Invalid parameter value for 'temporal_{key}': expected an integer in "
                                 f"[{lo}, {hi}]") from None
        try:
            check_temporal(max_diff=tkw['max_diff'])
        except ValueError:
            raise ValueError("Invalid parameter value for 'temporal_max_diff': expected a finite number > 0") from None
        if p.get('upsample', 'none') not in ('none', 'joint'):
            raise ValueError("Invalid parameter value for 'upsample': expected 'none' or 'joint'")
        ukw = self._upsample_kwargs()
        for key, (lo, hi) in (('radius', (1, 3)), ('sigma', (1, 64))):
            try:
                check_upsample(**{key: ukw[key]})
            except ValueError:
                raise ValueError(f"Invalid parameter value for 'upsample_{key}': expected an integer in "
                                 f"[{lo}, {hi}]") from None
        try:
            check_upsample(max_diff=ukw['max_diff'])
        except ValueError:
            raise ValueError("Invalid parameter value for 'upsample_max_diff': expected a finite number > 0") from None
        # any (re)configuration forgets the temporal state; the filter objects are built on first use
        if getattr(self, '_temporal', None) is not None:
            self._temporal.close()
        self._temporal = _TemporalState(**tkw) if p.get('temporal', 'none') == 'recursive' else None
        self.P1 = 8 * p['block_size'] ** 2
        self.P2 = 32 * p['block_size'] ** 2
        self.mode = p.get('sgbm_mode', 'sgbm_3way') if p.get('sgbm_mode') in _SGBM_MODES else 'sgbm_3way'
        old = self.sgbm
        self.sgbm = HipBlockMatcher(
            min_disp=p['min_disp'],
            num_disp=max(int(p['num_disp']), 1),
            block_size=p['block_size'],
            cost=p['cost'],
            uniqueness_ratio=p['uniqueness_ratio'],
            disp12_max_diff=p['disp12_max_diff'],
            subpixel=p['subpixel'],
            device=p['device'],
            aggregation=self.mode if p.get('aggregation', 'none') == 'sgm' else None,
            p1=self.P1,
            p2=self.P2,
            prefilter_cap=p['prefilter_cap'],
            sgbm_post=bool(p.get('sgbm_post', False)),
            speckle_window_size=p['speckle_window_size'],
            speckle_range=p['speckle_range'],
            lr_form=p.get('lr_form', 'bm'),
            prefilter_type=p.get('prefilter_type', 'none'),
            prefilter_size=p.get('prefilter_size', 9),
            texture_threshold=p.get('texture_threshold', 0),
            confidence_threshold=int(t),
        )
        if old is not None:
            old.close()

    def configure_sgbm(self, **kwargs):
        """stereo_core.py:77-123: unknown keys -> ValueError; num_disp / focal_length / doffs
        scaled by downscale_factor (int() truncation for num_disp); matcher rebuilt."""
        valid_params = self.sgbm_params.keys()
        for key in kwargs:
            if key not in valid_params:
                raise ValueError(f"Invalid parameter '{key}'. Valid parameters: {list(valid_params)}")
        if 'num_disp' in kwargs:
            kwargs['num_disp'] = int(kwargs['num_disp'] * self.downscale_factor)
        if 'focal_length' in kwargs:
            kwargs['focal_length'] = kwargs['focal_length'] * self.downscale_factor
        if 'doffs' in kwargs:
            kwargs['doffs'] = kwargs['doffs'] * self.downscale_factor
        if _valid_principal_point(kwargs.get('principal_point')):  # anything else: _build_sgbm refuses it
            kwargs['principal_point'] = tuple(float(v) * self.downscale_factor for v in kwargs['principal_point'])
        self.sgbm_params.update(kwargs)
        self._build_sgbm()

    def _refine_kwargs(self) -> dict:
        """The 'refine*' keys as the keywords of postprocess_disparity and the device calls."""
        p = self.sgbm_params
        return dict(refine=p.get('refine', 'none'), refine_radius=int(p.get('refine_radius', 5)),
                    refine_sigma=int(p.get('refine_sigma', 8)), refine_fill=bool(p.get('refine_fill', True)))

    def _temporal_kwargs(self) -> dict:
        """The 'temporal_*' keys as the keywords of TemporalFilter / TemporalFilterDevice."""
        p = self.sgbm_params
        return dict(max_age=p.get('temporal_max_age', 4), max_diff=p.get('temporal_max_diff', 1.0),
                    motion_radius=p.get('temporal_motion_radius', 1),
                    motion_threshold=p.get('temporal_motion_threshold', 6), hold=p.get('temporal_hold', 2))

    def _upsample_kwargs(self) -> dict:
        """The 'upsample_*' keys as the keywords of joint_upsample / joint_upsample_device."""
        p = self.sgbm_params
        return dict(radius=p.get('upsample_radius', 1), sigma=p.get('upsample_sigma', 8),
                    max_diff=p.get('upsample_max_diff', 1.0))

    def _depth_kwargs(self) -> dict:
        """The depth scalars as the upsampling launch takes them (the low-resolution calibration)."""
        p = self.sgbm_params
        return dict(focal_length=p.get('focal_length'), baseline=p.get('baseline'), doffs=p.get('doffs', 0.0),
                    eps=p.get('min_disp', 5.0), max_depth=p.get('max_depth'))

    def _upsample_on(self, input_scale) -> bool:
        """The stage runs in this call: 'upsample': 'joint' and an ``input_scale`` other than 1.  ValueError with
        a full calibration set."""
        p = self.sgbm_params
        if p.get('upsample', 'none') != 'joint' or input_scale is None or input_scale == 1.0:
            return False
        if all(p.get(k) is not None for k in _CALIBRATION_KEYS):
            raise ValueError("'upsample': 'joint' cannot run with a full calibration: rectification runs after the "
                             "downscale, so the full-size frame is not rectified and cannot guide the upsampling")
        return True

    def reset_temporal(self) -> None:
        """Forget the temporal filter's state: the next frame is filtered as a first frame (a scene cut)."""
        if self._temporal is not None:
            self._temporal.reset()

    def get_sgbm_params(self) -> Dict[str, int]:
        return self.sgbm_params.copy()

    # -- pipeline ------------------------------------------------------------------------
    def _prepare_rectified(self, left_img: np.ndarray, right_img: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """stereo_core.py:125-160: rectify when calibrated, else BGR->gray."""
        p = self.sgbm_params
        if all(p.get(k) is not None for k in ('cam_matrix_L', 'cam_matrix_R', 'baseline', 'image_width',
                                               'image_height')):
            return rectify_images(left_img, right_img, p['cam_matrix_L'], p['cam_matrix_R'], p['baseline'],
                                  p['image_width'], p['image_height'], dist_coeff_L=p.get('dist_coeff_L'),
                                  dist_coeff_R=p.get('dist_coeff_R'), rotation=p.get('rotation'),
                                  translation=p.get('translation'), alpha=1.0, cache=self._rect_cache)
        if left_img.ndim == 3:
            left_img = to_grayscale_bgr(left_img)
        if right_img.ndim == 3:
            right_img = to_grayscale_bgr(right_img)
        return left_img, right_img

    def _process_pair(self, left_img: np.ndarray, right_img: np.ndarray,
                      full_guide=None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """stereo_core.py:162-200: disparity -> crop [:, num_disp:] -> median (fast) or
        postprocess -> depth when focal length and baseline are set.  ``full_guide``: the full-size left frame of
        a call with ``input_scale`` and 'upsample': 'joint' - the maps are then upsampled to it (upsample.py)."""
        raw_left = np.asarray(left_img)
        self._upsampled = False
        if self.sgbm_params.get('confidence', False) and 'compute_disparity' not in self.__dict__:
            if self.sgbm is None:
                self._build_sgbm()
            conf = np.empty(np.asarray(left_img).shape[:2], np.uint8)
            disparity_px = self.sgbm.compute(left_img, right_img, out_confidence=conf).astype(np.float32) / 16.0
            self.confidence_map = conf[:, self.sgbm_params['num_disp']:]
        else:
            disparity_px = self.compute_disparity(left_img, right_img)
            self.confidence_map = None
        disparity_px = disparity_px[:, self.sgbm_params['num_disp']:]
        guide = np.asarray(left_img)[:, self.sgbm_params['num_disp']:] if self._temporal is not None else None
        refine = self._refine_kwargs()
        if refine['refine'] != 'none' and not self.fast_mode:
            left_img = np.asarray(left_img)[:, self.sgbm_params['num_disp']:]  # the guide: the map's own pixels
        if self.fast_mode:
            disparity_px = median_blur3(disparity_px.astype(np.float32))
        else:
            disparity_px = postprocess_disparity(
                disparity_px,
                left_image=left_img,
                max_speckle_size=int(100 * self.downscale_factor),
                max_diff=1.0,
                outlier_threshold=2.5,
                fill_method=self.sgbm_params.get('fill_method', 'inpaint'),
                apply_outlier_removal=True,
                apply_hole_filling=self.sgbm_params.get('hole_filling', False),
                **refine,
            )
        if self._temporal is not None:  # behind the mode's tail, guided by the raw left image
            disparity_px = self._temporal.host_filter()(np.ascontiguousarray(disparity_px, np.float32), guide)
        f_pixels = self.sgbm_params.get('focal_length', None)
        baseline_m = self.sgbm_params.get('baseline', None)
        doffs = self.sgbm_params.get('doffs', 0.0)
        min_disparity = self.sgbm_params.get('min_disp', 5.0)
        max_depth = self.sgbm_params.get('max_depth')
        depth_m = None
        if full_guide is not None:  # the upsampling writes the depth of the unscaled average
            disparity_px, depth_m = joint_upsample(np.ascontiguousarray(disparity_px, np.float32),
                                                   min(self.sgbm_params['num_disp'], raw_left.shape[1]), raw_left,
                                                   full_guide,
                                                   **self._upsample_kwargs(), **self._depth_kwargs())
            self._upsampled = True
        elif f_pixels is not None and baseline_m is not None:
            depth_m = self.disparity_to_depth(disparity_px, f_pixels, baseline_m, doffs, eps=min_disparity,
                                              max_depth=max_depth)
        self.disparity_map = disparity_px
        self.depth_map = depth_m
        return disparity_px, depth_m

    def compute_disparity(self, rectified_L: np.ndarray, rectified_R: np.ndarray) -> np.ndarray:
        """stereo_core.py:212-232: float32 disparity in pixels (1/16-px steps), invalid
        (min_disp - 1)."""
        if self.sgbm is None:
            self._build_sgbm()
        disp_fixed = self.sgbm.compute(rectified_L, rectified_R)
        return disp_fixed.astype(np.float32) / 16.0

    def compute_disparity_device(self, left, right, out=None, stream=None):
        """Device-resident variant: uint8 HIP tensors in, float32 HIP tensor out (the
        kernel writes fixed/16 directly; nothing crosses PCIe)."""
        import torch
        if self.sgbm is None:
            self._build_sgbm()
        if out is None:
            out = torch.empty(left.shape, dtype=torch.float32, device=left.device)
        self.sgbm.compute_device(left, right, out_float=out, stream=stream)
        return out

    def _prepare_rectified_device(self, left, right, stream=None):
        """Device version of ``_prepare_rectified`` (stereo_core.py:125-160): uint8 HIP frames
        (H x W x 3 BGR or gray) -> rectified gray on the device.  The maps come from the same
        host RectificationCache (computed once per calibration) and stay resident in HBM."""
        import torch
        p = self.sgbm_params
        if all(p.get(k) is not None for k in ('cam_matrix_L', 'cam_matrix_R', 'baseline', 'image_width',
                                               'image_height')):
            W, H = int(p['image_width']), int(p['image_height'])
            if tuple(left.shape[:2]) != (H, W) or tuple(right.shape[:2]) != (H, W):
                raise ValueError("device rectification needs frames of the calibrated size "
                                 f"{W}x{H} (host rectify_images resizes)")
            maps = self._rect_cache.get_maps(p['cam_matrix_L'], p['cam_matrix_R'], p['baseline'], W, H,
                                             p.get('dist_coeff_L'), p.get('dist_coeff_R'), p.get('rotation'),
                                             p.get('translation'), 1.0)
            if self._dev_maps is None or self._dev_maps[0] is not maps or self._dev_maps[1] != left.device:
                dm = tuple(torch.from_numpy(maps[k]).to(left.device) for k in ('map1_L', 'map2_L', 'map1_R', 'map2_R'))
                self._dev_maps = (maps, left.device, dm)
            m1L, m2L, m1R, m2R = self._dev_maps[2]
            return rectify_device(left, m1L, m2L, stream=stream), rectify_device(right, m1R, m2R, stream=stream)
        return rectify_device(left, stream=stream), rectify_device(right, stream=stream)

    def estimate_depth_device(self, left_source, right_source, stream=None, input_scale=None):
        """``estimate_depth`` (stereo_core.py:274-293) with every step on the device: raw uint8
        HIP frames -> rectify / gray -> matcher -> crop + median (+ depth).  Returns HIP tensors.

        ``input_scale``: the frames arrive at full size and the input downscale (input.py:38-43,
        ``resize_area``) runs on the device first, fused with the gray conversion for BGR frames - one
        kernel instead of resize + gray; with a calibration the rectification then remaps the gray image.
        Equal bit for bit to passing ``resize_area(frame, input_scale)``."""
        if left_source is None or right_source is None:
            raise ValueError("Left and right sources must be set before estimating depth.")
        full_guide = left_source if self._upsample_on(input_scale) else None
        if input_scale is not None and input_scale != 1.0:
            left_source = resize_area_device(left_source, input_scale, gray=left_source.dim() == 3, stream=stream)
            right_source = resize_area_device(right_source, input_scale, gray=right_source.dim() == 3, stream=stream)
        self.left_rectified, self.right_rectified = self._prepare_rectified_device(left_source, right_source, stream)
        return self.process_pair_device(self.left_rectified, self.right_rectified, stream=stream, full_guide=full_guide)

    def process_pair_device(self, left, right, stream=None, full_guide=None):
        """Device-resident ``_process_pair`` (stereo_core.py:162-200) for rectified uint8 HIP
        tensors: matcher -> crop -> post-processing -> depth, all in HBM.  Fast mode: 3x3 median
        (SURVEY.md 8f row F1); otherwise speckle filter + outlier removal (+ hole filling
        with ``hole_filling``, by ``fill_method``; + the guided weighted median with ``refine``, guided
        by ``left``) + median (row F2).  Returns float32 HIP tensors
        (disparity_px, depth_m or None).  ``full_guide``: the full-size left frame (uint8, H x W or H x W x 3) of a
        call with ``input_scale`` and 'upsample': 'joint': the chain and the temporal filter then run without
        depth scalars, and the upsampling launch writes the full-size disparity and the depth."""
        p = self.sgbm_params
        self._upsampled = full_guide is not None
        if full_guide is not None:
            d, _ = self._process_pair_lowres_device(left, right, stream, None, None)
            return joint_upsample_device(d, min(p['num_disp'], left.shape[1]), left, full_guide, stream=stream,
                                         **self._upsample_kwargs(), **self._depth_kwargs())
        return self._process_pair_lowres_device(left, right, stream, p.get('focal_length'), p.get('baseline'))

    def _process_pair_lowres_device(self, left, right, stream, f, B):
        """``process_pair_device`` at the matcher's resolution (depth when ``f`` and ``B``)."""
        p = self.sgbm_params
        doffs, eps, max_depth = p.get('doffs', 0.0), p.get('min_disp', 5.0), p.get('max_depth')
        fill = bool(p.get('hole_filling', False)) and not self.fast_mode
        method = p.get('fill_method', 'inpaint')
        timed = fill and method == 'inpaint'  # only Telea's persistent launch can time out
        want_conf = bool(p.get('confidence', False)) and 'compute_disparity_device' not in self.__dict__
        self.confidence_map = None
        if self._temporal is not None:
            # the chain runs without depth scalars and the filter's launch writes the depth of the filtered map
            # (no depth map is computed twice); the map is filtered in place
            d, _ = self._chain_device(left, right, stream, want_conf, method, timed, None, None)
            if d.shape[1] == 0:
                return d, (d.clone() if f is not None and B is not None else None)
            filt = self._temporal.device_filter(left.get_device())
            return filt.run(d, left[:, p['num_disp']:], out=d, focal_length=f, baseline=B, doffs=doffs, eps=eps,
                            max_depth=max_depth, stream=stream)
        return self._chain_device(left, right, stream, want_conf, method, timed, f, B)

    def _chain_device(self, left, right, stream, want_conf, method, timed, f, B):
        """The per-frame chain of ``process_pair_device`` up to the mode's tail (depth when ``f`` and ``B``)."""
        p = self.sgbm_params
        doffs, eps, max_depth = p.get('doffs', 0.0), p.get('min_disp', 5.0), p.get('max_depth')
        if not want_conf and 'compute_disparity_device' not in self.__dict__ and self.sgbm is not None and \
                getattr(self.sgbm, 'process_pair_device', None) is not None and \
                getattr(self.sgbm, 'params', {}).get('float_mode', 'fixed') == 'fixed':
            # one C-ABI call per frame (dsx_process_pair_device): the handle owns the float map and
            # the post-processing workspace, and the hole filling's timeout flag
            self._fill_check = self.sgbm.fill_status if timed else None
            return self.sgbm.process_pair_device(
                left, right, fast_mode=self.fast_mode, max_speckle_size=int(100 * self.downscale_factor),
                max_diff=1.0, apply_outlier_removal=True, outlier_threshold=2.5, outlier_kernel=5,
                fill_radius=3 if p.get('hole_filling', False) else 0, focal_length=f, baseline=B, doffs=doffs,
                eps=eps, max_depth=max_depth, stream=stream, fill_method=method, **self._refine_kwargs())
        if want_conf:
            # the map comes with the matcher call: the two-step route (compute_device, then the post-processing)
            import torch
            if self.sgbm is None:
                self._build_sgbm()
            disp = torch.empty(left.shape, dtype=torch.float32, device=left.device)
            conf = torch.empty(left.shape, dtype=torch.uint8, device=left.device)
            self.sgbm.compute_device(left, right, out_float=disp, stream=stream, out_confidence=conf)
            self.confidence_map = conf[:, p['num_disp']:]
        else:
            disp = self.compute_disparity_device(left, right, stream=stream)
        self._fill_check = None
        if self.fast_mode:
            return postprocess_fast_device(disp, p['num_disp'], f, B, doffs, eps, max_depth, stream=stream)
        # fill_kernel 3: postprocess_disparity's default as _process_pair calls it (postprocess.py:165)
        if timed:
            ws = default_workspace(disp.device, stream, "post")
            self._fill_check = lambda: fill_holes_status(ws)
        return postprocess_full_device(disp, p['num_disp'], max_speckle_size=int(100 * self.downscale_factor),
                                       max_diff=1.0, apply_outlier_removal=True, outlier_threshold=2.5,
                                       outlier_kernel=5, focal_length=f, baseline=B, doffs=doffs, eps=eps,
                                       max_depth=max_depth, stream=stream,
                                       apply_hole_filling=bool(p.get('hole_filling', False)), fill_kernel=3,
                                       fill_method=method, guide=left, **self._refine_kwargs())

    def disparity_to_depth(self, disp: np.ndarray, f_pixels: float, baseline_m: float, doffs: float = 0.0,
                           eps: float = 1e-6, max_depth: Optional[float] = None) -> np.ndarray:
        """stereo_core.py:234-272: Z = f*B / (d + doffs) where d + doffs > eps, else inf;
        optional clamp to max_depth."""
        adjusted_disp = disp + doffs
        Z = np.full_like(disp, np.inf, dtype=np.float32)
        valid_mask = adjusted_disp > eps
        Z[valid_mask] = (f_pixels * baseline_m) / adjusted_disp[valid_mask]
        if max_depth is not None:
            Z[Z > max_depth] = max_depth
        return Z

    # -- point cloud ---------------------------------------------------------------------
    def resolve_principal_point(self, height: int, width: int) -> Tuple[float, float]:
        """(cx, cy) of the left rectified image, ``height`` x ``width`` uncropped: the 'principal_point' key;
        else, with a full calibration, (P1[0, 2], P1[1, 2]) of the stereo_rectify call behind the
        rectification maps (computed once per calibration); else the image centre."""
        p = self.sgbm_params
        if p.get('principal_point') is not None:
            cx, cy = p['principal_point']
            return float(cx), float(cy)
        if all(p.get(k) is not None for k in _CALIBRATION_KEYS):
            args = (p['cam_matrix_L'], p['cam_matrix_R'], p['baseline'], p['image_width'], p['image_height'],
                    p.get('dist_coeff_L'), p.get('dist_coeff_R'), p.get('rotation'), p.get('translation'), 1.0)
            key = self._rect_cache._make_key(*args)
            if self._pp_cache is None or self._pp_cache[0] != key:
                self._pp_cache = (key, rectified_principal_point(*args))
            return self._pp_cache[1]
        return (width - 1) / 2.0, (height - 1) / 2.0

    def _cloud_kwargs(self, height: int, width: int) -> dict:
        """The reprojection of a cropped ``height`` x ``width`` map of this core, as the depth call passes it:
        x0 = num_disp, eps = min_disp; focal length, baseline, doffs and max_depth from the params."""
        p = self.sgbm_params
        f, B = p.get('focal_length'), p.get('baseline')
        if f is None or B is None:
            raise ValueError("A point cloud needs 'focal_length' and 'baseline' (configure_sgbm).")
        x0 = int(p['num_disp'])
        return dict(focal_length=f, baseline=B, principal_point=self.resolve_principal_point(height, x0 + width),
                    doffs=p.get('doffs', 0.0), eps=p.get('min_disp', 5.0), max_depth=p.get('max_depth'), x0=x0)

    def _refuse_upsampled_cloud(self) -> None:
        if self._upsampled:
            raise ValueError("point_cloud cannot reproject an upsampled frame: its intrinsics and crop are the "
                             "low-resolution ones (run with 'upsample': 'none' for a cloud)")

    def point_cloud(self, colors=None):
        """The last frame's ``disparity_map`` as a point cloud: ``(points, colors, index)`` host arrays -
        float32 N x 3 metric XYZ (x right, y down, z forward) of the valid pixels in row-major order, uint8
        N x 3 RGB, int32 N ``y * W + x`` into the cropped map (to gather ``confidence_map`` or anything else).
        ``colors``: an uncropped uint8 image, H x W_full x 3 BGR or H x W_full gray; None: ``left_rectified``.
        The device compacts the cloud (matcher.point_cloud_device) when the matcher has not been replaced
        (no ``compute_disparity`` override) and a HIP device is there - a rule of its own, looser than
        ``_device_pipeline_ok``: the map is a finished host array whatever produced it.  Otherwise the host
        restatement (pointcloud.point_cloud) runs; the arrays are the same either way.  This path is not
        device-resident: the host ``disparity_map`` that ``estimate_depth`` copied back is uploaded again and
        the cloud comes back over PCIe (only the rectified left image of a device frame is reused in HBM).
        Callers that keep frames on the device use ``point_cloud_device``."""
        disp = self.disparity_map
        if disp is None:
            raise ValueError("No frame has been processed: call estimate_depth first.")
        self._refuse_upsampled_cloud()
        disp = np.asarray(disp, np.float32)
        H, W = disp.shape
        kw = self._cloud_kwargs(H, W)
        on_device = 'compute_disparity' not in self.__dict__ and self._torch_device_ok()
        if colors is None:
            left = self.__dict__.get("_left_rect")
            # the device pipeline's rectified image is still in HBM: no copy back just to send it again
            colors = left.t if on_device and isinstance(left, _HostView) else self.left_rectified
        if colors is not None and not hasattr(colors, "is_cuda"):
            colors = np.asarray(colors)
        if colors is not None and tuple(colors.shape[:2]) != (H, kw['x0'] + W):
            raise ValueError("colors must be a uint8 image of the uncropped frame's size")
        if not on_device:
            if hasattr(colors, "is_cuda"):
                colors = colors.cpu().numpy()
            return host_point_cloud(disp, colors=colors, **kw)
        import torch
        dev = torch.device("cuda", int(self.sgbm_params.get('device', 0)))
        if colors is not None:
            colors = colors.to(dev) if hasattr(colors, "is_cuda") else torch.from_numpy(np.ascontiguousarray(colors)).to(dev)
        pts, col, idx = point_cloud_device(torch.from_numpy(np.ascontiguousarray(disp)).to(dev), colors=colors, **kw)
        return pts.cpu().numpy(), None if col is None else col.cpu().numpy(), idx.cpu().numpy()

    def point_cloud_device(self, disp, colors=None, stream=None, sync=True):
        """``point_cloud`` for the tensors of ``estimate_depth_device`` / ``process_pair_device``: ``disp`` the
        cropped float32 disparity tensor, ``colors`` an uncropped uint8 tensor on its device (None: the
        rectified left image of the last device frame, if it has the frame's size).  Returns what
        matcher.point_cloud_device returns: with ``sync`` the exact-length tensors, without it the
        full-capacity tensors and the count tensor, with no host synchronisation."""
        self._refuse_upsampled_cloud()
        H, W = disp.shape
        kw = self._cloud_kwargs(H, W)
        if colors is None:
            v = self.__dict__.get("_left_rect")
            v = v.t if isinstance(v, _HostView) else v
            if hasattr(v, "is_cuda") and v.is_cuda and v.device == disp.device and \
                    tuple(v.shape[:2]) == (H, kw['x0'] + W):
                colors = v
        return point_cloud_device(disp, colors=colors, stream=stream, sync=sync, **kw)

    @staticmethod
    def _torch_device_ok() -> bool:
        try:
            import torch
        except ImportError:  # pragma: no cover - torch is part of the image
            return False
        return torch.cuda.is_available()

    def estimate_depth(self, left_source, right_source, input_scale=None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """stereo_core.py:274-293.  Host arrays in, host arrays out; the work runs on the
        device pipeline (``estimate_depth_device``: rectify / gray, matcher, post-processing,
        depth, all in HBM - bit-identical to the host steps, tests/test_gpu_host_api.py) unless
        the matcher was replaced.

        ``input_scale``: full-size frames in, downscaled by that factor on the device first
        (``estimate_depth_device``); where the device pipeline does not apply to the downscaled shape,
        the host ``resize_area`` and the host path run instead - the same result either way."""
        if left_source is None or right_source is None:
            raise ValueError("Left and right sources must be set before estimating depth.")
        if input_scale is not None and input_scale == 1.0:
            input_scale = None
        if input_scale is not None and not self._device_pipeline_ok(left_source, right_source, input_scale):
            if self._upsample_on(input_scale):
                self.left_rectified, self.right_rectified = self._prepare_rectified(
                    resize_area(np.ascontiguousarray(left_source), input_scale),
                    resize_area(np.ascontiguousarray(right_source), input_scale))
                return self._process_pair(self.left_rectified, self.right_rectified,
                                          full_guide=np.ascontiguousarray(left_source))
            return self.estimate_depth(resize_area(np.ascontiguousarray(left_source), input_scale),
                                       resize_area(np.ascontiguousarray(right_source), input_scale))
        if self._device_pipeline_ok(left_source, right_source, input_scale):
            import torch
            dev = torch.device("cuda", int(self.sgbm_params.get('device', 0)))
            tl = torch.from_numpy(np.require(left_source, requirements=('C', 'W'))).to(dev)
            tr = torch.from_numpy(np.require(right_source, requirements=('C', 'W'))).to(dev)
            d, z = self.estimate_depth_device(tl, tr, input_scale=input_scale)
            self.left_rectified = _HostView(self.left_rectified)
            self.right_rectified = _HostView(self.right_rectified)
            self.disparity_map = d.cpu().numpy()
            self.depth_map = None if z is None else z.cpu().numpy()
            if self.confidence_map is not None:  # host arrays in, host arrays out
                self.confidence_map = self.confidence_map.cpu().numpy()
            self.check_fill_status()  # the copies above waited for the march: a timed-out fill raises
            return self.disparity_map, self.depth_map
        self.left_rectified, self.right_rectified = self._prepare_rectified(left_source, right_source)
        return self._process_pair(self.left_rectified, self.right_rectified)

    def check_fill_status(self) -> None:
        """Raise RuntimeError if the hole filling of this core's last device frame timed out (its
        holes were left unfilled): the matcher handle's flag (one-call path) or the post-processing
        workspace's (two-step path).  Call it once the frame's stream has finished."""
        chk = getattr(self, '_fill_check', None)
        if chk is not None:
            chk()

    def _device_pipeline_ok(self, left, right, input_scale=None) -> bool:
        if 'compute_disparity' in self.__dict__:
            return False
        if not (isinstance(left, np.ndarray) and isinstance(right, np.ndarray)):
            return False
        if left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim not in (2, 3) or left.shape != right.shape:
            return False
        if left.ndim == 3 and left.shape[2] != 3:
            return False
        p = self.sgbm_params
        if all(p.get(k) is not None for k in ('cam_matrix_L', 'cam_matrix_R', 'baseline', 'image_width', 'image_height')):
            hw = tuple(left.shape[:2]) if input_scale is None else (int(left.shape[0] * input_scale),
                                                                    int(left.shape[1] * input_scale))
            if hw != (int(p['image_height']), int(p['image_width'])):
                return False  # rectify_images' resize-on-mismatch path (rectify.py:92-105) is host-side
        try:
            import torch
        except ImportError:  # pragma: no cover - torch is part of the image
            return False
        return torch.cuda.is_available()
