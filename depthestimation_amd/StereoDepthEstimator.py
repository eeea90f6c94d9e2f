"""StereoDepthEstimator facade (mirrors depthlib/StereoDepthEstimator.py:7-107).

Visualisation (matplotlib, StereoDepthEstimator.py:109-122) is outside the hot path and not
provided; everything else keeps the reference's names, arguments and errors.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from .input import load_stereo_pair
from .pointcloud import write_ply
from .stereo_core import StereoCore


class StereoDepthEstimator:
    """Depth from a still stereo pair."""

    def __init__(self, left_source=None, right_source=None, downscale_factor=1.0, device_downscale=False):
        if downscale_factor <= 0 or downscale_factor > 1.0:
            raise ValueError("downscale_factor must be between 0 and 1.")
        self.downscale_factor = downscale_factor
        # True: the pair is loaded at full size and downscaled on the GPU (StereoCore.estimate_depth's
        # input_scale) instead of by load_stereo_pair (input.py:38-43) - the same maps
        self.device_downscale = bool(device_downscale)
        self.core = StereoCore(downscale_factor=downscale_factor)
        self.left_source = None
        self.right_source = None
        if left_source is not None and right_source is not None:
            self.left_source, self.right_source = load_stereo_pair(
                left_source, right_source, downscale_factor=1.0 if self.device_downscale else downscale_factor)
        self.sgbm = None
        self.disparity_map = None
        self.depth_map = None

    def configure_sgbm(self, **kwargs):
        """StereoDepthEstimator.py:49-78 -> StereoCore.configure_sgbm."""
        self.core.configure_sgbm(**kwargs)

    def get_sgbm_params(self) -> Dict[str, int]:
        return self.core.get_sgbm_params()

    @property
    def confidence_map(self):
        """The last estimate's peak-ratio confidence map (uint8, cropped like the disparity) when
        ``configure_sgbm(confidence=True)``; None otherwise.  Read-only."""
        return self.core.confidence_map

    def estimate_depth(self) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """StereoDepthEstimator.py:90-107."""
        if self.left_source is None or self.right_source is None:
            raise ValueError("Left and right sources must be provided for depth estimation.")
        kw = {"input_scale": self.downscale_factor} if self.device_downscale else {}
        disparity_px, depth_m = self.core.estimate_depth(self.left_source, self.right_source, **kw)
        self.disparity_map = disparity_px
        self.depth_map = depth_m
        return disparity_px, depth_m

    def point_cloud(self, colors=None):
        """The last estimate as a point cloud (StereoCore.point_cloud): ``(points, colors, index)`` - float32
        N x 3 metric XYZ of the valid pixels in row-major order, uint8 N x 3 RGB (from the left rectified
        image unless ``colors`` is given), int32 N pixel indices into the disparity map.  An addition of this
        build; needs 'focal_length' and 'baseline'."""
        return self.core.point_cloud(colors=colors)

    def save_point_cloud(self, path, colors=None) -> int:
        """Write ``point_cloud()`` as a binary little-endian PLY (pointcloud.write_ply); returns the number of points."""
        points, rgb, _ = self.point_cloud(colors=colors)
        write_ply(path, points, rgb)
        return len(points)
