"""Point-cloud output: a finished disparity map to metric XYZ (+ RGB), on the host.

This is the restatement of the device calls ``dsx_reproject_device`` / ``dsx_point_cloud_device``
(include/dsx.h, csrc/dsx_cloud.hip): the device results equal these bit for bit, the number and the order of
the points included.  An addition of this build: parity with nothing outside this repository is claimed.

The arithmetic (the contract).  ``d`` is a float32 H x W map whose column 0 is image column ``x0`` (the crop:
``num_disp`` for StereoCore's maps).  Everything is float32, every operation correctly rounded, no FMA::

    fB  = float32(float64(f) * float64(B))           # the depth map's own constant
    adj = d + float32(doffs)
    Z   = fB / adj
    valid = (adj > float32(eps)) and (0 < Z < inf) and (max_depth is None or Z <= float32(max_depth))
    s   = Z / float32(f)
    X   = (float32(x + x0) - float32(cx)) * s
    Y   = (float32(y)      - float32(cy)) * s

NaN compares false, so NaN disparities are invalid.  Axes are cv2's: x right, y down, z forward.  Points
beyond ``max_depth`` are dropped (the depth map clamps them instead); a valid point's ``Z`` has the depth
map's bits wherever that depth is below ``max_depth``.  Results in the denormal range are outside the contract.
"""
from __future__ import annotations

import math

import numpy as np


def _principal_point(principal_point, H, W, x0):
    """(cx, cy) in uncropped image coordinates; None: the centre of the uncropped image."""
    if principal_point is None:
        return (x0 + W - 1) / 2.0, (H - 1) / 2.0
    cx, cy = principal_point
    return float(cx), float(cy)


def check_cloud_params(focal_length, baseline, cx, cy, doffs, eps, max_depth, x0):
    """The rules of dsx_check_cloud (include/dsx.h) on the host: ValueError for a value it refuses."""
    if focal_length is None or baseline is None:
        raise ValueError("a point cloud needs focal_length and baseline")
    f = np.float32(focal_length)
    with np.errstate(all="ignore"):
        fB = np.float32(np.float64(focal_length) * np.float64(baseline))
    if not (f > 0 and np.isfinite(f)):
        raise ValueError("focal_length must be > 0 and finite")
    if not np.isfinite(fB) or fB == 0:
        raise ValueError("baseline must be finite and != 0")
    if not all(math.isfinite(np.float32(v)) for v in (cx, cy, doffs, eps)):
        raise ValueError("the principal point, doffs and eps must be finite")
    if max_depth is not None and not np.float32(max_depth) > 0:
        raise ValueError("max_depth must be > 0")
    if isinstance(x0, (bool, np.bool_)) or int(x0) != x0 or int(x0) < 0:
        raise ValueError("x0 must be an integer >= 0")


def reproject_disparity(disp, focal_length, baseline, principal_point=None, doffs=0.0, eps=1e-6, max_depth=None,
                        x0=0):
    """The organized cloud of a float32 H x W disparity map: ``(xyz, valid)`` with ``xyz`` float32 H x W x 3
    (all three components NaN at invalid pixels) and ``valid`` the bool H x W mask.  ``principal_point``:
    (cx, cy) in UNCROPPED image coordinates, None for the centre ((x0 + W - 1) / 2, (H - 1) / 2)."""
    d = np.asarray(disp)
    if d.ndim != 2:
        raise ValueError("disp must be an H x W map")
    d = d.astype(np.float32, copy=False)
    H, W = d.shape
    doffs = 0.0 if doffs is None else doffs
    cx, cy = _principal_point(principal_point, H, W, x0)
    check_cloud_params(focal_length, baseline, cx, cy, doffs, eps, max_depth, x0)
    x0 = int(x0)
    f = np.float32(focal_length)
    fB = np.float32(np.float64(focal_length) * np.float64(baseline))
    with np.errstate(all="ignore"):
        adj = d + np.float32(doffs)
        Z = fB / adj
        valid = (adj > np.float32(eps)) & (Z > np.float32(0.0)) & (Z < np.float32(np.inf))
        if max_depth is not None:
            valid &= Z <= np.float32(max_depth)
        s = Z / f
        xs = (np.arange(W, dtype=np.int64) + x0).astype(np.float32) - np.float32(cx)
        ys = np.arange(H, dtype=np.int64).astype(np.float32) - np.float32(cy)
        xyz = np.empty((H, W, 3), np.float32)
        xyz[..., 0] = xs[None, :] * s
        xyz[..., 1] = ys[:, None] * s
        xyz[..., 2] = Z
    xyz[~valid] = np.float32(np.nan)
    return xyz, valid


def cloud_colors(colors, H, W, x0=0):
    """The RGB uint8 H x W x 3 colours of a map's pixels from the UNCROPPED uint8 image ``colors``:
    H x (x0 + W) x 3 BGR (channels swapped) or H x (x0 + W) gray (replicated), read from column x0 on."""
    c = np.asarray(colors)
    if c.dtype != np.uint8 or c.ndim not in (2, 3) or (c.ndim == 3 and c.shape[2] != 3) or \
            c.shape[:2] != (H, int(x0) + W):
        raise ValueError("colors must be a uint8 H x (x0 + W) gray or H x (x0 + W) x 3 BGR image")
    c = c[:, int(x0):]
    if c.ndim == 2:
        return np.repeat(c[..., None], 3, axis=2)
    return c[..., ::-1]


def point_cloud(disp, focal_length, baseline, principal_point=None, doffs=0.0, eps=1e-6, max_depth=None, x0=0,
                colors=None):
    """The compact cloud: ``(points, colors or None, index)`` - the valid points of ``reproject_disparity`` in
    row-major pixel order as float32 N x 3, their uint8 N x 3 RGB colours when ``colors`` (see
    ``cloud_colors``) is given, and int32 N ``y * W + x`` per point."""
    xyz, valid = reproject_disparity(disp, focal_length, baseline, principal_point, doffs, eps, max_depth, x0)
    H, W = valid.shape
    rgb = None if colors is None else np.ascontiguousarray(cloud_colors(colors, H, W, x0)[valid])
    return np.ascontiguousarray(xyz[valid]), rgb, np.flatnonzero(valid).astype(np.int32)


def write_ply(path, points, colors=None) -> None:
    """Binary little-endian PLY: ``float x y z`` and, with ``colors`` (uint8 N x 3 RGB), ``uchar red green blue``."""
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(pts)}",
            "property float x", "property float y", "property float z"]
    if colors is not None:
        col = np.asarray(colors)
        if col.dtype != np.uint8 or col.shape != pts.shape:
            raise ValueError("colors must be uint8 N x 3, one per point")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    rec = np.empty(len(pts), dtype=np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if colors is not None:
        rec["red"], rec["green"], rec["blue"] = col[:, 0], col[:, 1], col[:, 2]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\nend_header\n").encode("ascii"))
        fh.write(rec.tobytes())


def read_ply(path):
    """Read back what ``write_ply`` writes: ``(points float32 N x 3, colors uint8 N x 3 or None)``."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("not a PLY file")
    head = data[:end].decode("ascii").split("\n")
    if "format binary_little_endian 1.0" not in head:
        raise ValueError("only binary little-endian PLY is read")
    n = next(int(line.split()[2]) for line in head if line.startswith("element vertex "))
    props = [line.split()[1:] for line in head if line.startswith("property ")]
    want = [["float", "x"], ["float", "y"], ["float", "z"]]
    rgb = [["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    if props not in (want, want + rgb):
        raise ValueError("unexpected PLY properties (write_ply's layouts are read)")
    fields = [(name, "<f4" if t == "float" else "u1") for t, name in props]
    rec = np.frombuffer(data, dtype=np.dtype(fields), count=n, offset=end + len(b"end_header\n"))
    pts = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32) if n else np.empty((0, 3), np.float32)
    if len(props) == 3:
        return pts, None
    col = np.stack([rec["red"], rec["green"], rec["blue"]], axis=1) if n else np.empty((0, 3), np.uint8)
    return pts, col
