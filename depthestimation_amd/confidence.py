"""NumPy restatement of the matcher's confidence map (dsx_confidence of include/dsx.h; K2's confidence
variant in csrc/dsx_kernels.hip computes the same integers).

An addition of this build: parity with nothing outside this repository is claimed.  For an integer cost
volume C[y, x, d], d in [0, D) - block costs of any cost, or SGM path sums - let b be the lowest-d argmin,
cb = C[b], and nm the minimum of C over the disparities with |d - b| > 1 (the set the uniqueness test scans):

    q = 255                      if that set is empty (D <= 2, or D = 3 with b = 1),
    q = 0                        if nm == 0 (then cb == 0 too: a perfect tie),
    q = 255 - (255 * cb) // nm   otherwise (cb <= nm, so q lies in [0, 255]),
    q = 0                        outside the valid band of the handle's lr_form.

q describes the WTA decision alone.  Every in-band pixel that uniqueness_ratio u rejects has
q <= 255 - (255 * (100 - u)) // 100 (``uniqueness_bound``): C[d] (100 - u) < cb 100 for a far d gives
255 cb / nm > 255 (100 - u) / 100, and the floor keeps the order.
"""
from __future__ import annotations

import numpy as np

__all__ = ["peak_ratio", "apply_threshold", "uniqueness_bound", "valid_band"]


def valid_band(W: int, D: int, min_disp: int, lr_form: str = "bm"):
    """Boolean [W]: the columns of the valid band ('bm': [m + D - 1, W - 1 + m]; 'sgbm':
    [max(m + D, 0), W + min(m, 0)))."""
    if lr_form not in ("bm", "sgbm"):
        raise ValueError("lr_form must be 'bm' or 'sgbm'")
    x = np.arange(W)
    m = int(min_disp)
    if lr_form == "bm":
        return (x >= m + D - 1) & (x <= W - 1 + m)
    return (x >= max(m + D, 0)) & (x < W + min(m, 0))


def peak_ratio(C, min_disp: int, lr_form: str = "bm"):
    """uint8 H x W peak-ratio confidence of an integer volume C[y, x, d] (any integer dtype; non-negative)."""
    C = np.asarray(C)
    if C.ndim != 3 or not np.issubdtype(C.dtype, np.integer):
        raise ValueError("C must be an integer H x W x D volume")
    C = C.astype(np.int64)
    H, W, D = C.shape
    b = np.argmin(C, axis=2)
    cb = np.take_along_axis(C, b[..., None], 2)[..., 0]
    far = np.abs(np.arange(D)[None, None, :] - b[..., None]) > 1
    big = np.iinfo(np.int64).max
    nm = np.where(far, C, big).min(axis=2)
    empty = ~far.any(axis=2)
    den = np.where(empty | (nm == 0), 1, nm)
    q = 255 - (255 * cb) // den
    q = np.where(empty, 255, np.where(nm == 0, 0, q))
    q = np.where(valid_band(W, D, min_disp, lr_form)[None, :], q, 0)
    return q.astype(np.uint8)


def apply_threshold(disp, q, t: int, min_disp: int):
    """``disp`` (the int16 x16 map, or a float map) with the pixels of confidence q < t set to the invalid
    value: (min_disp - 1) * 16 in an integer map, min_disp - 1 in a float one.  t = 0 changes nothing."""
    disp = np.asarray(disp)
    q = np.asarray(q)
    if q.shape != disp.shape:
        raise ValueError("q must have the map's shape")
    if isinstance(t, bool) or int(t) != t or not 0 <= int(t) <= 255:
        raise ValueError("confidence_threshold must be an integer in [0, 255]")
    if np.issubdtype(disp.dtype, np.integer):
        inv = disp.dtype.type((int(min_disp) - 1) * 16)
    else:
        inv = disp.dtype.type(int(min_disp) - 1)
    return np.where(q < int(t), inv, disp).astype(disp.dtype)


def uniqueness_bound(u: int) -> int:
    """The largest q an in-band pixel rejected by uniqueness_ratio u can have."""
    return 255 - (255 * (100 - int(u))) // 100
