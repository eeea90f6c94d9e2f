"""Host restatements of the matcher prefilter and the texture threshold (include/dsx.h
``dsx_prefilter``; the device kernels in csrc/dsx_prefilter.hip equal them bit for bit).

cv2.StereoBM carries a prefilter in front of its SAD search and a texture threshold behind it; the
forms here are this build's own integer definitions (parity with OpenCV unpinned).  With ``c`` the
cap in [1, 63] and cx / cy the replicate clamp into the image:

  xsobel : P(x, y) = clip(Sx, -c, c) + c with the x-Sobel
           Sx = 2 (I(x+1, y) - I(x-1, y)) + I(x+1, cy(y-1)) - I(x-1, cy(y-1)) + I(x+1, cy(y+1)) - I(x-1, cy(y+1));
           columns 0 and W-1 hold c.
  mean   : S(x, y) = sum of I(cx(x+i), cy(y+j)) over |i|, |j| <= n // 2 (n odd, 5..21),
           mu = (S + n*n // 2) // (n*n),  P = clip(I - mu, -c, c) + c.
  texture: T(x, y) = sum of |P(cx(x+i), cy(y+j)) - c| over |i|, |j| <= block_size // 2;
           a pixel with T < t gets the matcher's invalid value (min_disp - 1) * 16.

Both filters return uint8 in [0, 2c].
"""
from __future__ import annotations

import numpy as np

__all__ = ["prefilter_xsobel", "prefilter_mean", "texture_sum", "apply_texture_threshold", "prefilter"]


def _gray(img):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 2 or a.size == 0:
        raise ValueError("image must be a non-empty uint8 H x W array")
    return a


def _cap(cap) -> int:
    c = int(cap)
    if not 1 <= c <= 63:
        raise ValueError("prefilter cap must be in [1, 63]")
    return c


def _box_sum(a, n: int):
    """Sum of ``a`` (int64 H x W) over the n x n window with replicate-clamped coordinates."""
    H, W = a.shape
    r = n // 2
    p = a[np.clip(np.arange(-r, H + r), 0, H - 1)][:, np.clip(np.arange(-r, W + r), 0, W - 1)]
    S = np.zeros((H + 2 * r + 1, W + 2 * r + 1), np.int64)
    S[1:, 1:] = p.cumsum(0).cumsum(1)
    return S[n:, n:] - S[:-n, n:] - S[n:, :-n] + S[:-n, :-n]


def prefilter_xsobel(img, cap: int = 31) -> np.ndarray:
    I = _gray(img).astype(np.int64)
    c = _cap(cap)
    H, W = I.shape
    up = I[np.maximum(np.arange(H) - 1, 0)]
    dn = I[np.minimum(np.arange(H) + 1, H - 1)]
    P = np.full((H, W), c, np.int64)
    if W >= 3:
        sx = 2 * (I[:, 2:] - I[:, :-2]) + (up[:, 2:] - up[:, :-2]) + (dn[:, 2:] - dn[:, :-2])
        P[:, 1:W - 1] = np.clip(sx, -c, c) + c
    return P.astype(np.uint8)


def prefilter_mean(img, size: int = 9, cap: int = 31) -> np.ndarray:
    I = _gray(img).astype(np.int64)
    c, n = _cap(cap), int(size)
    if n % 2 == 0 or not 5 <= n <= 21:
        raise ValueError("prefilter size must be odd and in [5, 21]")
    mu = (_box_sum(I, n) + (n * n) // 2) // (n * n)
    return (np.clip(I - mu, -c, c) + c).astype(np.uint8)


def prefilter(img, prefilter_type: str = "xsobel", prefilter_size: int = 9, prefilter_cap: int = 31) -> np.ndarray:
    """The filter by its name ('none' returns the image)."""
    if prefilter_type == "none":
        return _gray(img)
    if prefilter_type == "xsobel":
        return prefilter_xsobel(img, prefilter_cap)
    if prefilter_type == "mean":
        return prefilter_mean(img, prefilter_size, prefilter_cap)
    raise ValueError("prefilter_type must be 'none', 'xsobel' or 'mean'")


def texture_sum(pref, block_size: int, cap: int = 31) -> np.ndarray:
    """T of a prefiltered image: uint16 H x W."""
    P = _gray(pref).astype(np.int64)
    c, k = _cap(cap), int(block_size)
    if k % 2 == 0 or not 1 <= k <= 15:
        raise ValueError("block_size must be odd and in [1, 15]")
    return _box_sum(np.abs(P - c), k).astype(np.uint16)


def apply_texture_threshold(fixed, T, t: int, min_disp: int = 0) -> np.ndarray:
    """The int16 x16 map with (min_disp - 1) * 16 wherever T < t (t = 0: unchanged)."""
    fixed = np.asarray(fixed)
    out = fixed.copy()
    out[np.asarray(T).astype(np.int64) < int(t)] = (int(min_disp) - 1) * 16
    return out
