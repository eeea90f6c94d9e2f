"""Seeded synthetic rectified stereo pairs.

The reference's sample pair (assets/stereo_pairs/im0.png, im1.png) is missing from the
checkout (.MISSING_LARGE_BLOBS:1-2), so every benchmark and parity input is synthetic:
R is a 3x3-box-smoothed uniform texture (unique SAD minima); L is R shifted right by a
ground-truth disparity field made of vertical bands of constant integer disparity in
[min_disp, min_disp + num_disp - 1] plus one slanted (sub-pixel) band, i.e.
L(x, y) = R(x - d_gt(x, y), y) - the convention of depthlib (left image = reference,
disparity = x_left - x_right).
"""
from __future__ import annotations

import numpy as np


def texture(H: int, W: int, rng: np.random.Generator) -> np.ndarray:
    t = rng.integers(0, 256, (H + 2, W + 2), dtype=np.int32)
    s = (t[:-2, :-2] + t[:-2, 1:-1] + t[:-2, 2:] + t[1:-1, :-2] + t[1:-1, 1:-1] + t[1:-1, 2:] +
         t[2:, :-2] + t[2:, 1:-1] + t[2:, 2:])
    return (s // 9).astype(np.uint8)


def stereo_pair(H: int, W: int, min_disp: int = 0, num_disp: int = 64, seed: int = 1234,
                bands: int = 6, slant: bool = True):
    """Returns (L, R, d_gt) with d_gt float32 H x W (ground-truth disparity)."""
    rng = np.random.default_rng(seed)
    R = texture(H, W, rng)
    lo, hi = min_disp, min_disp + max(num_disp - 1, 0)
    edges = np.linspace(0, W, bands + 1).astype(int)
    d_gt = np.zeros((H, W), np.float32)
    for b in range(bands):
        d_gt[:, edges[b]:edges[b + 1]] = float(rng.integers(lo, hi + 1))
    if slant and bands >= 2:
        # a slanted plane over the second band: disparity varies linearly along y
        x0, x1 = edges[1], edges[2]
        ramp = np.linspace(lo + 0.25 * (hi - lo), lo + 0.75 * (hi - lo), H, dtype=np.float32)
        d_gt[:, x0:x1] = ramp[:, None]
    xs = np.arange(W, dtype=np.float32)[None, :] - d_gt
    x0i = np.floor(xs).astype(np.int64)
    fr = xs - x0i
    a = np.take_along_axis(R, np.clip(x0i, 0, W - 1), 1).astype(np.float32)
    b = np.take_along_axis(R, np.clip(x0i + 1, 0, W - 1), 1).astype(np.float32)
    L = np.clip(np.rint(a * (1 - fr) + b * fr), 0, 255).astype(np.uint8)
    return L, R, d_gt


def binary_pair(H: int, W: int, min_disp: int = 0, num_disp: int = 64, seed: int = 1234):
    """``stereo_pair`` thresholded to {0, 255} (> 127 -> 255): every pixel difference is 0 or 255,
    so block costs reach 255 * bs^2 and SGM path costs climb towards max cost + P2."""
    L, R, d_gt = stereo_pair(H, W, min_disp, num_disp, seed=seed)
    return _threshold(L), _threshold(R), d_gt


STRIPE_COLS = 40


def striped_pair(H: int, W: int, min_disp: int = 0, num_disp: int = 64, seed: int = 1234):
    """``binary_pair`` whose first STRIPE_COLS columns hold period-2 vertical stripes (0, 255, 0,
    255, ...) in both images (L == R there).  Inside the stripes every odd shift costs 255 * bs^2 and
    every even shift 0 at every pixel (min_disp even), so with P1 = P2 the odd path costs grow by the
    full block cost per step until they sit exactly on max cost + P2."""
    L, R, d_gt = binary_pair(H, W, min_disp, num_disp, seed=seed)
    n = min(STRIPE_COLS, W)
    stripes = ((np.arange(n) & 1) * 255).astype(np.uint8)
    L[:, :n] = stripes
    R[:, :n] = stripes
    return L, R, d_gt


def _threshold(img: np.ndarray) -> np.ndarray:
    return np.where(img > 127, 255, 0).astype(np.uint8)


def layered_pair(H: int, W: int, num_disp: int = 32, seed: int = 1234, disparities=(6, 12, 7, 13, 8),
                 levels=(60, 200, 100, 240, 140), amplitude: int = 8):
    """An occlusion-correct layered scene: returns (L, R, d_gt), d_gt float32 H x W.

    The columns from ``num_disp`` on (what survives the drop-in crop) are split into len(disparities)
    vertical layers of equal width; layer i has the constant integer disparity ``disparities[i]`` and grey
    level ``levels[i]`` + a uniform texture in [-amplitude, amplitude]; the first layer also covers the
    columns left of ``num_disp``.  The right view is rendered far to near - every layer is shifted left by
    its disparity and nearer layers overwrite farther ones - so a foreground edge hides background in one
    view only, as a real scene does; right pixels that no layer reaches take their own texture around the
    mean level.  Depth edges coincide with grey-level edges: what an image-guided filter can use.  Keep the
    disparity jumps smaller than the radius of a filter that is to reach across the occlusion band."""
    if len(disparities) != len(levels) or not disparities:
        raise ValueError("disparities and levels must be non-empty sequences of equal length")
    if min(disparities) < 0 or max(disparities) >= max(int(num_disp), 1):
        raise ValueError("disparities must lie in [0, num_disp)")
    rng = np.random.default_rng(seed)
    n = len(disparities)
    a = int(amplitude)
    edges = (min(int(num_disp), W) + np.linspace(0, max(W - int(num_disp), 0), n + 1)).astype(int)
    edges[0] = 0
    edges[-1] = W
    L = np.zeros((H, W), np.int32)
    d_gt = np.zeros((H, W), np.float32)
    for i in range(n):
        x0, x1 = edges[i], edges[i + 1]
        L[:, x0:x1] = int(levels[i]) + rng.integers(-a, a + 1, (H, x1 - x0))
        d_gt[:, x0:x1] = float(disparities[i])
    L = np.clip(L, 0, 255).astype(np.uint8)
    R = np.clip(int(np.mean(levels)) + rng.integers(-a, a + 1, (H, W)), 0, 255).astype(np.uint8)
    for i in np.argsort(np.asarray(disparities), kind="stable"):  # far (small disparity) first
        x0, x1, d = edges[i], edges[i + 1], int(disparities[i])
        lo = max(x0, d)  # left columns whose right position x - d is inside the image
        if x1 > lo:
            R[:, lo - d:x1 - d] = L[:, lo:x1]
    return L, R, d_gt
