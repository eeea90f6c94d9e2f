"""Full-resolution output for downscaled runs: the host restatement of dsx_upsample / dsx_upsample_device
(include/dsx.h, csrc/dsx_upsample.hip), equal to the device bit for bit.

A run with an input downscale (``downscale_factor`` / ``input_scale``) matches at ``h x Wl`` pixels.  The joint
bilateral upsampling brings its finished map ``d`` (``h x w``, column 0 = low-resolution column ``x0``) back to
the ``H x W`` frame the caller holds, guided by that frame ``G`` and by the low-resolution image ``g`` the
matcher ran on.  Per axis, with hi-res size I and low-res size O <= I, in integers:

    near(X) = ((2X + 1) O) // (2 I)                      the low-res pixel whose cell contains hi-res centre X
    tap k = near(X) + t - r, t = 0..2r;  n = |(2X + 1) O - (2k + 1) I|
    tent a(X, t) = max(0, 64 - ((64 n + (r + 1) I) // (2 (r + 1) I)))
    X0 = max(0, ceil((2 W x0 - Wl) / (2 Wl)))            the smallest X with near_x(X) >= x0

and per output pixel P = (X, Y), X = X0..W-1, over the (2r + 1)^2 taps (rows outer, columns inner) that lie
inside the map and are valid (0 < d < +inf):

    W_q = a_x a_y T[|G(P) - g(q)|]                         T = postprocess.wmedian_weights(sigma)
    m   = the smallest tap value v with 2 sum(W_q : d_q <= v) >= S,  S = sum of the W_q
    a   = (sum of float32(W_q) * d_q over |d_q - m| <= max_diff, in window order) / float32(sum of those W_q)
    out = a * float32(W / Wl);   depth = fB / (a + doffs) where a + doffs > eps, else inf, clamped to max_depth

every float32 operation rounded once.  Where no tap is valid the output keeps the bits of the centre tap
``d[near_y(Y), near_x(X) - x0]``, unscaled, and the depth rule is applied to that value.

``joint_upsample`` is the vectorised form; ``nearest_upsample`` is the plain nearest-neighbour map
(``d[near_y][near_x] * sx``) it is measured against.
"""
from __future__ import annotations

import numpy as np

from .postprocess import wmedian_weights

UPSAMPLE_DEFAULTS = {"radius": 1, "sigma": 8, "max_diff": 1.0}
MAX_DIM = 32768

_CHUNK = 1 << 21  # window taps held at once by joint_upsample (rows are processed in strips)


def check_upsample(radius=1, sigma=8, max_diff=1.0):
    """The ranges of dsx_check_upsample; returns the values as (int, int, float32)."""
    def integer(v, lo, hi, name):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or \
                int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer in [{lo}, {hi}]")
        return int(v)
    radius = integer(radius, 1, 3, "radius")
    sigma = integer(sigma, 1, 64, "sigma")
    if isinstance(max_diff, (bool, np.bool_)) or not isinstance(max_diff, (int, float, np.integer, np.floating)):
        raise ValueError("max_diff must be a finite number > 0")
    with np.errstate(over="ignore"):
        md = np.float32(max_diff)  # rounded to float32 once
    if not np.isfinite(md) or not md > 0:
        raise ValueError("max_diff must be a finite number > 0")
    return radius, sigma, md


def upsample_taps(in_size: int, out_size: int, radius: int = 1):
    """(near, tent) of one axis: ``near`` int64 [in_size], ``tent`` int64 [in_size, 2 radius + 1]
    (dsx_upsample_taps).  ``in_size`` is the hi-res size I, ``out_size`` the low-res size O <= I."""
    I, O, r = int(in_size), int(out_size), int(radius)
    if not 1 <= O <= I <= MAX_DIM:
        raise ValueError("sizes must satisfy 1 <= out_size <= in_size <= 32768")
    if not 1 <= r <= 3:
        raise ValueError("radius must be in [1, 3]")
    X = np.arange(I, dtype=np.int64)
    p = (2 * X + 1) * O
    near = p // (2 * I)
    k = near[:, None] + np.arange(2 * r + 1, dtype=np.int64)[None, :] - r
    n = np.abs(p[:, None] - (2 * k + 1) * I)
    tent = np.maximum(0, 64 - (64 * n + (r + 1) * I) // (2 * (r + 1) * I))
    return near, tent


def upsample_x0(W: int, Wl: int, x0: int) -> int:
    """The first output column: the smallest X with near_x(X) >= x0 (dsx_upsample_x0)."""
    W, Wl, x0 = int(W), int(Wl), int(x0)
    if not (1 <= Wl <= W <= MAX_DIM and 0 <= x0 <= Wl):
        raise ValueError("bad W, Wl or x0")
    return max(0, -((Wl - 2 * W * x0) // (2 * Wl)))  # ceil of a quotient of integers


def guide_gray(G: np.ndarray) -> np.ndarray:
    """The gray value the kernel forms of a 3-channel guide, in memory order (rectify_device's formula)."""
    G = np.asarray(G)
    if G.ndim == 2:
        return G
    c = G.astype(np.int64)
    return ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def _inputs(disp, x0, guide_lo, guide):
    d = np.asarray(disp)
    g = np.asarray(guide_lo)
    G = np.asarray(guide)
    if d.dtype != np.float32 or d.ndim != 2:
        raise ValueError("disp must be a float32 h x w array")
    if g.dtype != np.uint8 or g.ndim != 2 or g.shape[0] != d.shape[0]:
        raise ValueError("guide_lo must be a uint8 h x Wl array (the uncropped low-resolution image)")
    if G.dtype != np.uint8 or G.ndim not in (2, 3) or (G.ndim == 3 and G.shape[2] not in (1, 3)):
        raise ValueError("guide must be a uint8 H x W or H x W x 3 array (the full-size frame)")
    if G.ndim == 3 and G.shape[2] == 1:
        G = G[..., 0]
    x0 = int(x0)
    h, w = d.shape
    Wl = g.shape[1]
    H, W = G.shape[:2]
    if x0 < 0 or x0 + w != Wl:
        raise ValueError("disp must cover the low-resolution columns x0 .. Wl - 1 (x0 + w == Wl)")
    if not (1 <= h <= H <= MAX_DIM and 1 <= Wl <= W <= MAX_DIM):
        raise ValueError("shapes must satisfy 1 <= h <= H <= 32768 and 1 <= Wl <= W <= 32768")
    return d, x0, g, G


def _depth(v, focal_length, baseline, doffs, eps, max_depth):
    """The depth map's own rule in float32 (dsx_postprocess_fast_device)."""
    fB = np.float32(float(focal_length) * float(baseline))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        adj = v + np.float32(doffs)
        z = np.where(adj > np.float32(eps), fB / adj, np.float32(np.inf)).astype(np.float32)
        if max_depth is not None:
            z[z > np.float32(max_depth)] = np.float32(max_depth)
    return z


def nearest_upsample(disp, x0, guide_lo_width, shape):
    """Nearest-neighbour upsampling of the same map to ``shape`` = (H, W): ``d[near_y][near_x - x0] * sx`` over
    the columns X0 .. W - 1 (what a caller resizing by hand gets; the baseline of the quality figures)."""
    d = np.asarray(disp, np.float32)
    H, W = shape
    Wl = int(guide_lo_width)
    X0 = upsample_x0(W, Wl, x0)
    ny, _ = upsample_taps(H, d.shape[0], 1)
    nx, _ = upsample_taps(W, Wl, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return d[ny[:, None], nx[None, X0:] - x0] * np.float32(W / Wl)


def joint_upsample(disp, x0, guide_lo, guide, radius=1, sigma=8, max_diff=1.0, focal_length=None, baseline=None,
                   doffs=0.0, eps=1e-6, max_depth=None):
    """The joint bilateral upsampling of the module docstring.  ``disp`` float32 h x w, ``guide_lo`` uint8
    h x Wl (uncropped, Wl = x0 + w), ``guide`` uint8 H x W or H x W x 3.  Returns ``(out, depth)``: float32
    H x (W - X0) each, ``depth`` None without ``focal_length`` and ``baseline``."""
    d, x0, g, G = _inputs(disp, x0, guide_lo, guide)
    r, sigma, md = check_upsample(radius, sigma, max_diff)
    h, w = d.shape
    Wl = g.shape[1]
    H, W = G.shape[:2]
    X0 = upsample_x0(W, Wl, x0)
    Wo = W - X0
    want_depth = focal_length is not None and baseline is not None
    out = np.zeros((H, max(Wo, 0)), np.float32)
    if w == 0 or Wo <= 0:
        return out, (out.copy() if want_depth else None)
    T = wmedian_weights(sigma).astype(np.int64)
    Gg = guide_gray(G)[:, X0:].astype(np.int64)
    ny, ay = upsample_taps(H, h, r)
    nx, ax = upsample_taps(W, Wl, r)
    nx, ax = nx[X0:], ax[X0:]
    sx = np.float32(W / Wl)
    bits = d.view(np.uint32)
    gl = g.astype(np.int64)
    n = 2 * r + 1
    depth = np.zeros((H, Wo), np.float32) if want_depth else None
    inf = np.float32(np.inf)
    rows = max(1, _CHUNK // (n * n * Wo))
    for y0 in range(0, H, rows):
        y1 = min(H, y0 + rows)
        R = y1 - y0
        dv = np.empty((n * n, R, Wo), np.float32)
        wv = np.empty((n * n, R, Wo), np.int64)
        gp = Gg[y0:y1]
        for j in range(n):
            y = ny[y0:y1] + j - r
            yin = (y >= 0) & (y < h)
            yc = np.clip(y, 0, h - 1)
            for i in range(n):
                x = nx + i - r
                xin = (x - x0 >= 0) & (x - x0 < w)
                xc = np.clip(x - x0, 0, w - 1)
                v = d[yc[:, None], xc[None, :]]
                with np.errstate(invalid="ignore"):
                    ok = yin[:, None] & xin[None, :] & (v > 0) & (v < inf)
                wq = ax[None, :, i] * ay[y0:y1, j, None] * T[np.abs(gp - gl[yc[:, None], xc[None, :] + x0])]
                dv[j * n + i] = np.where(ok, v, inf)
                wv[j * n + i] = np.where(ok, wq, 0)
        S = wv.sum(axis=0)
        # the selection: sorted by value, the first tap whose running weight reaches half of S (ties in value
        # give the same value wherever the running sum crosses inside them)
        order = np.argsort(dv, axis=0, kind="stable")
        ds = np.take_along_axis(dv, order, axis=0)
        cs = np.cumsum(np.take_along_axis(wv, order, axis=0), axis=0)
        first = np.argmax(2 * cs >= S[None], axis=0)
        m = np.take_along_axis(ds, first[None], axis=0)[0]
        # the gated average, in window order
        num = np.zeros((R, Wo), np.float32)
        den = np.zeros((R, Wo), np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            for p in range(n * n):
                inside = np.abs(dv[p] - m) <= md
                prod = wv[p].astype(np.float32) * np.where(inside, dv[p], np.float32(0))
                num = np.where(inside, num + prod, num)
                den += np.where(inside, wv[p], 0)
            a = num / np.maximum(den, 1).astype(np.float32)
            have = S > 0
            centre = bits[ny[y0:y1, None], nx[None, :] - x0]
            out.view(np.uint32)[y0:y1] = np.where(have, (a * sx).view(np.uint32), centre)
            if want_depth:
                val = np.where(have, a, centre.view(np.float32))
                depth[y0:y1] = _depth(val, focal_length, baseline, doffs, eps, max_depth)
    return out, depth
