"""Temporal disparity filter for video: the host restatement of dsx_temporal_params / dsx_tfilter
(include/dsx.h, csrc/dsx_temporal.hip), equal to the device bit for bit on every frame.

A motion-gated recursive average with a temporal hole filler.  Per frame the filter takes the finished
float32 disparity map ``d`` (what ``StereoCore._process_pair`` produces) and the uint8 guide ``G`` over the same
pixels (the raw left rectified image from column num_disp on) and keeps, per pixel, the filtered disparity
``S``, its age ``n`` (0: no state), the count ``h`` of consecutive held frames and the previous guide ``P``.
With r = motion_radius, cx / cy the replicate clamp and every disparity operation a correctly rounded float32
one (no FMA):

    v      = 0 < d < +inf
    M      = sum over |i|, |j| <= r of |G(cx(x+i), cy(y+j)) - P(cx(x+i), cy(y+j))|
    static = there is a previous frame  and  M <= motion_threshold * (2r + 1)^2
    v and static and n > 0 and |d - S| <= max_diff:
             S' = S + (d - S) * A[n];  n' = min(n + 1, max_age);  h' = 0;  out = S'
    else v:  S' = d;  n' = 1;  h' = 0;  out = d (the input bits)
    else static and n > 0 and h < hold:
             out = S;  S and n kept;  h' = h + 1
    else:    out = d (the input bits);  S' = 0;  n' = 0;  h' = 0
    then P <- G

with the gains A[n] = float32(1.0 / (n + 1)) computed in doubles (``temporal_gains``).  The first frame, the
first frame after ``reset()`` and the first frame after a shape change have no previous frame.

``TemporalFilter`` is the vectorised form; ``TemporalFilterLoop`` is the same rule written pixel by pixel, kept
for the tests.
"""
from __future__ import annotations

import numpy as np

TEMPORAL_DEFAULTS = {"max_age": 4, "max_diff": 1.0, "motion_radius": 1, "motion_threshold": 6, "hold": 2}


def temporal_gains(max_age: int) -> np.ndarray:
    """A[0..max_age] as float32: A[0] = 0, A[n] = float32(1.0 / (n + 1)) from doubles (dsx_temporal_gains)."""
    if isinstance(max_age, (bool, np.bool_)) or int(max_age) != max_age or not 1 <= int(max_age) <= 64:
        raise ValueError("max_age must be an integer in [1, 64]")
    out = np.zeros(int(max_age) + 1, np.float32)
    for n in range(1, int(max_age) + 1):
        out[n] = np.float32(1.0 / float(n + 1))
    return out


def check_temporal(max_age=4, max_diff=1.0, motion_radius=1, motion_threshold=6, hold=2):
    """The ranges of dsx_check_temporal; returns the values as (int, float32, int, int, int)."""
    def integer(v, lo, hi, name):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or \
                int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"{name} must be an integer in [{lo}, {hi}]")
        return int(v)
    max_age = integer(max_age, 1, 64, "max_age")
    motion_radius = integer(motion_radius, 0, 2, "motion_radius")
    motion_threshold = integer(motion_threshold, 0, 255, "motion_threshold")
    hold = integer(hold, 0, 255, "hold")
    if isinstance(max_diff, (bool, np.bool_)) or not isinstance(max_diff, (int, float, np.integer, np.floating)):
        raise ValueError("max_diff must be a finite number > 0")
    with np.errstate(over="ignore"):
        md = np.float32(max_diff)  # rounded to float32 once
    if not np.isfinite(md) or not md > 0:
        raise ValueError("max_diff must be a finite number > 0")
    return max_age, md, motion_radius, motion_threshold, hold


def _inputs(disp, guide):
    d = np.asarray(disp)
    G = np.asarray(guide)
    if d.dtype != np.float32 or d.ndim != 2:
        raise ValueError("disp must be a float32 H x W array")
    if G.dtype != np.uint8 or G.shape != d.shape:
        raise ValueError("guide must be a uint8 array of disp's shape")
    return d, G


class TemporalFilter:
    """The vectorised restatement.  ``f(disp, guide) -> out`` filters one frame and advances the state;
    ``reset()`` forgets it."""

    def __init__(self, max_age=4, max_diff=1.0, motion_radius=1, motion_threshold=6, hold=2):
        self.max_age, self.max_diff, self.motion_radius, self.motion_threshold, self.hold = check_temporal(
            max_age, max_diff, motion_radius, motion_threshold, hold)
        self.gains = temporal_gains(self.max_age)
        self.reset()

    def reset(self) -> None:
        self.S = self.n = self.h = self.P = None

    def motion_sum(self, G: np.ndarray) -> np.ndarray:
        """M of the rule (int32 H x W) against the stored previous guide."""
        r = self.motion_radius
        ad = np.abs(G.astype(np.int32) - self.P.astype(np.int32))
        if r == 0:
            return ad
        H, W = ad.shape
        pad = np.pad(ad, r, mode="edge")
        M = np.zeros((H, W), np.int32)
        for j in range(2 * r + 1):
            for i in range(2 * r + 1):
                M += pad[j:j + H, i:i + W]
        return M

    def __call__(self, disp, guide) -> np.ndarray:
        d, G = _inputs(disp, guide)
        if self.S is None or self.S.shape != d.shape:  # no previous frame
            self.S = np.zeros(d.shape, np.float32)
            self.n = np.zeros(d.shape, np.uint8)
            self.h = np.zeros(d.shape, np.uint8)
            static = np.zeros(d.shape, bool)
        else:
            k = 2 * self.motion_radius + 1
            static = self.motion_sum(G) <= self.motion_threshold * k * k
        S, n, h = self.S, self.n, self.h
        with np.errstate(invalid="ignore", over="ignore"):
            v = (d > 0) & (d < np.inf)
            have = static & (n > 0)
            diff = d - S                                # float32
            agree = v & have & (np.abs(diff) <= self.max_diff)
            avg = S + diff * self.gains[n]              # two float32 operations, each rounded
        fresh = v & ~agree
        held = ~v & have & (h < self.hold)
        out = d.copy()
        out[agree] = avg[agree]
        out[held] = S[held]
        self.S = np.where(agree, avg, np.where(fresh, d, np.where(held, S, np.float32(0)))).astype(np.float32)
        self.n = np.where(agree, np.minimum(n.astype(np.int32) + 1, self.max_age),
                          np.where(fresh, 1, np.where(held, n, 0))).astype(np.uint8)
        self.h = np.where(held, h.astype(np.int32) + 1, 0).astype(np.uint8)
        self.P = G.copy()
        return out


class TemporalFilterLoop:
    """The same rule as a plain loop over the pixels (slow; the tests compare it with ``TemporalFilter``)."""

    def __init__(self, max_age=4, max_diff=1.0, motion_radius=1, motion_threshold=6, hold=2):
        self.max_age, self.max_diff, self.motion_radius, self.motion_threshold, self.hold = check_temporal(
            max_age, max_diff, motion_radius, motion_threshold, hold)
        self.gains = temporal_gains(self.max_age)
        self.reset()

    def reset(self) -> None:
        self.S = self.n = self.h = self.P = None

    def __call__(self, disp, guide) -> np.ndarray:
        d, G = _inputs(disp, guide)
        H, W = d.shape
        prev = self.S is not None and self.S.shape == d.shape
        if not prev:
            self.S = np.zeros((H, W), np.float32)
            self.n = np.zeros((H, W), np.uint8)
            self.h = np.zeros((H, W), np.uint8)
        r = self.motion_radius
        limit = self.motion_threshold * (2 * r + 1) ** 2
        out = d.copy()
        inf = np.float32(np.inf)
        for y in range(H):
            for x in range(W):
                dv = d[y, x]
                S, n, h = self.S[y, x], int(self.n[y, x]), int(self.h[y, x])
                static = False
                if prev:
                    M = 0
                    for j in range(-r, r + 1):
                        yy = min(max(y + j, 0), H - 1)
                        for i in range(-r, r + 1):
                            xx = min(max(x + i, 0), W - 1)
                            M += abs(int(G[yy, xx]) - int(self.P[yy, xx]))
                    static = M <= limit
                v = bool(dv > 0) and bool(dv < inf)
                have = static and n > 0
                if v and have and abs(np.float32(dv - S)) <= self.max_diff:
                    t = np.float32(np.float32(dv - S) * self.gains[n])
                    S = np.float32(S + t)
                    n, h = min(n + 1, self.max_age), 0
                    out[y, x] = S
                elif v:
                    S, n, h = dv, 1, 0
                elif have and h < self.hold:
                    h += 1
                    out[y, x] = S
                else:
                    S, n, h = np.float32(0), 0, 0
                self.S[y, x], self.n[y, x], self.h[y, x] = S, n, h
        self.P = G.copy()
        return out
