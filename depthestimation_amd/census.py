"""Host restatement of the census costs (include/dsx.h ``DSX_COST_CENSUS9X7`` / ``DSX_COST_CENSUS5X5``;
the device kernels in csrc/dsx_census.hip equal it bit for bit).

Census is an addition of this build, as the prefilter is: parity with nothing outside this repository is
claimed.  The cost's name carries the window wx x wy ('census9x7': 62 bits, 'census5x5': 24 bits).  With
cx / cy the replicate clamp into the image, rx = wx // 2, ry = wy // 2:

  code : T(I)(x, y): the neighbours (i, j) with j from -ry to ry (outer loop) and i from -rx to rx (inner
         loop), the centre skipped, counted k = 0, 1, ...; bit k is 1 iff I(cx(x+i), cy(y+j)) < I(x, y)
         (strict).  The unused upper bits are 0.
  cost : C(x, y, d) = sum over |i|, |j| <= block_size // 2 of
         popcount(T_L[cy(y+j), cx(x+i)] xor T_R[cy(y+j), cx(x+i-m-d)])
         - the A5' window of oracle/stereo_bm.py over the codes: the coordinates of the codes are clamped,
         not the codes' inputs.  block_size 1 is the per-pixel Hamming cost used with SGM.

The volume feeds ``oracle.stereo_bm.wta_epilogue``, ``oracle.sgm.aggregate`` and ``oracle.sgbm_post`` like
any other int64 cost volume.
"""
from __future__ import annotations

import numpy as np

__all__ = ["WINDOWS", "census_bits", "max_cost_census", "census_transform", "popcount64", "cost_volume_census"]

WINDOWS = {"census9x7": (9, 7), "census5x5": (5, 5)}  # cost name -> (wx, wy)

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def _window(cost):
    if cost not in WINDOWS:
        raise ValueError(f"cost must be one of {list(WINDOWS)}, got {cost!r}")
    return WINDOWS[cost]


def census_bits(cost: str) -> int:
    """Bits of a code: 62 or 24."""
    wx, wy = _window(cost)
    return wx * wy - 1


def max_cost_census(block_size: int, cost: str) -> int:
    return block_size * block_size * census_bits(cost)


def census_transform(img, cost: str = "census9x7") -> np.ndarray:
    """T(I) as uint64 H x W."""
    wx, wy = _window(cost)
    I = np.asarray(img)
    if I.dtype != np.uint8 or I.ndim != 2 or I.size == 0:
        raise ValueError("image must be a non-empty uint8 H x W array")
    H, W = I.shape
    rx, ry = wx // 2, wy // 2
    p = I[np.clip(np.arange(-ry, H + ry), 0, H - 1)][:, np.clip(np.arange(-rx, W + rx), 0, W - 1)]
    T = np.zeros((H, W), np.uint64)
    k = 0
    for j in range(wy):
        for i in range(wx):
            if j == ry and i == rx:
                continue
            T |= (p[j:j + H, i:i + W] < I).astype(np.uint64) << np.uint64(k)
            k += 1
    return T


def popcount64(a) -> np.ndarray:
    """Set bits of every uint64 element (a byte table: any numpy), int64."""
    a = np.ascontiguousarray(a, np.uint64)
    return _POP8[a.view(np.uint8).reshape(a.shape + (8,))].sum(axis=-1, dtype=np.int64)


def cost_volume_census(L, R, min_disp: int, num_disp: int, block_size: int, cost: str = "census9x7") -> np.ndarray:
    """C[y, x, d] as int64 (the summed-area form of oracle/stereo_bm.py cost_volume over the codes)."""
    L = np.asarray(L)
    R = np.asarray(R)
    if L.shape != R.shape:
        raise ValueError("L and R must have the same shape")
    if block_size < 1 or block_size % 2 == 0:
        raise ValueError("block_size must be odd and >= 1")
    if num_disp < 1:
        raise ValueError("num_disp must be >= 1")
    TL, TR = census_transform(L, cost), census_transform(R, cost)
    H, W = TL.shape
    r, k = block_size // 2, block_size
    ys = np.clip(np.arange(-r, H + r), 0, H - 1)
    xs = np.arange(-r, W + r)
    Lp = TL[ys][:, np.clip(xs, 0, W - 1)]
    Rrows = TR[ys]
    C = np.empty((H, W, num_disp), np.int64)
    for d in range(num_disp):
        e = popcount64(Lp ^ Rrows[:, np.clip(xs - min_disp - d, 0, W - 1)])
        S = np.zeros((e.shape[0] + 1, e.shape[1] + 1), np.int64)
        S[1:, 1:] = e.cumsum(0).cumsum(1)
        C[:, :, d] = S[k:, k:] - S[:-k, k:] - S[k:, :-k] + S[:-k, :-k]
    return C
