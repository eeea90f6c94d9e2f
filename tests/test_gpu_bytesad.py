"""Byte-SAD column update of the packed-pair block-matching pass (csrc/dsx_bm.hip: v_sad_u8 /
v_sad_hi_u8 on zero-extended bytes, one staged dword per search entry and per reference column).

Every comparison is bit for bit over all pixels.  The plain left pass, the left pass with the
uniqueness and left-right checks (lr_form 'bm') and the volume path are compared with the C oracle
(oracle/cref.py); the C oracle has neither OpenCV's LR form nor a right map, so those two take the
numpy oracle on the same block costs (oracle/sgbm_post.wta_sgbm, oracle/stereo_bm.right_argmin), as
tests/test_sgbm_lr.py and tests/test_gpu_parity.py do.

Shapes: H = 40, W = 256.  At D = 128, R = 4 the strips x0 = 160 and 192 stage their rows with the
unaligned-dword loads and the others with clamped bytes, so both staging forms run; the block sizes
cover the transposed init (3, 5, 15) and the row-by-row init (9); D = 131 is an odd range on two
waves with padding disparities, D = 192 three waves' worth on four; grid_blocks 0 / 1 / 7 move the
segment starts to different rows.  Inputs: one seeded random pair and two carry stressors whose
neighbouring disparities hold 0 and the maximum cost in the two halves of one register."""
from __future__ import annotations

import numpy as np
import pytest

from depthestimation_amd.synthetic import stereo_pair
from oracle.cref import CRef
from oracle.sgbm_post import wta_sgbm
from oracle.stereo_bm import cost_volume, right_argmin

import fused_geometry as fg

pytestmark = pytest.mark.gpu

H, W = 40, 256
GRIDS = (0, 1, 7)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def cref():
    return CRef()


def _inputs(m, D):
    """name -> (L, R): the random pair and the two carry stressors."""
    L, R, _ = stereo_pair(H, W, m, D, seed=1000 + 7 * D + m)
    white = np.full((H, W), 255, np.uint8)
    x = np.arange(W)[None, :]
    y = np.arange(H)[:, None]
    cols = np.broadcast_to(((x & 1) * 255).astype(np.uint8), (H, W)).copy()  # columns 0, 255, 0, ...
    rows = (((x + y) & 1) * 255).astype(np.uint8)                            # rows alternate as well
    return {"random": (L, R), "carry_cols": (white, cols), "carry_rows": (white, rows)}


def _left(torch, pairs, wants, what, **kw):
    """One matcher per grid, every input through it."""
    from depthestimation_amd.matcher import HipBlockMatcher
    for g in GRIDS:
        mt = HipBlockMatcher(grid_blocks=g, **kw)
        try:
            for name, (L, R) in pairs.items():
                fg.check(mt.compute(L, R), wants[name], f"{what} grid_blocks={g} input={name}")
        finally:
            mt.close()


@pytest.mark.parametrize("m", [0, 5, -3])
@pytest.mark.parametrize("D", [128, 131, 192])
@pytest.mark.parametrize("bs", [3, 5, 9, 15])
def test_pair_layout_sides(torch_dev, cref, bs, D, m):
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    pairs = _inputs(m, D)
    base = dict(min_disp=m, num_disp=D, block_size=bs, cost="sad")
    vols = {n: cost_volume(L, R, m, D, bs, "sad") for n, (L, R) in pairs.items()}
    # plain left pass
    _left(torch, pairs, {n: cref(L, R, m, D, bs, "sad", 0, -1, True)["fixed"] for n, (L, R) in pairs.items()},
          "left", uniqueness_ratio=0, disp12_max_diff=-1, **base)
    # left pass + uniqueness + left-right check built along the tile's diagonals (side 3)
    _left(torch, pairs, {n: cref(L, R, m, D, bs, "sad", 10, 1, True)["fixed"] for n, (L, R) in pairs.items()},
          "lr bm", uniqueness_ratio=10, disp12_max_diff=1, lr_form="bm", **base)
    # left pass + OpenCV's LR keys (side 4)
    _left(torch, pairs, {n: wta_sgbm(vols[n], m, 10, 1, True)["fixed"] for n in pairs},
          "lr sgbm", uniqueness_ratio=10, disp12_max_diff=1, lr_form="sgbm", path="fused", **base)
    # right map (side 1)
    for g in GRIDS:
        mt = HipBlockMatcher(grid_blocks=g, **base)
        try:
            for name, (L, R) in pairs.items():
                out = torch.empty((H, W), dtype=torch.int16, device="cuda")
                mt.right_map_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), out)
                torch.cuda.synchronize()
                fg.check(out.cpu().numpy().astype(np.int32), right_argmin(vols[name], m),
                       f"right map grid_blocks={g} input={name}")
        finally:
            mt.close()


@pytest.mark.parametrize("m", [0, 5, -3])
@pytest.mark.parametrize("bs", [3, 5, 9, 15])
def test_pair_layout_volume_d48(torch_dev, cref, bs, m):
    """path='volume' at D = 48: the pair layout at D <= 64 (the fused path gives those to SAD1)."""
    D = 48
    pairs = _inputs(m, D)
    _left(torch_dev, pairs, {n: cref(L, R, m, D, bs, "sad", 10, 1, True)["fixed"] for n, (L, R) in pairs.items()},
          "volume", path="volume", min_disp=m, num_disp=D, block_size=bs, cost="sad", uniqueness_ratio=10,
          disp12_max_diff=1)


@pytest.mark.parametrize("cost,bs,D", [("sad", 5, 64), ("ssd", 13, 128)], ids=["sad1", "ssd_u32"])
def test_reference_row_layout_single_disparity_builds(torch_dev, cref, cost, bs, D):
    """SAD1 (one disparity per lane, D <= 64) and the u32 SSD build (R = 6) read the reference row
    as one dword per column."""
    pairs = _inputs(0, D)
    for u, lr in ((0, -1), (10, 1)):
        _left(torch_dev, pairs, {n: cref(L, R, 0, D, bs, cost, u, lr, True)["fixed"] for n, (L, R) in pairs.items()},
              f"{cost} u={u} lr={lr}", min_disp=0, num_disp=D, block_size=bs, cost=cost, uniqueness_ratio=u,
              disp12_max_diff=lr)
