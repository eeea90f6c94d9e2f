"""Row step of the fused block-matching pass (csrc/dsx_bm.hip) after the work around its SADs:
lane-indexed tile stores (ds_write_addtid_b32 with a per-wave M0 base, drained by hand before the
barrier of multi-wave blocks), the key-tree argmin of the packed-pair epilogue, prefetch loads in the
scalar-base form with offsets carried across the steps, the staging address carried across the steps
and the scalar priority band.

Every comparison is bit for bit over all pixels: the int16 x16 map and the float map - float mode
'fixed' against x16 / 16 (exact in f32), float mode 'parabola' against the oracle's parabola map by
bit pattern.  The plain left pass, the left pass with the uniqueness / left-right checks (lr_form
'bm') and the volume path take the C oracle (oracle/cref.py); OpenCV's LR form and the right map take
the numpy oracle on the same block costs (oracle/sgbm_post.wta_sgbm, oracle/stereo_bm.right_argmin).

Shapes: W = 256 or 250 (a partial last strip), H <= 40, grid_blocks 0, 1, 7.  At D = 128, R = 4 the
strips x0 = 160 and 192 stage their rows with the unaligned-dword loads and the others with clamped
bytes, so both copies of the loop run.
  * ties: a constant pair and pairs whose columns repeat with period 8 and 64 give equal costs at
    d, d + 8k and d + 64k - between the 8-disparity blocks of an epilogue lane and between the two
    lanes of a pixel; the lowest disparity must win.  With and without uniqueness_ratio = 10,
    sub-pixel on, both float modes, sides 0, 3 and 4;
  * lane-indexed stores under masks: D = 100 (padding disparities), 127 (odd range), 131 and 192 (two
    and four waves per block), SSD blocks 5 and 13 (which keep the address form), the right map and
    the volume path (same store loop);
  * staging: block sizes 5, 9, 15, min_disp 0, 5, -3, padded rows, two frames per launch,
    H = 1, 2, 9, 10;
  * three in-flight handles on three streams."""
from __future__ import annotations

import numpy as np
import pytest

from depthestimation_amd.synthetic import stereo_pair
from oracle.cref import CRef
from oracle.sgbm_post import wta_sgbm
from oracle.stereo_bm import cost_volume, right_argmin

import fused_geometry as fg

pytestmark = pytest.mark.gpu

GRIDS = (0, 1, 7)
PLAIN = dict(uniqueness_ratio=0, disp12_max_diff=-1)
UNIQ = dict(uniqueness_ratio=10, disp12_max_diff=-1)
LRBM = dict(uniqueness_ratio=10, disp12_max_diff=1, lr_form="bm")
LRBM0 = dict(uniqueness_ratio=0, disp12_max_diff=1, lr_form="bm")


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def cref():
    return CRef()


def _random(m, D, H, W, seed=0):
    L, R, _ = stereo_pair(H, W, m, D, seed=2000 + 7 * D + m + seed)
    return L, R


def _periodic(P, H, W, seed):
    """Left == right, columns repeating with period P (rows differ): C(x, d) == C(x, d + P)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, P), dtype=np.uint8)
    img = np.tile(base, (1, (W + P - 1) // P))[:, :W].copy()
    return img, img.copy()


def _tie_inputs(m, D, H, W):
    const = np.full((H, W), 93, np.uint8)
    return {"random": _random(m, D, H, W), "constant": (const, const.copy()),
            "period8": _periodic(8, H, W, 8), "period64": _periodic(64, H, W, 64)}


def _left(torch, pairs, wants, what, grids=GRIDS, fmode="fixed", **kw):
    """One matcher per grid, every input through it, both outputs checked."""
    from depthestimation_amd.matcher import HipBlockMatcher
    for g in grids:
        mt = HipBlockMatcher(grid_blocks=g, float_mode=fmode, **kw)
        try:
            for name, (L, R) in pairs.items():
                fx = torch.empty(L.shape, dtype=torch.int16, device="cuda")
                fl = torch.empty(L.shape, dtype=torch.float32, device="cuda")
                mt.compute_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), out_fixed=fx, out_float=fl)
                torch.cuda.synchronize()
                fg.check_maps(fx, fl, wants[name], f"{what} grid_blocks={g} input={name}", fmode)
        finally:
            mt.close()


def _cref_all(cref, pairs, m, D, bs, cost, u, lr):
    return {n: cref(L, R, m, D, bs, cost, u, lr, True) for n, (L, R) in pairs.items()}


def _right(torch, pairs, vols, m, what, **base):
    from depthestimation_amd.matcher import HipBlockMatcher
    for g in GRIDS:
        mt = HipBlockMatcher(grid_blocks=g, **base)
        try:
            for name, (L, R) in pairs.items():
                out = torch.empty(L.shape, dtype=torch.int16, device="cuda")
                mt.right_map_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), out)
                torch.cuda.synchronize()
                fg.check(out.cpu().numpy().astype(np.int32), right_argmin(vols[name], m),
                       f"{what} right map grid_blocks={g} input={name}")
        finally:
            mt.close()


# ---- ties --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tie_case(cref):
    """Inputs and oracles of the tie cases, computed once (H = 24: two segments per strip at 7 blocks)."""
    m, D, bs, H = 0, 128, 9, 24
    out = {}
    for W in (256, 250):
        pairs = _tie_inputs(m, D, H, W)
        refs = {(u, lr): _cref_all(cref, pairs, m, D, bs, "sad", u, lr) for u in (0, 10) for lr in (-1, 1)}
        vols = {n: cost_volume(L, R, m, D, bs, "sad") for n, (L, R) in pairs.items()}
        sg = {u: {n: wta_sgbm(vols[n], m, u, 1, True)["fixed"] for n in pairs} for u in (0, 10)}
        out[W] = (pairs, refs, sg)
    return out


@pytest.mark.parametrize("W", [256, 250])
@pytest.mark.parametrize("fmode", ["fixed", "parabola"])
@pytest.mark.parametrize("u", [0, 10])
def test_ties_left_and_lr_bm(torch_dev, tie_case, W, fmode, u):
    """Sides 0 and 3: equal costs 8 and 64 disparities apart, the lowest disparity wins."""
    pairs, refs, _ = tie_case[W]
    base = dict(min_disp=0, num_disp=128, block_size=9, cost="sad")
    _left(torch_dev, pairs, refs[(u, -1)], f"W={W} u={u} left", fmode=fmode, uniqueness_ratio=u, disp12_max_diff=-1, **base)
    _left(torch_dev, pairs, refs[(u, 1)], f"W={W} u={u} lr bm", fmode=fmode, uniqueness_ratio=u, disp12_max_diff=1,
          lr_form="bm", **base)


@pytest.mark.parametrize("W", [256, 250])
@pytest.mark.parametrize("u", [0, 10])
def test_ties_lr_sgbm(torch_dev, tie_case, W, u):
    """Side 4 (OpenCV's LR form on the fused path)."""
    pairs, _, sg = tie_case[W]
    _left(torch_dev, pairs, sg[u], f"W={W} u={u} lr sgbm", uniqueness_ratio=u, disp12_max_diff=1, lr_form="sgbm",
          path="fused", min_disp=0, num_disp=128, block_size=9, cost="sad")


@pytest.mark.parametrize("D", [131, 192])
def test_ties_multiwave(torch_dev, cref, D):
    """Two and four waves per block: ties across the epilogue lanes of different waves' slices."""
    m, bs, H, W = 0, 9, 12, 256
    pairs = _tie_inputs(m, D, H, W)
    base = dict(min_disp=m, num_disp=D, block_size=bs, cost="sad")
    for fmode in ("fixed", "parabola"):
        _left(torch_dev, pairs, _cref_all(cref, pairs, m, D, bs, "sad", 10, -1), f"D={D} left", fmode=fmode, **UNIQ, **base)
    _left(torch_dev, pairs, _cref_all(cref, pairs, m, D, bs, "sad", 0, 1), f"D={D} lr bm", **LRBM0, **base)


# ---- lane-indexed stores under masks -------------------------------------------------------------

@pytest.mark.parametrize("cost,bs,D", [("sad", 9, 100), ("sad", 9, 127), ("sad", 9, 131), ("sad", 9, 192),
                                       ("ssd", 5, 128), ("ssd", 13, 128)])
@pytest.mark.parametrize("W", [256, 250])
def test_masked_stores(torch_dev, cref, cost, bs, D, W):
    m, H = 0, 40
    pairs = {"random": _random(m, D, H, W), "period8": _periodic(8, H, W, 3)}
    base = dict(min_disp=m, num_disp=D, block_size=bs, cost=cost)
    _left(torch_dev, pairs, _cref_all(cref, pairs, m, D, bs, cost, 0, -1), "left", **PLAIN, **base)
    lr = _cref_all(cref, pairs, m, D, bs, cost, 10, 1)
    _left(torch_dev, pairs, lr, "lr bm", **LRBM, **base)
    if cost == "sad":  # the right map and the volume path share the left pass's store loop
        _left(torch_dev, pairs, lr, "volume", path="volume", uniqueness_ratio=10, disp12_max_diff=1, **base)
        vols = {n: cost_volume(L, R, m, D, bs, cost) for n, (L, R) in pairs.items()}
        _right(torch_dev, pairs, vols, m, f"D={D}", **base)
        _left(torch_dev, pairs, {n: wta_sgbm(vols[n], m, 10, 1, True)["fixed"] for n in pairs}, "lr sgbm",
              uniqueness_ratio=10, disp12_max_diff=1, lr_form="sgbm", path="fused", **base)


# ---- staging -------------------------------------------------------------------------------------

@pytest.mark.parametrize("bs,m", [(5, 0), (5, -3), (9, 0), (9, 5), (9, -3), (15, 0), (15, 5)])
def test_staging_blocks_and_min_disp(torch_dev, cref, bs, m):
    D, H, W = 128, 40, 250
    pairs = {"random": _random(m, D, H, W)}
    base = dict(min_disp=m, num_disp=D, block_size=bs, cost="sad")
    _left(torch_dev, pairs, _cref_all(cref, pairs, m, D, bs, "sad", 0, -1), "left", **PLAIN, **base)
    lr = _cref_all(cref, pairs, m, D, bs, "sad", 10, 1)
    _left(torch_dev, pairs, lr, "lr bm", **LRBM, **base)
    vols = {n: cost_volume(L, R, m, D, bs, "sad") for n, (L, R) in pairs.items()}
    _left(torch_dev, pairs, {n: wta_sgbm(vols[n], m, 10, 1, True)["fixed"] for n in pairs}, "lr sgbm",
          uniqueness_ratio=10, disp12_max_diff=1, lr_form="sgbm", path="fused", **base)
    _right(torch_dev, pairs, vols, m, f"bs={bs} m={m}", **base)


@pytest.mark.parametrize("H", [1, 2, 9, 10])
def test_staging_short_frames(torch_dev, cref, H):
    """Frames shorter than the window and segments of a single row (grid = strips x H)."""
    m, D, bs, W = 0, 128, 9, 256
    pairs = {"random": _random(m, D, H, W), "period64": _periodic(64, H, W, 5)}
    grids = GRIDS + ((W // 32) * H,)
    base = dict(min_disp=m, num_disp=D, block_size=bs, cost="sad")
    _left(torch_dev, pairs, _cref_all(cref, pairs, m, D, bs, "sad", 0, -1), f"H={H} left", grids, **PLAIN, **base)
    _left(torch_dev, pairs, _cref_all(cref, pairs, m, D, bs, "sad", 10, 1), f"H={H} lr bm", grids, **LRBM, **base)


@pytest.mark.parametrize("pad", [0, 24])
def test_two_frames_and_padded_rows(torch_dev, cref, pad):
    """Two different frames per launch (H = 19: with 7 blocks a block's rows cross the frame boundary),
    contiguous and with rows padded to W + 24; a single padded frame as well."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    m, D, bs, H, W = 0, 128, 9, 19, 256
    fr = [_random(m, D, H, W, seed=s) for s in (0, 1)]
    bufL = torch.zeros((2, H, W + pad), dtype=torch.uint8, device="cuda")
    bufR = torch.zeros((2, H, W + pad), dtype=torch.uint8, device="cuda")
    dL, dR = bufL[:, :, :W], bufR[:, :, :W]
    for i, (L, R) in enumerate(fr):
        dL[i].copy_(torch.from_numpy(L))
        dR[i].copy_(torch.from_numpy(R))
    base = dict(min_disp=m, num_disp=D, block_size=bs, cost="sad")
    for what, kw, u, lr in (("left", PLAIN, 0, -1), ("lr bm", LRBM, 10, 1)):
        wants = [cref(L, R, m, D, bs, "sad", u, lr, True) for L, R in fr]
        for g in GRIDS:
            mt = HipBlockMatcher(grid_blocks=g, **kw, **base)
            try:
                fx = torch.empty((2, H, W), dtype=torch.int16, device="cuda")
                fl = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
                mt.compute_batch_device(dL, dR, out_fixed=fx, out_float=fl)
                torch.cuda.synchronize()
                for i in range(2):
                    fg.check_maps(fx[i], fl[i], wants[i], f"batch {what} pad={pad} grid_blocks={g} frame={i}")
                fx1 = torch.empty((H, W), dtype=torch.int16, device="cuda")
                fl1 = torch.empty((H, W), dtype=torch.float32, device="cuda")
                mt.compute_device(dL[1], dR[1], out_fixed=fx1, out_float=fl1)
                torch.cuda.synchronize()
                fg.check_maps(fx1, fl1, wants[1], f"single {what} pad={pad} grid_blocks={g}")
            finally:
                mt.close()


# ---- handles -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw,u,lr", [(PLAIN, 0, -1), (LRBM, 10, 1)], ids=["left", "lr_bm"])
def test_three_in_flight(torch_dev, cref, kw, u, lr):
    """Three in_flight handles on three streams, two rounds, each with its own frame and oracle."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    m, D, bs, H, W = 0, 128, 9, 40, 256
    fr = [_random(m, D, H, W, seed=s) for s in (0, 1)] + [_periodic(8, H, W, 11)]
    wants = [cref(L, R, m, D, bs, "sad", u, lr, True) for L, R in fr]
    dev = [(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in fr]
    handles = [HipBlockMatcher(in_flight=True, min_disp=m, num_disp=D, block_size=bs, cost="sad", **kw) for _ in range(3)]
    streams = [torch.cuda.Stream() for _ in range(3)]
    fx = [torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(6)]
    fl = [torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    try:
        for i in range(6):
            handles[i % 3].compute_device(*dev[i % 3], out_fixed=fx[i], out_float=fl[i], stream=streams[i % 3])
        torch.cuda.synchronize()
        for i in range(6):
            fg.check_maps(fx[i], fl[i], wants[i % 3], f"in_flight handle {i % 3} call {i // 3}")
    finally:
        for h in handles:
            h.close()
