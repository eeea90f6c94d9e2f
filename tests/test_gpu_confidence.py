"""K2's confidence variant on the device (csrc/dsx_kernels.hip, vol_wta<..., CONF>) against the host
restatement: in every case the map equals depthestimation_amd/confidence.py ``peak_ratio`` of the host volume
bit for bit, and the disparity equals the oracle epilogue plus ``apply_threshold`` (then the texture mask and
the sgbm_post tail where set).

K2's geometry: 16 disparities per lane, TPP = Dp / 16 lanes per pixel, XC = 256 / TPP pixels per chunk,
4 row segments without the LR check (segment length a multiple of XC) and one with it."""
from __future__ import annotations

import numpy as np
import pytest

from depthestimation_amd import _dsx
from depthestimation_amd.census import cost_volume_census
from depthestimation_amd.confidence import apply_threshold, peak_ratio, uniqueness_bound
from depthestimation_amd.postprocess import median_blur3, postprocess_disparity
from depthestimation_amd.prefilter import apply_texture_threshold, prefilter, texture_sum
from depthestimation_amd.synthetic import binary_pair, stereo_pair
from oracle.bt_cost import cost_volume_bt
from oracle.sgbm_post import sgbm_post, wta_sgbm
from oracle.sgm import aggregate
from oracle.stereo_bm import cost_volume, wta_epilogue

pytestmark = pytest.mark.gpu


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _matcher(**kw):
    from depthestimation_amd.matcher import HipBlockMatcher
    return HipBlockMatcher(**kw)


def _largest_ssd_disp(bs):
    """The largest num_disp dsx_check_params accepts for SSD at this block size."""
    for D in (512, 256, 128, 64):
        try:
            _dsx.check_params(_dsx.make_params(num_disp=D, block_size=bs, cost="ssd"))
            return D
        except ValueError:
            continue
    raise AssertionError("no SSD geometry")


def _pair(kind, H, W, m, D, seed):
    if kind == "stereo":
        return stereo_pair(H, W, m, D, seed=seed)[:2]
    if kind == "binary":
        return binary_pair(H, W, m, D, seed=seed)[:2]
    rng = np.random.default_rng(seed)
    if kind == "flat":
        return np.full((H, W), 93, np.uint8), np.full((H, W), 93, np.uint8)
    if kind == "zero":
        return np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    if kind == "sat":  # near-saturated: every block cost sits just below the maximum
        return np.full((H, W), 255, np.uint8), rng.integers(0, 3, (H, W), dtype=np.uint8)
    if kind == "random":
        return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)
    raise AssertionError(kind)


DEF = dict(H=12, W=131, m=0, D=16, bs=5, cost="sad", agg=None, p1=0, p2=0, u=10, lr=-1, lr_form="bm", subpix=True,
           fmode="fixed", t=0, pair="stereo", pf=None, tex=0, post=False)


def _host(c):
    """(L, R, q, fixed, float map or None) of a case on the host."""
    L, R = _pair(c["pair"], c["H"], c["W"], c["m"], c["D"], seed=c["H"] * 7 + c["W"] + c["D"])
    m, D, bs = c["m"], c["D"], c["bs"]
    PL, PR = (prefilter(L, *c["pf"]), prefilter(R, *c["pf"])) if c["pf"] else (L, R)
    if c["cost"] in ("sad", "ssd"):
        C = cost_volume(PL, PR, m, D, bs, c["cost"])
    elif c["cost"] == "bt":
        C = cost_volume_bt(L, R, m, D, bs, 31)
    else:
        C = cost_volume_census(L, R, m, D, bs, c["cost"])
    if c["agg"]:
        C = aggregate(C, c["agg"], c["p1"] or 8 * bs * bs, c["p2"] or 32 * bs * bs)
    q = peak_ratio(C, m, c["lr_form"])
    if c["lr_form"] == "sgbm":
        ref = wta_sgbm(C, m, c["u"], c["lr"], c["subpix"])
    else:
        ref = wta_epilogue(C, m, c["u"], c["lr"], c["subpix"])
    fixed = apply_threshold(ref["fixed"], q, c["t"], m)
    flt = None
    if c["fmode"] == "parabola":
        flt = apply_threshold(ref["parabola"], q, c["t"], m)
    if c["tex"]:
        fixed = apply_texture_threshold(fixed, texture_sum(PL, bs, c["pf"][2]), c["tex"], m)
    if c["post"]:
        fixed = sgbm_post(fixed, m, 50, 2)
    if flt is None:
        flt = fixed.astype(np.float32) / np.float32(16)
    return L, R, C, q, fixed, flt


def _kw(c):
    kw = dict(min_disp=c["m"], num_disp=c["D"], block_size=c["bs"], cost=c["cost"], uniqueness_ratio=c["u"],
              disp12_max_diff=c["lr"], lr_form=c["lr_form"], subpixel=c["subpix"], float_mode=c["fmode"],
              confidence_threshold=c["t"], aggregation=c["agg"], p1=c["p1"], p2=c["p2"], sgbm_post=c["post"],
              speckle_window_size=50, speckle_range=2, texture_threshold=c["tex"])
    if c["pf"]:
        kw.update(prefilter_type=c["pf"][0], prefilter_size=c["pf"][1], prefilter_cap=c["pf"][2])
    return kw


def _run(c, expect_names=None):
    c = dict(DEF, **c)
    L, R, C, q, fixed, flt = _host(c)
    mm = _matcher(timing=True, **_kw(c))
    conf = np.full(L.shape, 77, np.uint8)
    gf = np.empty(L.shape, np.float32)
    got = mm.compute(L, R, out_float=gf, out_confidence=conf)
    names = set(mm.kernel_times())
    mm.close()
    np.testing.assert_array_equal(conf, q)
    np.testing.assert_array_equal(got, fixed)
    if c["fmode"] == "parabola":
        inv = fixed == (c["m"] - 1) * 16
        np.testing.assert_array_equal(gf[inv], np.float32(c["m"] - 1))
        np.testing.assert_allclose(gf, flt, rtol=0, atol=1e-3)
    else:
        np.testing.assert_array_equal(gf, flt)
    assert "volume_wta" in names and "bm_pass_left" not in names
    if expect_names:
        assert expect_names <= names
    return c, C, q, fixed


# ---------------------------------------------------------------- SAD: every D, widths, LR modes ----
@pytest.mark.parametrize("lr,lr_form", [(-1, "bm"), (1, "bm"), (1, "sgbm")], ids=["nolr", "lr_bm", "lr_sgbm"])
@pytest.mark.parametrize("D", [1, 2, 3, 16, 17, 63, 64, 65, 128, 129, 256])
def test_sad_every_disparity_count(D, lr, lr_form):
    _gpu()
    W = {128: 257, 129: 257, 256: 330}.get(D, 131)
    c, C, q, fixed = _run(dict(H=8, W=W, D=D, lr=lr, lr_form=lr_form, u=0, t=1 if D > 3 else 0))
    band = q[:, max(D, 1):]
    if D <= 2:
        assert (q[:, D:] == 255).all()          # no rival can exist
    else:
        assert len(np.unique(band)) > (3 if D == 3 else 20)   # the map is not a constant


def test_sad_512_on_a_narrow_band():
    """D = 512 (TPP 32, XC 8) on 6 x 540: the band [511, 539] is 29 columns wide."""
    _gpu()
    for lr, form in ((-1, "bm"), (1, "bm"), (1, "sgbm")):
        c, C, q, fixed = _run(dict(H=6, W=540, D=512, bs=3, lr=lr, lr_form=form, u=10, t=128))
        assert q[:, :511].max() == 0 and q[:, 512:].any()


@pytest.mark.parametrize("u", [0, 10])
@pytest.mark.parametrize("W", [70, 131, 257, 330])
def test_widths_and_uniqueness(W, u):
    """D = 16 (Dp 128, XC 32): W = 257 gives segments of 96 with a last chunk of one pixel; 70, 131 and 330
    put the segment edges off the chunk size.  u = 0: the rival scan must run without the uniqueness test."""
    _gpu()
    for lr, form in ((-1, "bm"), (1, "bm"), (1, "sgbm")):
        c, C, q, fixed = _run(dict(H=6, W=W, D=16, u=u, lr=lr, lr_form=form, t=128))
        inv = (c["m"] - 1) * 16
        assert (fixed[q < 128] == inv).all() and (fixed != inv).any()
        if u and lr < 0:
            # every in-band pixel uniqueness rejects lies at or below the bound
            keep = wta_epilogue(C, 0, 0, -1, True)["fixed"] != inv
            rej = keep & (wta_epilogue(C, 0, u, -1, True)["fixed"] == inv)
            assert rej.any() and int(q[rej].max()) <= uniqueness_bound(u)


def test_width_below_the_band_gives_an_all_zero_map():
    _gpu()
    for lr, form in ((-1, "bm"), (1, "bm"), (1, "sgbm")):
        c, C, q, fixed = _run(dict(H=6, W=40, m=7, D=64, lr=lr, lr_form=form, t=1))
        assert not q.any() and (fixed == 6 * 16).all()


@pytest.mark.parametrize("m", [-5, 0, 7])
@pytest.mark.parametrize("lr,lr_form", [(-1, "bm"), (0, "bm"), (2, "sgbm")], ids=["nolr", "lr_bm", "lr_sgbm"])
def test_min_disp_and_bands(m, lr, lr_form):
    _gpu()
    c, C, q, fixed = _run(dict(H=9, W=131, m=m, D=33, lr=lr, lr_form=lr_form, t=64))
    x = np.arange(131)
    band = (x >= m + 32) & (x <= 130 + m) if lr_form == "bm" else (x >= max(m + 33, 0)) & (x < 131 + min(m, 0))
    assert not q[:, ~band].any() and q[:, band].any()


# ---------------------------------------------------------------- costs and aggregation ------------
@pytest.mark.parametrize("bs", [11, 15])
def test_ssd_at_the_largest_disparity_count(bs):
    _gpu()
    D = _largest_ssd_disp(bs)
    assert D == {11: 512, 15: 256}[bs]
    _run(dict(H=6, W=D + 28, D=D, bs=bs, cost="ssd", lr=1, u=10, t=32))
    _run(dict(H=6, W=D + 28, D=D, bs=bs, cost="ssd", lr=-1, u=0, t=0, pair="random"))


def test_near_saturated_ssd_15x15():
    """L = 255, R in {0, 1, 2}: every cost is near 225 * 255^2 and 255 * cb passes 2^31."""
    _gpu()
    c, C, q, fixed = _run(dict(H=6, W=131, D=32, bs=15, cost="ssd", u=0, lr=-1, t=1, pair="sat"))
    assert 255 * int(C[:, 31:].min()) > 2 ** 31
    assert q[:, 31:].max() <= 8 and q[:, 31:].any()   # cb < nm gives q >= 1, cb == nm gives 0
    _run(dict(H=6, W=131, D=32, bs=15, cost="ssd", u=10, lr=1, lr_form="sgbm", t=2, pair="sat"))


@pytest.mark.parametrize("cost,bs", [("bt", 5), ("census9x7", 5), ("census5x5", 3), ("census9x7", 1)])
@pytest.mark.parametrize("lr,lr_form", [(-1, "bm"), (1, "bm"), (1, "sgbm")], ids=["nolr", "lr_bm", "lr_sgbm"])
def test_volume_only_costs(cost, bs, lr, lr_form):
    _gpu()
    _run(dict(H=12, W=131, D=48, bs=bs, cost=cost, lr=lr, lr_form=lr_form, t=32),
         {"bt": {"bt_vsum"}, "census9x7": {"census_volume"}, "census5x5": {"census_volume"}}[cost])


@pytest.mark.parametrize("agg,cost,bs,p1,p2,name", [
    ("sgbm_3way", "census9x7", 1, 8, 32, "sgm_paths"),   # NSUM 3
    ("hh", "sad", 5, 0, 0, "sgm_paths"),                 # NSUM 8
    ("hh4", "bt", 3, 0, 0, "sgm_paths"),                 # NSUM 4
    ("sgbm", "sad", 3, 0, 0, "sgm_paths"),               # NSUM 5
    ("sgbm_3way", "sad", 5, 100, 60000, "sgm_path"),     # max cost + P2 >= 0xFFFF: the sequential u32 sums
])
@pytest.mark.parametrize("lr,lr_form", [(-1, "bm"), (1, "bm"), (1, "sgbm")], ids=["nolr", "lr_bm", "lr_sgbm"])
def test_sgm_sums(agg, cost, bs, p1, p2, name, lr, lr_form):
    _gpu()
    _run(dict(H=12, W=131, D=48, bs=bs, cost=cost, agg=agg, p1=p1, p2=p2, lr=lr, lr_form=lr_form, t=32), {name})


# ---------------------------------------------------------------- epilogue options ------------------
@pytest.mark.parametrize("t", [0, 1, 128, 255])
@pytest.mark.parametrize("subpix", [True, False])
def test_thresholds_and_subpixel(t, subpix):
    _gpu()
    c, C, q, fixed = _run(dict(H=12, W=200, D=64, bs=5, u=10, lr=1, subpix=subpix, t=t))
    kept = float((fixed[:, 63:] != -16).mean())
    print(f"t={t}: kept {kept:.3f}")
    assert (kept > 0.3) if t < 255 else True


@pytest.mark.parametrize("lr", [-1, 1])
def test_float_mode_parabola(lr):
    _gpu()
    _run(dict(H=12, W=200, D=64, bs=5, u=10, lr=lr, fmode="parabola", t=64))
    _run(dict(H=12, W=131, m=-5, D=48, bs=1, cost="census9x7", agg="sgbm_3way", p1=8, p2=32, u=5, lr=lr,
              fmode="parabola", t=32))


@pytest.mark.parametrize("pair", ["flat", "zero"])
def test_flat_images_have_zero_confidence(pair):
    _gpu()
    for cost, bs in (("sad", 5), ("ssd", 15), ("census9x7", 3)):
        c, C, q, fixed = _run(dict(H=6, W=131, D=32, bs=bs, cost=cost, u=0, lr=-1, t=1, pair=pair))
        assert not q.any() and (fixed == -16).all()
        c, C, q, fixed = _run(dict(H=6, W=131, D=32, bs=bs, cost=cost, u=0, lr=1, t=0, pair=pair))
        assert not q.any()


def test_binary_pair():
    _gpu()
    _run(dict(H=12, W=200, D=64, bs=5, u=10, lr=1, t=16, pair="binary"))
    _run(dict(H=12, W=200, D=64, bs=3, cost="sad", agg="hh", u=10, lr=1, lr_form="sgbm", t=16, pair="binary"))


def test_texture_mask_and_sgbm_post_leave_the_map_alone():
    """The map with a prefilter + texture threshold equals the map of the filtered pair without the threshold,
    sgbm_post does not change it either, and the order is threshold -> texture mask -> sgbm_post."""
    _gpu()
    pf = ("xsobel", 9, 31)
    base = dict(H=24, W=160, D=32, bs=5, u=10, lr=1, t=48, pf=pf)
    _, _, q0, f0 = _run(dict(base))
    _, _, q1, f1 = _run(dict(base, tex=590))
    _, _, q2, f2 = _run(dict(base, tex=590, post=True))
    _run(dict(H=24, W=160, D=32, bs=5, u=10, lr=1, t=48, post=True))
    np.testing.assert_array_equal(q0, q1)
    np.testing.assert_array_equal(q0, q2)
    assert (f1 != f2).any()   # the tail ran, on the masked map (the host composition above has that order)
    _run(dict(base, tex=590, post=True, lr_form="sgbm", cost="ssd"))


# ---------------------------------------------------------------- routing ---------------------------
@pytest.mark.parametrize("D,lr", [(64, 1), (48, -1), (128, 1)])
def test_fused_handle_routes_confidence_calls_to_the_volume_path(D, lr):
    """One fused SAD handle: without, with, without a confidence output.  D <= 64 is the fused pass's
    one-disparity-per-lane layout, whose volume-path geometry differs (Dp 64 -> 128)."""
    torch = _gpu()
    H, W = 24, 200
    L, R, _ = stereo_pair(H, W, 0, D, seed=D)
    C = cost_volume(L, R, 0, D, 5, "sad")
    want = wta_epilogue(C, 0, 10, lr, True)["fixed"]
    Ld, Rd = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    mm = _matcher(num_disp=D, block_size=5, disp12_max_diff=lr, timing=True)
    outs = [torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(3)]
    conf = torch.full((H, W), 77, dtype=torch.uint8, device="cuda")
    mm.compute_device(Ld, Rd, out_fixed=outs[0])
    torch.cuda.synchronize()
    n0 = set(mm.kernel_times())
    ws0 = mm.workspace_bytes()
    mm.reset_times()
    mm.compute_device(Ld, Rd, out_fixed=outs[1], out_confidence=conf)
    torch.cuda.synchronize()
    n1 = {k for k, v in mm.kernel_times().items() if v[1]}
    ws1 = mm.workspace_bytes()
    mm.reset_times()
    mm.compute_device(Ld, Rd, out_fixed=outs[2])
    torch.cuda.synchronize()
    n2 = {k for k, v in mm.kernel_times().items() if v[1]}
    ws2 = mm.workspace_bytes()
    # map only: no disparity output at all
    conf2 = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    mm.compute_device(Ld, Rd, out_confidence=conf2)
    torch.cuda.synchronize()
    ws3 = mm.workspace_bytes()
    mm.close()
    for o in outs:
        np.testing.assert_array_equal(o.cpu().numpy(), want)
    np.testing.assert_array_equal(conf.cpu().numpy(), peak_ratio(C, 0))
    np.testing.assert_array_equal(conf2.cpu().numpy(), peak_ratio(C, 0))
    assert "bm_pass_left" in n0 and "volume_wta" not in n0
    assert n1 == {"cost_volume", "volume_wta"}
    assert "bm_pass_left" in n2 and "volume_wta" not in n2 and "cost_volume" not in n2
    Dp = 128 if D <= 128 else 256
    assert ws1 == ws0 + H * W * Dp * 2          # the volume, once
    assert ws2 == ws1 and ws3 == ws1


def test_threshold_on_a_fused_handle_and_set_params():
    """confidence_threshold > 0 makes every call of the handle a volume-path call; back at 0 it is fused
    again.  Host calls through dsx_compute_conf_host stage the map."""
    _gpu()
    H, W, D = 16, 150, 48
    L, R, _ = stereo_pair(H, W, 0, D, seed=3)
    C = cost_volume(L, R, 0, D, 5, "sad")
    ref = wta_epilogue(C, 0, 10, 1, True)["fixed"]
    q = peak_ratio(C, 0)
    mm = _matcher(num_disp=D, block_size=5, timing=True)
    np.testing.assert_array_equal(mm.compute(L, R), ref)
    mm.set_params(confidence_threshold=100)
    mm.reset_times()
    np.testing.assert_array_equal(mm.compute(L, R), apply_threshold(ref, q, 100, 0))
    assert {k for k, v in mm.kernel_times().items() if v[1]} == {"cost_volume", "volume_wta"}
    conf = np.zeros((H, W), np.uint8)
    np.testing.assert_array_equal(mm.compute(L, R, out_confidence=conf), apply_threshold(ref, q, 100, 0))
    np.testing.assert_array_equal(conf, q)
    mm.set_params(confidence_threshold=0)
    mm.reset_times()
    np.testing.assert_array_equal(mm.compute(L, R), ref)
    assert {k for k, v in mm.kernel_times().items() if v[1]} == {"bm_pass_left", "lr_fixup"}
    with pytest.raises(ValueError):
        mm.set_params(confidence_threshold=256)
    mm.close()


def test_batch_and_process_pair_honour_the_threshold():
    torch = _gpu()
    H, W, D, t = 40, 200, 64, 64
    pairs = [stereo_pair(H, W, 0, D, seed=s)[:2] for s in (1, 2, 3)]
    refs = []
    for L, R in pairs:
        C = cost_volume(L, R, 0, D, 5, "sad")
        refs.append(apply_threshold(wta_epilogue(C, 0, 10, 1, True)["fixed"], peak_ratio(C, 0), t, 0))
    assert all(0.05 < float((r[:, D:] == -16).mean()) < 0.9 for r in refs)
    mm = _matcher(num_disp=D, block_size=5, confidence_threshold=t)
    Ld = torch.stack([torch.from_numpy(p[0]) for p in pairs]).cuda()
    Rd = torch.stack([torch.from_numpy(p[1]) for p in pairs]).cuda()
    out = torch.empty((3, H, W), dtype=torch.int16, device="cuda")
    mm.compute_batch_device(Ld, Rd, out_fixed=out)
    torch.cuda.synchronize()
    for i in range(3):
        np.testing.assert_array_equal(out[i].cpu().numpy(), refs[i], err_msg=f"frame {i}")
    for i, fast in ((0, True), (1, False)):
        dd, dz = mm.process_pair_device(Ld[i], Rd[i], fast_mode=fast, max_speckle_size=100, max_diff=1.0,
                                        outlier_threshold=2.5, focal_length=700.0, baseline=0.1)
        torch.cuda.synchronize()
        disp = (refs[i].astype(np.float32) / np.float32(16))[:, D:]
        if fast:
            want = median_blur3(disp)
        else:
            want = postprocess_disparity(disp, max_speckle_size=100, max_diff=1.0, outlier_threshold=2.5,
                                         apply_outlier_removal=True, apply_hole_filling=False)
        np.testing.assert_array_equal(dd.cpu().numpy(), want, err_msg=f"fast={fast}")
        assert dz is not None
    mm.close()


@pytest.mark.parametrize("fast", [True, False])
def test_stereo_core_confidence_map(fast):
    torch = _gpu()
    from depthestimation_amd.StereoDepthEstimator import StereoDepthEstimator
    from depthestimation_amd.stereo_core import StereoCore
    H, W, D = 40, 200, 64
    L, R, _ = stereo_pair(H, W, 0, D, seed=8)
    C = cost_volume(L, R, 0, D, 5, "sad")
    q = peak_ratio(C, 0)[:, D:]
    core = StereoCore(fast_mode=fast)
    core.configure_sgbm(num_disp=D, block_size=5, confidence=True, confidence_threshold=48, focal_length=700.0,
                        baseline=0.1, hole_filling=not fast, fill_method="nearest")
    hd, hz = core._process_pair(L, R)
    hq = core.confidence_map
    assert isinstance(hq, np.ndarray) and hq.dtype == np.uint8 and hq.shape == (H, W - D)
    np.testing.assert_array_equal(hq, q)
    dd, dz = core.process_pair_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    torch.cuda.synchronize()
    dq = core.confidence_map
    assert isinstance(dq, torch.Tensor) and dq.dtype == torch.uint8 and tuple(dq.shape) == (H, W - D)
    np.testing.assert_array_equal(dq.cpu().numpy(), q)
    np.testing.assert_array_equal(dd.cpu().numpy(), hd)
    np.testing.assert_array_equal(dz.cpu().numpy(), hz)
    # the threshold alone stays on the one-call route and gives the same disparity; no map is kept
    core.configure_sgbm(confidence=False)
    d1, z1 = core.process_pair_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    torch.cuda.synchronize()
    assert core.confidence_map is None
    np.testing.assert_array_equal(d1.cpu().numpy(), hd)
    # the facade: host arrays in, the map as a host array
    est = StereoDepthEstimator()
    est.left_source, est.right_source = L, R
    est.core.fast_mode = fast
    est.configure_sgbm(num_disp=D, block_size=5, confidence=True, confidence_threshold=48,
                       hole_filling=not fast, fill_method="nearest")
    ed, _ = est.estimate_depth()
    np.testing.assert_array_equal(ed, hd)
    assert isinstance(est.confidence_map, np.ndarray)
    np.testing.assert_array_equal(est.confidence_map, q)
    est.core.sgbm.close()
    core.sgbm.close()
