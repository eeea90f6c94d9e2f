"""Joint-bilateral-upsampling timings at 1080 x 1920 <- 540 x 960 and 720 x 1280 <- 360 x 640 (x0 64, BGR guide):

* `upsample_joint`: the stage's one launch (dsx_upsample_device, depth included) at radius 1 and 2, called
  through `matcher.joint_upsample_device` as a user calls it, and `upsample_joint_raw`: the same C call with its
  arguments prepared once, which leaves the Python wrapper's checks out of the back-to-back calls;
* `torch_rule`: the same rule written with torch tensor operations on the same tensors - gathers of the
  (2r + 1)^2 taps, a sort for the selection, the gated sums in window order - the only other way to this result on
  the device (its output is compared with the launch's, bit for bit, before anything is timed);
* the model's bytes (per output pixel 8 written and `ch` read, plus 5 per low-resolution pixel) over the launch's
  time;
* the frame: `StereoCore.estimate_depth_device` of a 1080p BGR pair at input_scale 0.5 (the reference's defaults
  scaled: num_disp 64) with the stage on and off, and beside it the full-size frame at num_disp 128.

Stream events around `--calls` back-to-back calls, the variants alternating round by round in one process, after
warm-up rounds; median and range over the rounds.  One JSON line per shape and radius, one for the frame.

usage: python tools/upsample_bench.py [--rounds 15] [--calls 20] [--out profiles/upsample_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from depthestimation_amd import _dsx  # noqa: E402
from depthestimation_amd.matcher import joint_upsample_device  # noqa: E402
from depthestimation_amd.postprocess import wmedian_weights  # noqa: E402
from depthestimation_amd.stereo_core import StereoCore  # noqa: E402
from depthestimation_amd.synthetic import stereo_pair  # noqa: E402
from depthestimation_amd.upsample import upsample_taps, upsample_x0  # noqa: E402

FOCAL, BASE, DOFFS, EPS, ZMAX = 525.0, 0.12, 0.0, 0.0, 80.0
SIGMA, MAX_DIFF = 8, 1.0
SHAPES = {"1080p": (1080, 1920, 540, 960, 64), "720p": (720, 1280, 360, 640, 64)}


def scene(H, W, h, Wl, x0, seed=1234):
    """A low-resolution k / 16 map with smooth regions, steps and 5 % holes, its guide, and a BGR full-size guide
    correlated with it."""
    rng = np.random.default_rng(seed)
    w = Wl - x0
    d = (rng.integers(64, 96, (h, w)) + 160 * (rng.random((h, w)) < 0.3)).astype(np.float32) / 16
    d[rng.random((h, w)) < 0.05] = -1.0
    g = rng.integers(0, 256, (h, Wl), dtype=np.uint8)
    G = g[(np.arange(H) * h // H)[:, None], (np.arange(W) * Wl // W)[None, :]].astype(np.int32)
    G = np.clip(G[..., None] + rng.integers(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8)
    return d, g, G


class TorchRule:
    """The rule of include/dsx.h in torch tensor operations (eager: every operation its own kernel, so no
    multiply-add is fused and the results carry the kernel's bits).  The integer geometry is built once on the
    host, outside the timed calls."""

    def __init__(self, dev, H, W, h, Wl, x0, r):
        self.r, self.n, self.x0, self.h, self.w = r, 2 * r + 1, x0, h, Wl - x0
        X0 = upsample_x0(W, Wl, x0)
        ny, ay = upsample_taps(H, h, r)
        nx, ax = upsample_taps(W, Wl, r)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.ny, self.nx = t(ny), t(nx[X0:])
        self.ay, self.ax = t(ay.astype(np.int32)), t(ax[X0:].astype(np.int32))
        self.T = t(wmedian_weights(SIGMA).astype(np.int32))
        self.X0 = X0
        self.sx = float(np.float32(W / Wl))
        self.md = float(np.float32(MAX_DIFF))
        self.fB = torch.tensor(float(np.float32(FOCAL * BASE)), dtype=torch.float32, device=dev)  # a tensor: a true division

    def __call__(self, d, g, G):
        inf = float("inf")
        r, n = self.r, self.n
        c = G[:, self.X0:].to(torch.int32)
        gp = (c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14
        gl = g.to(torch.int32)
        dv, wv = [], []
        for j in range(n):
            y = self.ny + (j - r)
            yin = (y >= 0) & (y < self.h)
            yc = y.clamp(0, self.h - 1)
            for i in range(n):
                x = self.nx + (i - r) - self.x0
                xin = (x >= 0) & (x < self.w)
                xc = x.clamp(0, self.w - 1)
                v = d[yc[:, None], xc[None, :]]
                ok = yin[:, None] & xin[None, :] & (v > 0) & (v < inf)
                wq = self.ax[None, :, i] * self.ay[:, j, None] * self.T[(gp - gl[yc[:, None], (xc + self.x0)[None, :]]).abs()]
                dv.append(torch.where(ok, v, torch.full_like(v, inf)))
                wv.append(torch.where(ok, wq, torch.zeros_like(wq)))
        dv, wv = torch.stack(dv), torch.stack(wv)
        S = wv.sum(0)
        ds, order = torch.sort(dv, dim=0, stable=True)
        cs = torch.gather(wv, 0, order).cumsum(0)
        m = torch.where(2 * cs >= S[None], ds, torch.full_like(ds, inf)).amin(0)
        num = torch.zeros_like(m)
        den = torch.zeros_like(S)
        for p in range(n * n):
            inside = (dv[p] - m).abs() <= self.md
            prod = wv[p].to(torch.float32) * torch.where(inside, dv[p], torch.zeros_like(m))
            num = torch.where(inside, num + prod, num)
            den = den + torch.where(inside, wv[p], torch.zeros_like(S))
        a = num / den.clamp(min=1).to(torch.float32)
        have = S > 0
        centre = d[self.ny[:, None], (self.nx - self.x0)[None, :]]
        out = torch.where(have, a * self.sx, centre)
        val = torch.where(have, a, centre)
        adj = val + DOFFS
        z = torch.where(adj > EPS, self.fB / adj, torch.full_like(adj, inf)).clamp(max=ZMAX)
        return out, z


def time_calls(fn, calls, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for i in range(calls):
        fn(i)
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / calls


def stats(ts, scale=1e3, digits=2):
    return {"median": round(scale * float(np.median(ts)), digits), "min": round(scale * min(ts), digits),
            "max": round(scale * max(ts), digits)}


def run_rounds(variants, args, stream):
    times = {k: [] for k in variants}
    for r in range(args.warmup + args.rounds):
        for k, fn in variants.items():
            t = time_calls(fn, args.calls, stream)
            if r >= args.warmup:
                times[k].append(t)
    return times


def bench_launch(name, radius, args, dev, stream):
    H, W, h, Wl, x0 = SHAPES[name]
    with torch.cuda.stream(stream):
        scenes = [tuple(torch.from_numpy(a).to(dev) for a in scene(H, W, h, Wl, x0, 1234 + s)) for s in range(2)]
        Wo = W - upsample_x0(W, Wl, x0)
        out, depth = torch.empty((H, Wo), device=dev), torch.empty((H, Wo), device=dev)
        rule = TorchRule(dev, H, W, h, Wl, x0, radius)

        def launch(i):
            d, g, G = scenes[i % len(scenes)]
            joint_upsample_device(d, x0, g, G, radius, SIGMA, MAX_DIFF, focal_length=FOCAL, baseline=BASE, doffs=DOFFS,
                                  eps=EPS, max_depth=ZMAX, out=out, out_depth=depth, stream=stream)

        up = _dsx.make_upsample("joint", radius, SIGMA, MAX_DIFF)
        call = _dsx.lib().dsx_upsample_device
        raw_args = [(d.data_ptr(), h, Wl - x0, d.stride(0), x0, g.data_ptr(), Wl, g.stride(0), G.data_ptr(), H, W, 3,
                     G.stride(0), ctypes.byref(up), out.data_ptr(), depth.data_ptr(), FOCAL, BASE, DOFFS, EPS, ZMAX, 1,
                     stream.cuda_stream) for d, g, G in scenes]

        def launch_raw(i):
            if call(*raw_args[i % len(scenes)]) != 0:
                raise RuntimeError(_dsx.last_error())

        def torch_rule(i):
            return rule(*scenes[i % len(scenes)])

        for i in range(len(scenes)):  # the same result from both, at the timed size
            launch(i)
            to, tz = torch_rule(i)
            stream.synchronize()
            assert torch.equal(out.view(torch.int32), to.view(torch.int32)), (name, radius, i, "disparity")
            assert torch.equal(depth.view(torch.int32), tz.view(torch.int32)), (name, radius, i, "depth")
        launch_raw(0)
        stream.synchronize()
        assert torch.equal(out.view(torch.int32), torch_rule(0)[0].view(torch.int32)), (name, radius, "raw call")
        times = run_rounds({"upsample_joint": launch, "upsample_joint_raw": launch_raw, "torch_rule": torch_rule},
                           args, stream)
    model = H * Wo * (8 + 3) + 5 * h * (Wl - x0)
    step = float(np.median(times["upsample_joint"]))
    raw = float(np.median(times["upsample_joint_raw"]))
    return {"case": name, "H": H, "W": W, "h": h, "Wl": Wl, "x0": x0, "out_W": Wo, "channels": 3, "radius": radius,
            "sigma": SIGMA, "max_diff": MAX_DIFF, "calls_per_sample": args.calls, "rounds": args.rounds,
            "equals_torch_bit_for_bit": True, "model_bytes": model,
            "upsample_joint_us": stats(times["upsample_joint"]),
            "upsample_joint_raw_us": stats(times["upsample_joint_raw"]), "torch_rule_us": stats(times["torch_rule"]),
            "upsample_joint_model_TBps": round(model / (1e-3 * step) / 1e12, 3),
            "upsample_joint_raw_model_TBps": round(model / (1e-3 * raw) / 1e12, 3),
            # the acceptance figure: the torch form over the launch (> 1: the launch is faster)
            "torch_over_launch": round(float(np.median(times["torch_rule"])) / step, 2)}


def bench_frame(args, dev, stream):
    H, W, D = 1080, 1920, 128
    with torch.cuda.stream(stream):
        pairs = []
        for s in range(4):
            L, R, _ = stereo_pair(H, W, 0, D, seed=1234 + s)
            bgr = lambda a: np.ascontiguousarray(np.stack([a, a, a], axis=-1))  # noqa: E731
            pairs.append((torch.from_numpy(bgr(L)).to(dev), torch.from_numpy(bgr(R)).to(dev)))
        cores = {}
        for k in ("half_off", "half_on", "full"):
            cores[k] = StereoCore(downscale_factor=1.0 if k == "full" else 0.5)
            cores[k].configure_sgbm(num_disp=D, focal_length=1050.0, baseline=0.12, max_depth=ZMAX,
                                    upsample="joint" if k == "half_on" else "none")
        variants = {}
        for k, core in cores.items():
            kw = {} if k == "full" else {"input_scale": 0.5}
            variants[k] = lambda i, core=core, kw=kw: core.estimate_depth_device(*pairs[i % 4], stream=stream, **kw)
        shapes = {k: list(fn(0)[1].shape) for k, fn in variants.items()}
        stream.synchronize()
        times = run_rounds(variants, args, stream)
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"case": "frame_1080p_bgr", "num_disp_full": D, "num_disp_half": cores["half_on"].sgbm_params["num_disp"],
            "depth_shapes": shapes, "calls_per_sample": args.calls, "rounds": args.rounds,
            "half_off_ms": stats(times["half_off"], 1.0, 4), "half_on_ms": stats(times["half_on"], 1.0, 4),
            "full_ms": stats(times["full"], 1.0, 4),
            "half_on_minus_off_us": round(1e3 * (med["half_on"] - med["half_off"]), 2),
            "full_over_half_on": round(med["full"] / med["half_on"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=list(SHAPES))
    ap.add_argument("--radii", nargs="+", type=int, default=[1, 2])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("upsample_bench needs a HIP device")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    lines = []
    for name in args.cases:
        for radius in args.radii:
            lines.append(bench_launch(name, radius, args, dev, stream))
            print(json.dumps(lines[-1]), flush=True)
    if not args.no_frame:
        lines.append(bench_frame(args, dev, stream))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
