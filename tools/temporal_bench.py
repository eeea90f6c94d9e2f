"""Temporal-filter timings at the cropped maps of C2 (1080 x 1792) and C4 (720 x 1152):

* `temporal_step`: the filter's one launch per frame (dsx_tfilter_run_device, depth included, 16-byte path);
* `torch_rule`: the same rule written with torch tensor operations on the same tensors - the only other way to
  this result on the device (its output is compared with the launch's, bit for bit, before anything is timed);
* the model's bytes (27 B per pixel: read d 4, S 4, G 1, P 1, n + h 2; write out 4, S 4, P 1, n + h 2, depth 4)
  over the launch's time;
* the drop-in frame (`StereoCore.estimate_depth_device`, the reference's defaults) with the filter on and off.

Stream events around `--calls` back-to-back calls, the variants alternating round by round in one process, after
warm-up rounds; median and range over the rounds.  One JSON line per shape.

usage: python tools/temporal_bench.py [--configs c2 c4] [--rounds 15] [--calls 20] [--out profiles/temporal_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from depthestimation_amd.configs import CONFIGS  # noqa: E402
from depthestimation_amd.matcher import TemporalFilterDevice  # noqa: E402
from depthestimation_amd.stereo_core import StereoCore  # noqa: E402
from depthestimation_amd.synthetic import stereo_pair  # noqa: E402
from depthestimation_amd.temporal import TEMPORAL_DEFAULTS, temporal_gains  # noqa: E402

FOCAL, BASE, DOFFS, EPS, ZMAX = 1050.0, 0.12, 0.0, 0.0, 80.0
MODEL_BYTES_PER_PIXEL = 27


def sequence(H, W, n=4, seed=1234):
    """A static scene seen ``n`` times: a k / 16 map with +-1/4 px of noise and 5 % holes per frame, a guide with
    +-2 grey levels of noise and 3 % of its pixels replaced (motion)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(32, 2048, (H, W)).astype(np.float32) / 16.0
    g0 = rng.integers(0, 256, (H, W)).astype(np.int32)
    out = []
    for _ in range(n):
        d = base + rng.integers(-4, 5, (H, W)).astype(np.float32) / 16.0
        d[rng.random((H, W)) < 0.05] = -1.0
        g = np.where(rng.random((H, W)) < 0.03, rng.integers(0, 256, (H, W)), g0 + rng.integers(-2, 3, (H, W)))
        out.append((d.astype(np.float32), np.clip(g, 0, 255).astype(np.uint8)))
    return out


class TorchRule:
    """The rule of include/dsx.h in torch tensor operations (eager: every operation its own kernel, so no
    multiply-add is fused and the results carry the kernel's bits)."""

    def __init__(self, dev, max_age, max_diff, motion_radius, motion_threshold, hold):
        self.r, self.k = motion_radius, 2 * motion_radius + 1
        self.limit = float(motion_threshold * self.k * self.k)
        self.max_age, self.hold = max_age, hold
        self.max_diff = float(np.float32(max_diff))
        self.gains = torch.from_numpy(temporal_gains(max_age)).to(dev)
        self.fB = torch.tensor(float(np.float32(FOCAL * BASE)), dtype=torch.float32, device=dev)  # a tensor: a true division
        self.S = None

    def __call__(self, d, G):
        inf = float("inf")
        v = (d > 0) & (d < inf)
        if self.S is None:
            self.S = torch.zeros_like(d)
            self.n = torch.zeros_like(G)
            self.h = torch.zeros_like(G)
            static = torch.zeros_like(v)
        else:
            ad = (G.to(torch.int16) - self.P.to(torch.int16)).abs().to(torch.float32)[None, None]
            if self.r:
                ad = F.avg_pool2d(F.pad(ad, (self.r,) * 4, mode="replicate"), self.k, stride=1, divisor_override=1)
            static = ad[0, 0] <= self.limit
        S, n, h = self.S, self.n, self.h
        have = static & (n > 0)
        diff = d - S
        agree = v & have & (diff.abs() <= self.max_diff)
        avg = S + diff * self.gains[n.long()]
        fresh = v & ~agree
        held = ~v & have & (h < self.hold)
        out = torch.where(agree, avg, torch.where(held, S, d))
        zero = torch.zeros((), dtype=d.dtype, device=d.device)
        self.S = torch.where(agree, avg, torch.where(fresh, d, torch.where(held, S, zero)))
        one = torch.ones((), dtype=n.dtype, device=d.device)
        self.n = torch.where(agree, torch.clamp(n + 1, max=self.max_age), torch.where(fresh, one, torch.where(held, n, 0 * one)))
        self.h = torch.where(held, h + 1, 0 * one)
        self.P = G.clone()
        adj = out + DOFFS
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c2", "c4"])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("temporal_bench needs a HIP device")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    lines = []
    for cname in args.configs:
        cfg = CONFIGS[cname]
        H, D = cfg["H"], cfg["num_disp"]
        W = cfg["W"] - D
        with torch.cuda.stream(stream):
            seq = [(torch.from_numpy(d).to(dev), torch.from_numpy(g).to(dev)) for d, g in sequence(H, W)]
            out, depth = torch.empty((H, W), device=dev), torch.empty((H, W), device=dev)
            filt = TemporalFilterDevice(device=0, **TEMPORAL_DEFAULTS)
            rule = TorchRule(dev, **TEMPORAL_DEFAULTS)

            def launch(i):
                filt.run(*seq[i % len(seq)], out=out, out_depth=depth, focal_length=FOCAL, baseline=BASE, doffs=DOFFS,
                         eps=EPS, max_depth=ZMAX, stream=stream)

            def torch_rule(i):
                return rule(*seq[i % len(seq)])

            # the same result from both, at the timed size, on every frame of two passes over the sequence
            depth_equal = True
            for i in range(2 * len(seq)):
                launch(i)
                to, tz = torch_rule(i)
                stream.synchronize()
                assert torch.equal(out.view(torch.int32), to.view(torch.int32)), (cname, i)
                depth_equal = depth_equal and torch.equal(depth.view(torch.int32), tz.view(torch.int32))
            # the drop-in frame with the filter off and on
            pairs = []
            for s in range(4):
                L, R, _ = stereo_pair(H, cfg["W"], 0, D, seed=1234 + s)
                pairs.append((torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)))
            cores = {}
            for k in ("off", "on"):
                cores[k] = StereoCore()
                cores[k].configure_sgbm(num_disp=D, block_size=cfg["block_size"], focal_length=700.0, baseline=0.1,
                                        temporal="recursive" if k == "on" else "none")
            variants = {"temporal_step": launch, "torch_rule": torch_rule}
            for k, core in cores.items():
                variants["dropin_" + k] = lambda i, core=core: core.estimate_depth_device(*pairs[i % 4], stream=stream)
            times = {k: [] for k in variants}
            for r in range(args.warmup + args.rounds):
                for k, fn in variants.items():
                    t = time_calls(fn, args.calls, stream)
                    if r >= args.warmup:
                        times[k].append(t)
            state_bytes = filt.state_bytes()
            filt.close()
        model = MODEL_BYTES_PER_PIXEL * H * W
        step = float(np.median(times["temporal_step"]))
        line = {"config": cname, "H": H, "W": W, "params": dict(TEMPORAL_DEFAULTS), "calls_per_sample": args.calls,
                "rounds": args.rounds, "model_bytes": model, "state_bytes": state_bytes,
                "depth_equals_torch": depth_equal,
                "temporal_step_us": stats(times["temporal_step"]), "torch_rule_us": stats(times["torch_rule"]),
                "temporal_step_model_GBps": round(model / (1e-3 * step) / 1e9, 1),
                # the acceptance figure: the torch form over the launch (> 1: the launch is faster)
                "torch_over_step": round(float(np.median(times["torch_rule"])) / step, 2),
                "dropin_off_ms": stats(times["dropin_off"], 1.0, 4), "dropin_on_ms": stats(times["dropin_on"], 1.0, 4),
                "dropin_on_minus_off_us": round(1e3 * (float(np.median(times["dropin_on"])) -
                                                       float(np.median(times["dropin_off"]))), 2)}
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
