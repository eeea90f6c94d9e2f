"""Point-cloud output timings at the cropped maps of C2 (1080 x 1792) and C4 (720 x 1152), about 85 % valid:
the three compaction launches with the lane-per-point stores (libdsx.so) and with the LDS-staged stores
(libdsx_cloud_staged.so, `make -C depthestimation_amd/csrc cloud_staged`, when it is there), `cloud_reproject`,
and the baseline - torch's own boolean-mask gather of the same organized map and colours (`xyz[mask]` plus
`rgb[mask]`, mask precomputed) on the same tensors.  Stream events around `--calls` back-to-back calls, the
variants alternating round by round in one process, after warm-up rounds; median and range over the rounds.
The outputs of every variant are compared before anything is timed.  A staged library older than its sources
is skipped with a message (`--allow-stale-staged` times it anyway); `staged_lib` in the line says which.
One JSON line per shape.

usage: python tools/cloud_bench.py [--configs c2 c4] [--rounds 15] [--calls 20] [--out profiles/cloud_bench.jsonl]
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
from depthestimation_amd.configs import CONFIGS  # noqa: E402
from depthestimation_amd.matcher import reproject_device  # noqa: E402

STAGED_LIB = os.path.join(ROOT, "depthestimation_amd", "libdsx_cloud_staged.so")
STAGED_SOURCES = [os.path.join(ROOT, "depthestimation_amd", "csrc", n) for n in ("dsx_cloud.hip", "dsx_internal.h")] + \
    [os.path.join(ROOT, "include", "dsx.h")]
F, B, DOFFS, EPS, ZMAX =1050.0, 0.12, 0.0, 0.0, 80.0


def scene(H, W, x0, seed=1234):
    """A k / 16 map in [2, 128) px with 15 % invalid pixels (-1 in runs along rows, as occlusions and failed
    matches come) and an uncropped BGR image."""
    rng = np.random.default_rng(seed)
    d = rng.integers(32, 2048, (H, W)).astype(np.float32) / 16.0
    runs = rng.random((H, W // 8 + 1)) < 0.15
    d[np.repeat(runs, 8, axis=1)[:, :W]] = -1.0
    bgr = rng.integers(0, 256, (H, x0 + W, 3), dtype=np.uint8)
    return d, bgr


def time_calls(fn, calls, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(calls):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c2", "c4"])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_bench.jsonl"))
    ap.add_argument("--allow-stale-staged", action="store_true",
                    help="time libdsx_cloud_staged.so even when it is older than its sources")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("cloud_bench needs a HIP device")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    libs = {"direct": _dsx.lib()}  # the library's own form first
    staged_note = "absent (make cloud_staged)"
    if os.path.exists(STAGED_LIB):
        # `make cloud_staged` is a step of its own: a variant left from an older tree must not be timed unnoticed
        newer = [s for s in STAGED_SOURCES if os.path.getmtime(s) > os.path.getmtime(STAGED_LIB)]
        if newer and not args.allow_stale_staged:
            staged_note = "skipped: older than " + ", ".join(os.path.relpath(s, ROOT) for s in newer)
            print(f"cloud_bench: {STAGED_LIB} {staged_note}; rebuild it with `make cloud_staged` "
                  "(or pass --allow-stale-staged)", file=sys.stderr)
        else:
            libs["staged"] = _dsx._bind(ctypes.CDLL(STAGED_LIB))
            staged_note = "timed" + (" (older than its sources)" if newer else "")
    lines = []
    for cname in args.configs:
        cfg = CONFIGS[cname]
        H, x0 = cfg["H"], cfg["num_disp"]
        W = cfg["W"] - x0
        d, bgr = scene(H, W, x0)
        c = _dsx.make_cloud(F, B, (x0 + W - 1) / 2, (H - 1) / 2, DOFFS, EPS, ZMAX, x0)
        with torch.cuda.stream(stream):
            disp, color = torch.from_numpy(d).to(dev), torch.from_numpy(bgr).to(dev)
            xyz = reproject_device(disp, F, B, None, DOFFS, EPS, ZMAX, x0, stream=stream)
            mask = ~torch.isnan(xyz[..., 2])
            rgb = color[:, x0:].flip(2).contiguous()           # the organized RGB of the map's pixels
            N = int(mask.sum().item())
            nbytes = int(libs["direct"].dsx_point_cloud_workspace_bytes(H, W))
            outs = {k: (torch.empty((H * W, 3), dtype=torch.float32, device=dev),
                        torch.empty((H * W, 3), dtype=torch.uint8, device=dev),
                        torch.empty((H * W,), dtype=torch.int32, device=dev),
                        torch.zeros(1, dtype=torch.int32, device=dev),
                        torch.empty(nbytes, dtype=torch.uint8, device=dev)) for k in libs}

            def cloud(k):
                P, C, I, n, ws = outs[k]
                rc = libs[k].dsx_point_cloud_device(disp.data_ptr(), H, W, W, ctypes.byref(c), color.data_ptr(),
                                                    color.stride(0), 3, P.data_ptr(), C.data_ptr(), I.data_ptr(), H * W,
                                                    n.data_ptr(), ws.data_ptr(), nbytes, stream.cuda_stream)
                if rc:
                    raise RuntimeError(libs[k].dsx_last_error().decode())

            def torch_gather():
                return xyz[mask], rgb[mask]

            variants = {k: (lambda k=k: cloud(k)) for k in libs}
            variants["reproject"] = lambda: reproject_device(disp, F, B, None, DOFFS, EPS, ZMAX, x0, out=xyz, stream=stream)
            variants["torch_mask_gather"] = torch_gather
            # the same result from every variant, at the timed size
            tp, tc = torch_gather()
            for k in libs:
                cloud(k)
                stream.synchronize()
                P, C, I, n, _ = outs[k]
                assert int(n.item()) == N == len(tp), (k, int(n.item()), N)
                assert torch.equal(P[:N].view(torch.int32), tp.view(torch.int32)) and torch.equal(C[:N], tc), k
                assert torch.equal(I[:N].long(), mask.flatten().nonzero().flatten()), k
            times = {k: [] for k in variants}
            for r in range(args.warmup + args.rounds):
                for k, fn in variants.items():
                    t = time_calls(fn, args.calls, stream)
                    if r >= args.warmup:
                        times[k].append(t)
        # the map is read twice (count, scatter), the colour of a point once; 12 + 3 + 4 B per point
        model = 2 * 4 * H * W + 3 * N + (12 + 3 + 4) * N
        line = {"config": cname, "H": H, "W": W, "x0": x0, "points": N, "valid": round(N / (H * W), 4),
                "calls_per_sample": args.calls, "rounds": args.rounds, "model_bytes": model,
                "staged_lib": staged_note}
        for k, ts in times.items():
            line[k + "_us"] = {"median": round(1e3 * float(np.median(ts)), 2), "min": round(1e3 * min(ts), 2),
                               "max": round(1e3 * max(ts), 2)}
        for k in libs:
            line[k + "_model_GBps"] = round(model / (1e-3 * float(np.median(times[k]))) / 1e9, 1)
        line["reproject_GBps"] = round(16 * H * W / (1e-3 * float(np.median(times["reproject"]))) / 1e9, 1)
        # the acceptance figure: torch's gather over the library's three launches (> 1: the library is faster)
        line["torch_over_cloud"] = round(float(np.median(times["torch_mask_gather"])) / float(np.median(times["direct"])), 2)
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
