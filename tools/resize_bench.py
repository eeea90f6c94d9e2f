"""Device area downscale (csrc/dsx_resize.hip): kernel times and the video facade's frame rate with the
downscale on the host against on the device.  Writes the report to --out (profiles/resize_area_ab.txt).

(a) kernel: resident frames, stream events around batches of launches, min / median / max of the batches
    per launch, for 1920x1080x3 -> 0.5 and 0.667 and 1280x720x3 -> 0.5 (and 0.25: the looping form), plain
    and gray-fused.  Comparator: the gray_only kernel on the same full-size frame (reads the same bytes).
(b) facade: StereoDepthEstimatorVideo(downscale_factor=0.5, fast_mode=True, target_fps=0) over --frames
    synthetic 1080p BGR frames from ndarray sources, device_downscale False against True, alternating,
    --pairs runs each, wall clock around the whole generator.

usage: python tools/resize_bench.py [--out FILE] [--skip-facade] [--frames 200] [--pairs 3]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from depthestimation_amd import StereoDepthEstimatorVideo  # noqa: E402
from depthestimation_amd.input import resize_area, resize_area_device  # noqa: E402
from depthestimation_amd.matcher import rectify_device  # noqa: E402
from depthestimation_amd.rectify import to_grayscale_bgr  # noqa: E402
from depthestimation_amd.synthetic import stereo_pair  # noqa: E402


def timed_us(fn, stream, batches=30, per_batch=20):
    """(min, median, max) microseconds per launch over `batches` event-timed batches of `per_batch`."""
    for _ in range(2 * per_batch):
        fn()
    stream.synchronize()
    ts = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(per_batch):
            fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / per_batch)
    return min(ts), float(np.median(ts)), max(ts)


def kernel_part(say):
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    rng = np.random.default_rng(1)
    say("(a) kernel time per launch, microseconds: min / median / max of 30 batches of 20 launches")
    for (H, W), factor in (((1080, 1920), 0.5), ((1080, 1920), 0.667), ((720, 1280), 0.5), ((1080, 1920), 0.25)):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        d = torch.from_numpy(img).to(dev)
        ref = resize_area(img, factor)
        Ho, Wo = ref.shape[:2]
        out3 = torch.empty((Ho, Wo, 3), dtype=torch.uint8, device=dev)
        out1 = torch.empty((Ho, Wo), dtype=torch.uint8, device=dev)
        full = torch.empty((H, W), dtype=torch.uint8, device=dev)
        mb = (H * W * 3 + Ho * Wo * 3) / 1e6
        say(f"{W}x{H}x3 -> {factor} ({Wo}x{Ho}), {mb:.2f} MB moved by the 3-channel form")
        with torch.cuda.stream(stream):
            t = timed_us(lambda: rectify_device(d, out=full, stream=stream), stream)
            say(f"  gray_only (full size, comparator)  {t[0]:8.2f} {t[1]:8.2f} {t[2]:8.2f}")
            for gray, out in ((False, out3), (True, out1)):
                t = timed_us(lambda: resize_area_device(d, factor, gray=gray, out=out, stream=stream), stream)
                stream.synchronize()
                want = to_grayscale_bgr(ref) if gray else ref
                bad = int(np.count_nonzero(out.cpu().numpy() != want))
                say(f"  resize_area {'gray-fused' if gray else '3-channel '}              "
                    f"{t[0]:8.2f} {t[1]:8.2f} {t[2]:8.2f}   bytes differing from the host: {bad}")


def facade_part(say, frames, pairs):
    H, W, base_n = 1080, 1920, 8
    base = []
    for i in range(base_n):
        Lg, Rg, _ = stereo_pair(H, W, 0, 64, seed=100 + i)
        base.append((np.stack([Lg, np.roll(Lg, 1, 0), Lg // 2], 2).astype(np.uint8),
                     np.stack([Rg, np.roll(Rg, 1, 0), Rg // 2], 2).astype(np.uint8)))
    idx = np.arange(frames) % base_n
    lefts = np.stack([base[i][0] for i in idx])
    rights = np.stack([base[i][1] for i in idx])

    def run(dd):
        v = StereoDepthEstimatorVideo(lefts, rights, downscale_factor=0.5, fast_mode=True, target_fps=0,
                                      device_downscale=dd)
        v.configure_sgbm(num_disp=256, block_size=5, focal_length=2800.0, baseline=0.1)  # 64 at 960x540
        t0 = time.perf_counter()
        n, last = 0, None
        for z in v.estimate_depth():
            n, last = n + 1, z
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert n == frames
        return frames / dt, last

    say(f"(b) video facade, {frames} synthetic {W}x{H} BGR frames, downscale_factor 0.5, fast_mode, "
        "target_fps 0: frames/s")
    run(False)  # warm-up of both forms (code objects, tables, pinned buffers)
    run(True)
    for k in range(pairs):
        fh, zh = run(False)
        fd, zd = run(True)
        same = bool(np.array_equal(zh, zd))
        say(f"  pairing {k + 1}: host downscale {fh:8.1f}   device downscale {fd:8.1f}   ratio {fd / fh:6.2f}   "
            f"last depth maps equal: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "resize_area_ab.txt"))
    ap.add_argument("--skip-facade", action="store_true")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("resize_bench needs a HIP device")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say(f"tools/resize_bench.py on {torch.cuda.get_device_name(0)}")
        kernel_part(say)
        if not args.skip_facade:
            facade_part(say, args.frames, args.pairs)


if __name__ == "__main__":
    main()
