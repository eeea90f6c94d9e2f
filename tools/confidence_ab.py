"""A/B timings of the matcher's confidence map (K2's confidence variant, csrc/dsx_kernels.hip): the same
configuration with and without a confidence output, alternating in one process, round after round - the
`volume_wta` kernel (HIP-event kernel timings of a timing handle) and the whole call (stream events around
`--calls` calls of a plain handle).  Dev tool; one JSON line per (round, variant), then a summary per variant
(mean, standard deviation and range over the rounds).

    python tools/confidence_ab.py [--rounds 8] [--calls 10]
    python tools/confidence_ab.py --other-root DIR    # K2 without confidence: this tree against another built
                                                      # tree (DIR/depthestimation_amd), alternating child processes
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

# --root DIR (the children of --other-root): import the package of that tree instead of this one
_ROOT = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv[:-1] else \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(_ROOT))

# (matcher keywords beyond the config's own, hand a confidence output)
VARIANTS = {
    "c2_volume": (dict(path="volume"), False),
    "c2_volume_conf": (dict(path="volume"), True),
    "c2_fused": (dict(), False),
    "c2_fused_conf": (dict(), True),
    "c2_census_sgm3": (dict(cost="census9x7", aggregation="sgbm_3way", block_size=1, p1=8, p2=32,
                            uniqueness_ratio=10, disp12_max_diff=1), False),
    "c2_census_sgm3_conf": (dict(cost="census9x7", aggregation="sgbm_3way", block_size=1, p1=8, p2=32,
                                 uniqueness_ratio=10, disp12_max_diff=1), True),
}


class Variant:
    def __init__(self, name, Ld, Rd):
        import torch
        from depthestimation_amd.configs import CONFIGS, matcher_kwargs
        from depthestimation_amd.matcher import HipBlockMatcher
        over, conf = VARIANTS[name]
        kw = matcher_kwargs(CONFIGS["c2"], **over)
        self.name, self.Ld, self.Rd = name, Ld, Rd
        self.plain, self.timed = HipBlockMatcher(**kw), HipBlockMatcher(timing=True, **kw)
        self.out = torch.empty(Ld.shape, dtype=torch.int16, device=Ld.device)
        self.conf = torch.empty(Ld.shape, dtype=torch.uint8, device=Ld.device) if conf else None
        self.stream = torch.cuda.Stream(Ld.device)
        for m in (self.plain, self.timed):  # warm-up: code objects, buffers
            self.call(m, 5)
        self.stream.synchronize()

    def call(self, m, n):
        kw = {} if self.conf is None else dict(out_confidence=self.conf)
        for _ in range(n):
            m.compute_device(self.Ld, self.Rd, out_fixed=self.out, stream=self.stream, **kw)

    def round(self, calls):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(self.stream)
        self.call(self.plain, calls)
        e1.record(self.stream)
        e1.synchronize()
        self.timed.reset_times()
        self.call(self.timed, calls)
        self.stream.synchronize()
        kt = {k: round(v[0], 4) for k, v in self.timed.kernel_times().items() if v[1]}
        return dict(variant=self.name, call_ms=round(e0.elapsed_time(e1) / calls, 4), kernels_ms=kt)

    def close(self):
        self.plain.close()
        self.timed.close()


def summary(rows, key):
    out = {}
    for name in dict.fromkeys(r["variant"] for r in rows):
        v = [key(r) for r in rows if r["variant"] == name and key(r) is not None]
        if v:
            out[name] = dict(mean=round(statistics.mean(v), 4), sd=round(statistics.pstdev(v), 4),
                             min=round(min(v), 4), max=round(max(v), 4), n=len(v))
    return out


def run(names, rounds, calls):
    import torch
    from depthestimation_amd.configs import CONFIGS
    from depthestimation_amd.synthetic import stereo_pair
    cfg = CONFIGS["c2"]
    L, R, _ = stereo_pair(cfg["H"], cfg["W"], 0, cfg["num_disp"], seed=1)
    dev = torch.device("cuda:0")
    Ld, Rd = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    vs = [Variant(n, Ld, Rd) for n in names]
    rows = []
    for r in range(rounds):
        for v in (vs if r % 2 == 0 else vs[::-1]):  # alternate, and alternate the order
            row = dict(v.round(calls), round=r)
            rows.append(row)
            print(json.dumps(row), flush=True)
    for v in vs:
        v.close()
    print(json.dumps({"summary": "volume_wta_ms", **summary(rows, lambda r: r["kernels_ms"].get("volume_wta"))}))
    print(json.dumps({"summary": "call_ms", **summary(rows, lambda r: r["call_ms"])}), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", nargs="+", default=list(VARIANTS))
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--other-root", default=None, help="another built tree: K2 without confidence, tree against tree")
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not args.other_root:
        run(args.variants, args.rounds, args.calls)
        return
    # one fresh child per (round, build), alternating: each child runs the c2 volume path on its library
    rows = []
    for r in range(args.rounds):
        for tag, root in ((("this", _ROOT), ("other", args.other_root)) if r % 2 == 0 else
                          (("other", args.other_root), ("this", _ROOT))):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--variants", "c2_volume", "--rounds", "3",
                                "--calls", str(args.calls), "--root", root], capture_output=True, text=True,
                               timeout=300)
            if p.returncode != 0:
                sys.stderr.write(p.stderr)
                raise SystemExit(f"child ({tag}) failed with {p.returncode}")
            for line in p.stdout.splitlines():
                row = json.loads(line) if line.startswith("{") else {}
                if "variant" in row:
                    row = dict(row, variant=tag, round=r)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    print(json.dumps({"summary": "volume_wta_ms", **summary(rows, lambda r: r["kernels_ms"].get("volume_wta"))}))
    print(json.dumps({"summary": "call_ms", **summary(rows, lambda r: r["call_ms"])}), flush=True)


if __name__ == "__main__":
    main()
