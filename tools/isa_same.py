"""Is the fused pass's device code the same as at a base revision?

Cross-compiles depthestimation_amd/csrc/dsx_bm.hip of the working tree and of `git show <rev>:...` (with the
headers it includes) to gfx950 assembly, one unit per block radius plus the dispatch unit, with the Makefile's
flags, and compares every kernel: the instruction text of its body and its descriptor block (VGPRs, SGPRs,
scratch, LDS, ...).  One line per kernel; exit status 1 on any difference or if the symbol sets differ.
Identity only: nothing here looks at what the instructions are.

usage: python tools/isa_same.py --base <rev> [--flags "-D..."] [--radii 0..7,dispatch] [--jobs N]
"""
from __future__ import annotations

import argparse
import hashlib
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from valu_roofline import ROOT, function_body  # noqa: E402

CSRC = "depthestimation_amd/csrc"
FILES = [f"{CSRC}/dsx_bm.hip", f"{CSRC}/dsx_internal.h", f"{CSRC}/dsx_plan.h", f"{CSRC}/dsx_partition.h",
         f"{CSRC}/dsx_subpix.h", "include/dsx.h"]
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"  # the Makefile's FLAGS


def units(spec: str):
    out = []
    for part in spec.split(","):
        if ".." in part:
            lo, hi = part.split("..")
            out += [str(r) for r in range(int(lo), int(hi) + 1)]
        else:
            out.append(part)
    return out


def compile_unit(tree: str, unit: str, extra: list, out: str):
    rad = [] if unit == "dispatch" else [f"-DDSX_RADIUS={unit}"]
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS.split(), *rad, *extra, "--cuda-device-only", "-S", "-o", out,
                    os.path.join(tree, CSRC, "dsx_bm.hip")], check=True)
    return out


def kernels(asm_path: str):
    """{symbol: (instruction count, sha256 of instruction text + descriptor)}"""
    asm = open(asm_path).read()
    out = {}
    for sym, desc in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S):
        lines = [re.sub(r"\s*;.*$", "", ln) for ln in function_body(asm, sym).split("\n")]
        lines = [ln for ln in lines if ln.startswith(".LBB") or (ln.strip() and not ln.strip().startswith("."))]
        insts = sum(1 for ln in lines if ln.startswith("\t"))
        desc = "\n".join(ln.strip() for ln in desc.split("\n"))
        out[sym] = (insts, hashlib.sha256(("\n".join(lines) + "\n--\n" + desc).encode()).hexdigest())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--base", default="HEAD")
    ap.add_argument("--flags", default="")
    ap.add_argument("--radii", default="0..7,dispatch")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    argv = sys.argv[1:]
    if "--flags" in argv[:-1]:  # its value begins with a dash: hand it over as --flags=VALUE
        i = argv.index("--flags")
        argv[i:i + 2] = ["--flags=" + argv[i + 1]]
    args = ap.parse_args(argv)
    extra, us = shlex.split(args.flags), units(args.radii)
    rev = subprocess.run(["git", "rev-parse", "--short", args.base], cwd=ROOT, check=True, capture_output=True,
                         text=True).stdout.strip()
    print(f"# isa_same: working tree against {rev}, flags '{args.flags}', units {','.join(us)}")
    bad = False
    with tempfile.TemporaryDirectory(prefix="isa_same_") as tmp:
        for f in FILES:
            dst = os.path.join(tmp, "base", f)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            with open(dst, "wb") as fh:
                fh.write(subprocess.run(["git", "show", f"{args.base}:{f}"], cwd=ROOT, check=True, capture_output=True).stdout)
        with ThreadPoolExecutor(max(1, min(16, args.jobs))) as pool:
            jobs = {(side, u): pool.submit(compile_unit, tree, u, extra, os.path.join(tmp, f"{side}_{u}.s"))
                    for side, tree in (("base", os.path.join(tmp, "base")), ("new", ROOT)) for u in us}
            asm = {k: j.result() for k, j in jobs.items()}
        for u in us:
            kb, kn = kernels(asm["base", u]), kernels(asm["new", u])
            for sym in sorted(set(kb) - set(kn)):
                print(f"{u} {sym} only in base  DIFFERENT")
            for sym in sorted(set(kn) - set(kb)):
                print(f"{u} {sym} only in new  DIFFERENT")
            bad |= set(kb) != set(kn)
            for sym in sorted(set(kb) & set(kn)):
                same = kb[sym] == kn[sym]
                bad |= not same
                print(f"{u} {sym} insts {kb[sym][0]}/{kn[sym][0]} base {kb[sym][1][:16]} new {kn[sym][1][:16]} "
                      f"{'same' if same else 'DIFFERENT'}")
            if not kb and not kn:
                print(f"{u} (no kernels in this unit on either side)")
    print("# result:", "DIFFERENT" if bad else "all same")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
