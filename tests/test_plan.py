"""The matcher handle's pure decisions (csrc/dsx_plan.h): launch geometry, the SGM form and plan_call().

The header is plain C++; this test compiles a small harness against it with g++ (no HIP, no GPU) and
checks, over a table of parameter sets, that plan_call() takes the path, runs the stages and names the
buffers that include/dsx.h documents, restated here independently:
  - BT and census costs exist only as a volume; SGM runs on the volume; otherwise `path` decides;
  - a call handed a confidence output, and every call of a handle whose confidence threshold is > 0, runs
    the volume path (K2 has the variant); dsx_right_map_device is unaffected;
  - DSX_LR_FORM_SGBM is always on, the bm form runs when disp12_max_diff >= 0;
  - all SGM directions run in one u16 launch while max cost + P2 < 0xFFFF, else one u32 pass per direction;
  - a handle without prefilter, LR check and sgbm_post tail owns no scratch on the fused path;
  - buffers follow the handle's parameters (a fused handle keeps its LR buffers through confidence calls).
The table is the parameter walk of tests/test_gpu_handle_reuse.py plus what that file lacks (prefilter,
census, confidence, sgbm_post on a fused handle, right-map and process_pair calls).  The GPU side of the same
plan is tests/test_gpu_launch_plan.py.
"""
import os
import shutil
import subprocess

import pytest

import test_gpu_handle_reuse as walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "depthestimation_amd", "csrc")

HARNESS = r"""
#include "dsx_plan.h"
#include <cstdio>
#include <cstring>
int main() {
    char tag[8];
    while (scanf("%7s", tag) == 1) {
        if (!strcmp(tag, "G")) {  // cost D path aggregation no_sad1
            dsx_params p{};
            int no_sad1;
            if (scanf("%d %d %d %d %d", &p.cost, &p.num_disp, &p.path, &p.aggregation, &no_sad1) != 5) return 1;
            dsx::Geometry g{}, v{};
            const int ok = dsx::pick_geometry(p, no_sad1 != 0, g), vok = dsx::pick_volume_geometry(p, v);
            printf("%d %d %d %d %d %d %d %d %d %d %d\n", ok, g.NW, g.Dp, g.TPP, g.DB, g.kind, vok, v.NW, v.Dp, v.DB, v.kind);
        } else {  // the 20 words of dsx_params, then prefilter type / threshold, confidence threshold, the call
            dsx_params p{};
            dsx_prefilter f{};
            dsx_confidence c{};
            int32_t w[20];
            for (int i = 0; i < 20; ++i)
                if (scanf("%d", &w[i]) != 1) return 1;
            memcpy(&p, w, sizeof(w));
            int kind, conf_out, nframes, seq;
            if (scanf("%d %d %d %d %d %d %d", &f.type, &f.texture_threshold, &c.threshold, &kind, &conf_out, &nframes,
                      &seq) != 7)
                return 1;
            const dsx::CallPlan pl = dsx::plan_call(p, f, c, kind, conf_out != 0, nframes, seq != 0);
            printf("%d %d %d %d %d %d %d %d %d %d %d %u %d %llu %d %d\n", (int)pl.conf, (int)pl.fused, pl.builder, pl.lr,
                   pl.sgm, pl.sgm_ndir, (int)pl.scratch, (int)pl.prefilter, (int)pl.texture, (int)pl.post,
                   (int)pl.defer_lr_ok, pl.buffers, pl.nframes, (unsigned long long)dsx::max_cost(p), dsx::sgm_p2(p),
                   (int)dsx::sgm_concurrent(p, seq != 0));
        }
    }
    return 0;
}
"""

# include/dsx.h
COST = dict(sad=0, ssd=1, bt=2, census9x7=3, census5x5=4)
AGG = {None: 0, "sgbm_3way": 3, "hh4": 4, "sgbm": 5, "hh": 8}
COMPUTE, BATCH, RIGHT, PAIR_FAST, PAIR_FULL = range(5)
NONE, BLOCK, BT, CENSUS = range(4)            # builder
LR_NONE, LR_BM, LR_SGBM = range(3)
SGM_NONE, SGM_CONCURRENT, SGM_SEQUENTIAL = range(3)
BUF = dict(prefilter=1, lr=2, volume=4, bt=8, census=16, post=32, sgm_l=64, sgm_s=128, pair_disp=256,
           pair_fixed=512, pair_ws=1024)
FIELDS = ("min_disp", "num_disp", "block_size", "cost", "uniqueness_ratio", "disp12_max_diff", "subpixel",
          "float_mode", "path", "timing", "grid_blocks", "aggregation", "p1", "p2", "prefilter_cap", "sgbm_post",
          "speckle_window_size", "speckle_range", "lr_form", "in_flight")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("plan")
    src = d / "h.cpp"
    src.write_text(HARNESS)
    exe = d / "h"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(l + "\n" for l in lines), capture_output=True, text=True,
                             check=True).stdout
        rows = [list(map(int, line.split())) for line in out.strip().split("\n")]
        assert len(rows) == len(lines)
        return rows

    return run


def _words(p):
    w = dict(p, cost=COST[p["cost"]], aggregation=AGG[p["aggregation"]], subpixel=int(p["subpixel"]),
             float_mode=dict(fixed=0, parabola=1)[p["float_mode"]], path=dict(fused=0, volume=1)[p["path"]],
             timing=int(p["timing"]), sgbm_post=int(p["sgbm_post"]), lr_form=dict(bm=0, sgbm=1)[p["lr_form"]],
             in_flight=int(p["in_flight"]))
    return [w[k] for k in FIELDS]


def _max_cost(p):
    n = p["block_size"] ** 2
    if p["cost"] == "bt":
        return n * (2 * (max(p["prefilter_cap"], 15) | 1) + 63)
    return n * dict(sad=255, ssd=255 * 255, census9x7=62, census5x5=24)[p["cost"]]


def _expect(p, pf, thr, conf_t, kind, conf_out, seq):
    """The documented rules, for one row: every field the harness prints but the echoes."""
    volume_only = p["cost"] in ("bt", "census9x7", "census5x5")
    fused_handle = p["path"] == "fused" and not p["aggregation"] and not volume_only
    right = kind == RIGHT
    conf = not right and (conf_out or conf_t > 0)
    lr = LR_SGBM if p["lr_form"] == "sgbm" else (LR_BM if p["disp12_max_diff"] >= 0 else LR_NONE)
    p2 = p["p2"] if p["p2"] > 0 else 32 * p["block_size"] ** 2
    concurrent = not seq and _max_cost(p) + p2 < 0xFFFF
    ndir = {None: 0, "sgbm_3way": 3, "hh4": 4, "sgbm": 5, "hh": 8}[p["aggregation"]]
    need = set()
    if pf:
        need.add("prefilter")
    if lr != LR_NONE and fused_handle:
        need.add("lr")
    if not fused_handle or conf:
        need.add("volume")
    if p["cost"] == "bt":
        need.add("bt")
    if p["cost"].startswith("census"):
        need.add("census")
    if p["sgbm_post"]:
        need.add("post")
    if p["aggregation"]:
        need.add("sgm_l" if concurrent else "sgm_s")
    if kind == PAIR_FAST:
        need.add("pair_disp")
    if kind == PAIR_FULL:
        need |= {"pair_fixed", "pair_ws"}
    e = dict(conf=int(conf), buffers=sum(BUF[b] for b in need), prefilter=int(pf), ndir=ndir)
    if right:  # the right-view pass alone, behind the prefilter
        e.update(fused=0, builder=NONE, lr=LR_NONE, sgm=SGM_NONE, scratch=int(pf), texture=0, post=0, defer=0)
        return e
    fused = fused_handle and not conf
    e.update(fused=int(fused),
             builder=NONE if fused else (BT if p["cost"] == "bt" else CENSUS if volume_only else BLOCK),
             lr=lr, sgm=SGM_NONE if not p["aggregation"] else (SGM_CONCURRENT if concurrent else SGM_SEQUENTIAL),
             scratch=int(lr != LR_NONE or not fused or p["sgbm_post"] or pf), texture=int(pf and thr > 0),
             post=int(p["sgbm_post"]),
             defer=int(kind == PAIR_FULL and fused and not p["sgbm_post"] and lr != LR_NONE and thr == 0))
    return e


def _table():
    """(label, params, prefilter on, texture threshold, confidence threshold, kind, conf output, nframes, seq)"""
    P = {n: getattr(walk, n) for n in ("P1", "P3", "P4", "P5", "P6", "P7", "P8", "P9", "P10", "P11", "P12", "P15",
                                       "P15M", "P18")}
    P["P13a"] = dict(walk.P12, aggregation="hh4")
    P["P13b"] = dict(walk.P12, aggregation="sgbm")
    P["P14a"] = dict(walk.P12, p1=50, p2=60000)          # explicit penalties past the u16 bound
    P["P14edge"] = dict(walk.P12, p1=50, p2=0xFFFF - 255 * 81 - 1)   # the last explicit P2 below it
    P["P14at"] = dict(walk.P12, p1=50, p2=0xFFFF - 255 * 81)         # the first at it
    rows = []
    for name, p in P.items():
        rows.append((name, p, False, 0, 0, COMPUTE, False, 1, False))
        rows.append((name + " batch of 3", p, False, 0, 0, BATCH, False, 3, False))
    sad, vol = walk.P1, walk.P7
    assert sad["path"] == "fused" and sad["cost"] == "sad" and sad["num_disp"] <= 64   # the BM_SAD1 geometry
    rows += [
        ("prefilter", sad, True, 0, 0, COMPUTE, False, 1, False),
        ("prefilter + texture threshold", sad, True, 40, 0, COMPUTE, False, 1, False),
        ("prefilter, no LR", walk.P4, True, 0, 0, COMPUTE, False, 1, False),
        ("census 9x7", dict(sad, cost="census9x7"), False, 0, 0, COMPUTE, False, 1, False),
        ("census 5x5", dict(sad, cost="census5x5"), False, 0, 0, COMPUTE, False, 1, False),
        ("census 9x7 + hh, P2 60000", dict(sad, cost="census9x7", block_size=15, aggregation="hh", p1=50, p2=60000),
         False, 0, 0, COMPUTE, False, 1, False),
        ("BT 15 / 63 + hh, default penalties", dict(walk.P10, aggregation="hh"), False, 0, 0, COMPUTE, False, 1, False),
        ("BT 15 / 63 + hh, P2 at the bound", dict(walk.P10, aggregation="hh", p1=50, p2=0xFFFF - 225 * 189),
         False, 0, 0, COMPUTE, False, 1, False),
        ("DSX_SGM_SEQ", walk.P11, False, 0, 0, COMPUTE, False, 1, True),
        ("confidence output, fused SAD1 handle", sad, False, 0, 0, COMPUTE, True, 1, False),
        ("confidence threshold, fused SAD1 handle", sad, False, 0, 30, COMPUTE, False, 1, False),
        ("confidence threshold, batch", sad, False, 0, 30, BATCH, False, 3, False),
        ("confidence output, no LR", walk.P4, False, 0, 0, COMPUTE, True, 1, False),
        ("sgbm_post on a fused handle", dict(sad, sgbm_post=True), False, 0, 0, COMPUTE, False, 1, False),
        ("sgbm_post, no LR, batch", dict(walk.P4, sgbm_post=True), False, 0, 0, BATCH, False, 3, False),
        ("right map", sad, False, 0, 0, RIGHT, False, 1, False),
        ("right map, confidence threshold (no volume)", sad, False, 0, 30, RIGHT, False, 1, False),
        ("right map behind a prefilter", sad, True, 40, 0, RIGHT, False, 1, False),
        ("right map, volume handle", vol, False, 0, 0, RIGHT, False, 1, False),
        ("right map, SGM + sgbm_post handle", walk.P15, False, 0, 0, RIGHT, False, 1, False),
        ("process_pair fast", sad, False, 0, 0, PAIR_FAST, False, 1, False),
        ("process_pair full", sad, False, 0, 0, PAIR_FULL, False, 1, False),
        ("process_pair full, OpenCV's LR form", walk.P3, False, 0, 0, PAIR_FULL, False, 1, False),
        ("process_pair full, no LR", walk.P4, False, 0, 0, PAIR_FULL, False, 1, False),
        ("process_pair full, texture threshold", sad, True, 40, 0, PAIR_FULL, False, 1, False),
        ("process_pair full, confidence threshold", sad, False, 0, 30, PAIR_FULL, False, 1, False),
        ("process_pair full, sgbm_post", dict(sad, sgbm_post=True), False, 0, 0, PAIR_FULL, False, 1, False),
        ("process_pair full, volume handle", vol, False, 0, 0, PAIR_FULL, False, 1, False),
        ("process_pair fast, SGM", walk.P11, False, 0, 0, PAIR_FAST, False, 1, False),
    ]
    return rows


def test_plan_call_follows_the_documented_rules(harness):
    rows = _table()
    lines = [" ".join(map(str, ["P"] + _words(p) + [1 if pf else 0, thr, ct, kind, int(co), nf, int(seq)]))
             for (_, p, pf, thr, ct, kind, co, nf, seq) in rows]
    names = ("conf", "fused", "builder", "lr", "sgm", "ndir", "scratch", "prefilter", "texture", "post", "defer",
             "buffers", "nframes", "max_cost", "p2", "concurrent")
    seen = dict(fused=set(), builder=set(), lr=set(), sgm=set())
    for (label, p, pf, thr, ct, kind, co, nf, seq), got in zip(rows, harness(lines)):
        got = dict(zip(names, got))
        want = _expect(p, pf, thr, ct, kind, co, seq)
        for k, v in want.items():
            assert got[k] == v, (label, k, got, want)
        assert got["nframes"] == nf, label
        # the bound itself, with default and explicit penalties
        assert got["max_cost"] == _max_cost(p), label
        assert got["p2"] == (p["p2"] or 32 * p["block_size"] ** 2), label
        assert got["concurrent"] == int(not seq and got["max_cost"] + got["p2"] < 0xFFFF), label
        for k in seen:
            seen[k].add(got[k])
    # the table reaches every path, builder, LR form and SGM form
    assert seen == dict(fused={0, 1}, builder={NONE, BLOCK, BT, CENSUS}, lr={LR_NONE, LR_BM, LR_SGBM},
                        sgm={SGM_NONE, SGM_CONCURRENT, SGM_SEQUENTIAL}), seen


def test_sgm_form_flips_at_the_u16_bound(harness):
    """max cost + P2 = 0xFFFE runs concurrently, 0xFFFF (the u16 pad value) must not."""
    base = dict(walk.P12, p1=50)
    below, at = (dict(base, p2=0xFFFF - 255 * 81 - 1), dict(base, p2=0xFFFF - 255 * 81))
    lines = [" ".join(map(str, ["P"] + _words(p) + [0, 0, 0, COMPUTE, 0, 1, 0])) for p in (below, at)]
    (a, b) = harness(lines)
    assert (a[4], a[11] & (BUF["sgm_l"] | BUF["sgm_s"])) == (SGM_CONCURRENT, BUF["sgm_l"])
    assert (b[4], b[11] & (BUF["sgm_l"] | BUF["sgm_s"])) == (SGM_SEQUENTIAL, BUF["sgm_s"])


@pytest.mark.parametrize("cost", ["sad", "ssd"])
def test_geometry_of_both_layouts(harness, cost):
    """Dp / DB of the handle's geometry and of its volume geometry.  SAD lanes own disparity pairs (Dp =
    128 nw, nw <= 4), SSD lanes one disparity (Dp = 64 nw, nw <= 8); a fused SAD handle without aggregation
    takes the one-disparity layout for D <= 64 (BM_SAD1) unless DSX_NO_SAD1 is set, and its volume-path
    launches keep the pair layout.  DB = ceil(log2(Dp)).  Every layout reaches 512 disparities (dsx_check_params'
    bound); 513 is past all of them and is rejected."""
    SAD, SSD, SAD1 = 0, 1, 2
    Ds = (1, 48, 64, 65, 128, 129, 256, 512, 513)
    cases = [(D, path, agg, no) for D in Ds for path in (0, 1) for agg in (0, 8) for no in (0, 1)]
    rows = harness([f"G {COST[cost]} {D} {path} {agg} {no}" for (D, path, agg, no) in cases])

    def layout(D, lane1):
        unit, maxnw = (64, 8) if lane1 else (128, 4)
        nw = 1
        while nw * unit < D:
            nw *= 2
        return (nw, nw * unit) if nw <= maxnw else None

    for (D, path, agg, no), (ok, NW, Dp, TPP, DB, kind, vok, vNW, vDp, vDB, vkind) in zip(cases, rows):
        sad1 = cost == "sad" and D <= 64 and path == 0 and agg == 0 and not no
        want, wantv = layout(D, cost == "ssd" or sad1), layout(D, cost == "ssd")
        msg = (cost, D, path, agg, no)
        assert bool(ok) == (want is not None) and bool(vok) == (wantv is not None), msg
        assert kind == (SSD if cost == "ssd" else SAD1 if sad1 else SAD), msg
        assert vkind == (SSD if cost == "ssd" else SAD), msg
        if want:
            assert (NW, Dp, TPP) == (want[0], want[1], want[1] // 32) and 1 << DB == Dp, msg
        if wantv:
            assert (vNW, vDp) == wantv and 1 << vDB == vDp, msg
    assert {c[0] for c, r in zip(cases, rows) if not r[0]} == {513}


# Rows of the table with their plan written out by hand from include/dsx.h (not through _expect):
# label -> (conf, fused, builder, lr, sgm, directions, scratch, prefilter, texture, post, defer, buffers)
LITERAL = {
    "P1": (0, 1, NONE, LR_BM, SGM_NONE, 0, 1, 0, 0, 0, 0, {"lr"}),
    "P3": (0, 1, NONE, LR_SGBM, SGM_NONE, 0, 1, 0, 0, 0, 0, {"lr"}),
    "P4": (0, 1, NONE, LR_NONE, SGM_NONE, 0, 0, 0, 0, 0, 0, set()),          # the plain pass: no scratch, no buffer
    "P7": (0, 0, BLOCK, LR_BM, SGM_NONE, 0, 1, 0, 0, 0, 0, {"volume"}),
    "P8 batch of 3": (0, 0, BLOCK, LR_BM, SGM_NONE, 0, 1, 0, 0, 0, 0, {"volume"}),
    "P9": (0, 0, BT, LR_BM, SGM_NONE, 0, 1, 0, 0, 0, 0, {"volume", "bt"}),
    "P11": (0, 0, BLOCK, LR_BM, SGM_CONCURRENT, 3, 1, 0, 0, 0, 0, {"volume", "sgm_l"}),
    "P13a": (0, 0, BLOCK, LR_BM, SGM_CONCURRENT, 4, 1, 0, 0, 0, 0, {"volume", "sgm_l"}),
    "P13b": (0, 0, BLOCK, LR_BM, SGM_CONCURRENT, 5, 1, 0, 0, 0, 0, {"volume", "sgm_l"}),
    "P14a": (0, 0, BLOCK, LR_BM, SGM_SEQUENTIAL, 8, 1, 0, 0, 0, 0, {"volume", "sgm_s"}),
    "P15": (0, 0, BLOCK, LR_BM, SGM_CONCURRENT, 8, 1, 0, 0, 1, 0, {"volume", "sgm_l", "post"}),
    "BT 15 / 63 + hh, default penalties": (0, 0, BT, LR_BM, SGM_CONCURRENT, 8, 1, 0, 0, 0, 0, {"volume", "bt", "sgm_l"}),
    "BT 15 / 63 + hh, P2 at the bound": (0, 0, BT, LR_BM, SGM_SEQUENTIAL, 8, 1, 0, 0, 0, 0, {"volume", "bt", "sgm_s"}),
    "DSX_SGM_SEQ": (0, 0, BLOCK, LR_BM, SGM_SEQUENTIAL, 3, 1, 0, 0, 0, 0, {"volume", "sgm_s"}),
    "prefilter + texture threshold": (0, 1, NONE, LR_BM, SGM_NONE, 0, 1, 1, 1, 0, 0, {"prefilter", "lr"}),
    "prefilter, no LR": (0, 1, NONE, LR_NONE, SGM_NONE, 0, 1, 1, 0, 0, 0, {"prefilter"}),
    "census 9x7": (0, 0, CENSUS, LR_BM, SGM_NONE, 0, 1, 0, 0, 0, 0, {"volume", "census"}),
    "confidence output, fused SAD1 handle": (1, 0, BLOCK, LR_BM, SGM_NONE, 0, 1, 0, 0, 0, 0, {"lr", "volume"}),
    "confidence threshold, batch": (1, 0, BLOCK, LR_BM, SGM_NONE, 0, 1, 0, 0, 0, 0, {"lr", "volume"}),
    "confidence output, no LR": (1, 0, BLOCK, LR_NONE, SGM_NONE, 0, 1, 0, 0, 0, 0, {"volume"}),
    "sgbm_post, no LR, batch": (0, 1, NONE, LR_NONE, SGM_NONE, 0, 1, 0, 0, 1, 0, {"post"}),
    "right map": (0, 0, NONE, LR_NONE, SGM_NONE, 0, 0, 0, 0, 0, 0, {"lr"}),
    "right map, confidence threshold (no volume)": (0, 0, NONE, LR_NONE, SGM_NONE, 0, 0, 0, 0, 0, 0, {"lr"}),
    "right map behind a prefilter": (0, 0, NONE, LR_NONE, SGM_NONE, 0, 1, 1, 0, 0, 0, {"prefilter", "lr"}),
    "right map, volume handle": (0, 0, NONE, LR_NONE, SGM_NONE, 0, 0, 0, 0, 0, 0, {"volume"}),
    "process_pair fast": (0, 1, NONE, LR_BM, SGM_NONE, 0, 1, 0, 0, 0, 0, {"lr", "pair_disp"}),
    "process_pair full": (0, 1, NONE, LR_BM, SGM_NONE, 0, 1, 0, 0, 0, 1, {"lr", "pair_fixed", "pair_ws"}),
    "process_pair full, no LR": (0, 1, NONE, LR_NONE, SGM_NONE, 0, 0, 0, 0, 0, 0, {"pair_fixed", "pair_ws"}),
    "process_pair full, texture threshold": (0, 1, NONE, LR_BM, SGM_NONE, 0, 1, 1, 1, 0, 0,
                                             {"prefilter", "lr", "pair_fixed", "pair_ws"}),
    "process_pair full, confidence threshold": (1, 0, BLOCK, LR_BM, SGM_NONE, 0, 1, 0, 0, 0, 0,
                                                {"lr", "volume", "pair_fixed", "pair_ws"}),
    "process_pair full, sgbm_post": (0, 1, NONE, LR_BM, SGM_NONE, 0, 1, 0, 0, 1, 0,
                                     {"lr", "post", "pair_fixed", "pair_ws"}),
}


def test_plan_call_literal_rows(harness):
    rows = {r[0]: r for r in _table()}
    assert set(LITERAL) <= set(rows)
    labels = list(LITERAL)
    lines = []
    for label in labels:
        (_, p, pf, thr, ct, kind, co, nf, seq) = rows[label]
        lines.append(" ".join(map(str, ["P"] + _words(p) + [1 if pf else 0, thr, ct, kind, int(co), nf, int(seq)])))
    for label, got in zip(labels, harness(lines)):
        want = LITERAL[label]
        assert tuple(got[:11]) == want[:11], (label, got[:11], want[:11])
        assert got[11] == sum(BUF[b] for b in want[11]), (label, got[11], want[11])
