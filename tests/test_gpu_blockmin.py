"""Block minima of the rotated row loop of the fused SAD pass (csrc/dsx_bm.hip, bm2<R, SAD, 1, 0> with R <= 5):
-DDSX_ROWSTEP_BLOCKMIN, default 1 - the minimum of a 16-byte tile block takes v_pk_minimum3_f16 of three of its words
and one integer packed minimum with the fourth (block_min8, csrc/dsx_internal.h), and the host pads the tile with
0x7BFF, the largest finite f16 pattern, instead of 0xFFFF.

What this form can get wrong, and the cases for it:
  * costs that are small as f16 patterns: identical views (every cost 0) and views 0 .. 3 grey levels apart (every
    window sum below 1,024, the denormal patterns, which a flushing minimum would turn into 0);
  * costs at the top of the range: views of 0 against 255 at R = 5 (30,855 = 0x7887) and R = 4 (20,655), alone and
    mixed with zero columns, and next to the padding (D = 127, D = 100: 0x7BFF must lose against 0x7887);
  * every radius that runs this loop (R = 0, 2, 3, 4, 5), on frames that hold a strip of the unaligned-dword copy
    and clamped strips, the ragged last one included;
  * the padding: D = 127 (the odd-D overwrite) and D = 100 (padded blocks), random views and a winner at d = D - 1,
    the last real disparity, next to the padding;
  * ties: equal minima first in every block (element 0), in the two blocks that a key pair of the epilogue folds
    and across pair boundaries (blocks 1|2, 3|4), and in the slices of the two lanes of a pixel (d against d + 64);
    the winner is the lowest disparity.  Every tie is first shown on the CPU in the oracle's cost rows;
  * uniqueness_ratio 10 and 15: that branch reads the blocks again through the same minimum, and compares its result
    with the padding value;
  * each output alone, a batch of two frames, three in_flight handles on three streams;
  * the primitive alone (dsx_block_min8_device): every block of eight costs drawn from 0, 1, 0x03FF, 0x0400, 0x7887,
    0x7BFF and 2^20 seeded blocks of costs below 0x7C00, against the integer minimum, equal bits.

Every map is compared bit for bit over all pixels against the C oracle (oracle/cref.py).  The cases hold for both
settings of the switch; the file was run on the default build and on the build with the switch off.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from depthestimation_amd.synthetic import stereo_pair

import fused_geometry as fg

pytestmark = pytest.mark.gpu

M, D = 0, 128
BASE = dict(cost="sad", disp12_max_diff=-1)
SHAPES = [(12, 224), (24, 330)]
BLOCKS = [1, 5, 7, 9, 11]  # R = 0, 2, 3, 4, 5
GRIDS = (0, 5)  # the default grid and five blocks (segments of many rows, cut inside strips)
TH, TW = SHAPES[0]
TX0 = 160  # the unaligned strip of the 224-column frame, R <= 5


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _strips(H, W, bs, d=D):
    """(x0 of the unaligned strips, of the clamped strips left of them, of the clamped strips right of them)"""
    bl = fg.blocks(H, 0, W, M, 1, bs // 2, d)
    f = sorted({s.x0 for b in bl for s in b if s.fast})
    c = sorted({s.x0 for b in bl for s in b if not s.fast})
    return f, [x for x in c if f and x < f[0]], [x for x in c if f and x > f[-1]]


def _pair(H, W, d=D, seed=0):
    L, R, _ = stereo_pair(H, W, M, d, seed=8200 + 17 * H + W + seed)
    return L, R


def _run(torch, dL, dR, shape, want, what, fmode="fixed", outs="both", **kw):
    from depthestimation_amd.matcher import HipBlockMatcher
    for g in GRIDS:
        mt = HipBlockMatcher(grid_blocks=g, float_mode=fmode, **kw)
        try:
            fx = torch.empty(shape, dtype=torch.int16, device="cuda") if outs in ("both", "fixed") else None
            fl = torch.empty(shape, dtype=torch.float32, device="cuda") if outs in ("both", "float") else None
            mt.compute_device(dL, dR, out_fixed=fx, out_float=fl)
            torch.cuda.synchronize()
            fg.check_maps(fx, fl, want, f"{what} grid_blocks={g} outs={outs}", fmode)
        finally:
            mt.close()


def _case(torch, key, L, R, what, bs=9, d=D, u=0, fmodes=("fixed", "parabola"), **run_kw):
    kw = dict(BASE, min_disp=M, num_disp=d, block_size=bs, uniqueness_ratio=u, subpixel=True)
    want = fg.want(key, L, R, M, d, bs, u)
    dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    for fmode in fmodes:
        _run(torch, dL, dR, L.shape, want, f"{what} {fmode}", fmode=fmode, **run_kw, **kw)
    return want


def _costs(L, R, bs, d=D):
    from oracle.stereo_bm import cost_volume
    return cost_volume(L, R, M, d, bs, "sad")


def test_geometry():
    """Both frames hold an unaligned strip and clamped strips left of it at every radius; the 330-column frame ends in
    a ragged clamped strip; D = 100 and D = 127 keep an unaligned strip."""
    for (H, W) in SHAPES:
        for bs in BLOCKS:
            f, left, right = _strips(H, W, bs)
            assert f and left, (H, W, bs)
            assert right or W == 224, (H, W, bs)
    assert 330 % fg.TX != 0  # a ragged last strip
    assert TX0 in _strips(TH, TW, 9)[0] and TX0 in _strips(TH, TW, 11)[0]
    for d in (100, 127):
        assert _strips(TH, TW, 9, d)[0] and _strips(TH, TW, 11, d)[0]


# ---- every radius of the rotated loop ------------------------------------------------------------------

@pytest.mark.parametrize("bs", BLOCKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_frames(torch_dev, shape, bs):
    H, W = shape
    L, R = _pair(H, W)
    _case(torch_dev, ("random", H, W), L, R, f"{H}x{W} block {bs}", bs=bs)


# ---- the bottom of the cost range ----------------------------------------------------------------------

def _flat(seed, lo, hi, shape=SHAPES[1]):
    return np.random.default_rng(seed).integers(lo, hi + 1, shape, dtype=np.uint8)


@pytest.mark.parametrize("bs", [11, 9, 5, 1])
def test_zero_costs(torch_dev, bs):
    """Identical constant views: every cost of every disparity is 0; the winner is d = 0."""
    L = np.full(SHAPES[1], 131, np.uint8)
    assert np.all(_costs(L, L, bs) == 0)
    want = _case(torch_dev, ("zero",), L, L, f"zero costs block {bs}", bs=bs)
    assert np.all(want["fixed"][:, D - 1:] == 0)


@pytest.mark.parametrize("u", [0, 10])
@pytest.mark.parametrize("bs", [11, 9, 7, 5, 1])
@pytest.mark.parametrize("spread", [1, 2, 3])
def test_denormal_range(torch_dev, spread, bs, u):
    """Views whose pixels lie within `spread` grey levels: every window sum is at most 121 * 3 = 363 < 1,024, so every
    cost is an f16 denormal pattern (or 0), and many minima are small and distinct."""
    L, R = _flat(10 + spread, 100, 100 + spread), _flat(20 + spread, 100, 100 + spread)
    C = _costs(L, R, bs)
    assert 0 < C.max() < 1024
    _case(torch_dev, ("denormal", spread), L, R, f"denormal range spread {spread} block {bs} u={u}", bs=bs, u=u)


# ---- the top of the cost range -------------------------------------------------------------------------

@pytest.mark.parametrize("d", [128, 127, 100])
@pytest.mark.parametrize("bs", [11, 9])
def test_top_of_the_range(torch_dev, bs, d):
    """0 against 255: every real cost is 255 * bs^2 (30,855 = 0x7887 at R = 5, 20,655 at R = 4), the largest the
    kernels form, and with D < 128 it stands next to the padding value 0x7BFF, which must not win: d = 0 does."""
    L, R = np.zeros((TH, TW), np.uint8), np.full((TH, TW), 255, np.uint8)
    assert np.all(_costs(L, R, bs, d) == 255 * bs * bs) and 255 * bs * bs in (30855, 20655)
    want = _case(torch_dev, ("opposed",), L, R, f"0 / 255 block {bs} D={d}", bs=bs, d=d)
    assert np.all(want["fixed"][:, d - 1:] == 0)
    for u in (10, 15):  # the second minimum equals the first: the ratio test rejects, the padding must not count
        _case(torch_dev, ("opposed",), L, R, f"0 / 255 block {bs} D={d} u={u}", bs=bs, d=d, u=u, fmodes=("fixed",))
    # columns of 0 and 255 at random: costs from 0 to the maximum in steps of 255 * bs
    bits = _flat(bs + d, 0, 1, (1, TW))
    bits[:, 40:56], bits[:, 100:116] = 1, 0  # a window of each kind for every block size
    Rm = np.ascontiguousarray(np.broadcast_to(bits * np.uint8(255), (TH, TW)))
    C = _costs(L, Rm, bs, d)
    assert C.max() == 255 * bs * bs and C.min() == 0
    _case(torch_dev, ("opposed columns",), L, Rm, f"0 / 255 columns block {bs} D={d}", bs=bs, d=d)


# ---- padding -------------------------------------------------------------------------------------------

def _noise(seed):
    return np.random.default_rng(seed).integers(0, 256, (TH, TW), dtype=np.uint8)


def _periodic(seed, period):
    """Noise that repeats every `period` columns."""
    return np.ascontiguousarray(np.tile(_noise(seed)[:, :period], (1, TW // period + 1))[:, :TW])


def _shift(R, s):
    """L with L(x) = R(x - s) (columns left of s: R's first column, as the clamped search reads it)"""
    return np.ascontiguousarray(R[:, np.clip(np.arange(R.shape[1]) - s, 0, R.shape[1] - 1)])


@pytest.mark.parametrize("d", [100, 127])
@pytest.mark.parametrize("bs", [11, 9, 5, 1])
def test_padded_and_odd_range(torch_dev, d, bs):
    """D = 100: 28 padding disparities, whole padded blocks.  D = 127: the last pair's high half is overwritten with
    the padding value.  Random views, with and without the uniqueness test, and a zero-cost winner at d = D - 1."""
    L, R = _pair(TH, TW, d=d, seed=d)
    _case(torch_dev, ("random", d), L, R, f"D={d} block {bs}", bs=bs, d=d)
    _case(torch_dev, ("random", d), L, R, f"D={d} block {bs} u=15", bs=bs, d=d, u=15, fmodes=("fixed",))
    Rr = _periodic(d, 160)
    want = _case(torch_dev, ("last", d), _shift(Rr, d - 1), Rr, f"D={d} winner D-1 block {bs}", bs=bs, d=d,
                 fmodes=("fixed",))
    if bs > 1:  # (a one-pixel block meets its value at lower disparities too)
        f = _strips(TH, TW, bs, d)[0]
        assert np.all(want["fixed"][:, f[0]:f[0] + fg.TX] == 16 * (d - 1))


# ---- tie order -----------------------------------------------------------------------------------------

# ("periodic", p, s): a right view of period p and the left view s < p columns on - zero cost at d = s, s + p, ...
# ("adjacent", d): the two equal minima of a row at d and d + 1, nothing else tied
TIES = {
    "every block, element 0": ("periodic", 8, 0),    # d = 0, 8, 16, ...: first in each of the 16 blocks
    "every block, element 7": ("periodic", 8, 7),    # last in each block
    "even blocks": ("periodic", 16, 0),              # blocks 0, 2, 4, ...: the first block of each key pair
    "odd blocks": ("periodic", 16, 8),               # blocks 1, 3, 5, ...: the second block of each key pair
    "blocks 1, 4, 7, 10, 13": ("periodic", 24, 8),   # first and second blocks of pairs, both lanes' slices
    "blocks 2, 5, 8, 11, 14": ("periodic", 24, 16),
    "lanes, d 5 / 69": ("periodic", 64, 5),          # block 0 of lane 0's slice against block 0 of lane 1's
    "lanes, d 63 / 127": ("periodic", 64, 63),       # the last element of each slice
    "blocks 0|1": ("adjacent", 7),                   # inside a key pair
    "blocks 1|2": ("adjacent", 15),                  # across pair boundaries
    "blocks 3|4": ("adjacent", 31),
    "blocks 5|6": ("adjacent", 47),
    "blocks 7|8": ("adjacent", 63),                  # lane 0's last disparity against lane 1's first
    "blocks 9|10": ("adjacent", 79),
}


def _tie(name):
    """(L, R, tied disparities)"""
    kind, *a = TIES[name]
    if kind == "periodic":
        p, s = a
        R = _periodic(100 * p + s, p)
        return _shift(R, s), R, list(range(s, D, p))
    # right view: an even triangle wave of period 160 (> D: one pair of minima in range) whose phase moves with the
    # row; the left pixel lies midway between the right pixels it meets at d and d + 1, so every term of the two costs
    # is the same, and on the wave's slopes a term is |2 (d' - d) - 1| at disparity d'
    d, = a
    x, y = np.meshgrid(np.arange(TW), np.arange(TH))
    R = (40 + 2 * np.abs((x + 13 * y) % 160 - 80)).astype(np.uint8)
    L = ((_shift(R, d).astype(np.int64) + _shift(R, d + 1)) // 2).astype(np.uint8)
    return L, R, [d, d + 1]


@pytest.mark.parametrize("bs", [9, 11, 5])
@pytest.mark.parametrize("name", list(TIES))
def test_tie_order(torch_dev, name, bs):
    L, R, tied = _tie(name)
    # the oracle's cost rows in the band's part of the unaligned strip hold the tie: the tied disparities at the row's
    # minimum, none below the first
    C = _costs(L, R, bs)[:, TX0:TX0 + fg.TX]
    cmin = C.min(axis=2)
    assert len(tied) >= 2 and all(np.all(C[:, :, d] == cmin) for d in tied), name
    assert np.all(C[:, :, :tied[0]] > cmin[..., None]), name
    assert np.all((C == cmin[..., None]).sum(axis=2) == len(tied)), name
    want = _case(torch_dev, ("tie", name), L, R, f"tie {name} block {bs}", bs=bs)
    # the lowest tied disparity: C(d + 1) = C(d) < C(d - 1) puts the parabola's vertex at d + 1/2, 8 in x16; between
    # tied blocks the sub-pixel step is at most half a disparity
    w = want["fixed"][:, TX0:TX0 + fg.TX].astype(np.int64)
    if TIES[name][0] == "adjacent":
        assert np.all(w == 16 * tied[0] + 8), name
    else:
        assert np.all(np.abs(w - 16 * tied[0]) <= 8), name
    for u in (10, 15):  # the second minimum equals the first, or lies next to it and is left out
        _case(torch_dev, ("tie", name), L, R, f"tie {name} block {bs} u={u}", bs=bs, u=u, fmodes=("fixed",))


# ---- uniqueness ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("u", [10, 15])
@pytest.mark.parametrize("bs", [11, 9, 7, 1])
def test_uniqueness(torch_dev, bs, u):
    H, W = SHAPES[1]
    L, R = _pair(H, W, seed=u)
    want = _case(torch_dev, ("random", H, W, "u"), L, R, f"u={u} block {bs}", bs=bs, u=u)
    band = want["fixed"][:, D - 1:]
    # the branch decides both ways (a one-pixel block finds a zero cost nearly everywhere, and zero passes the test)
    assert (band != -16).any() and ((band == -16).any() or bs == 1)


# ---- outputs and launches ------------------------------------------------------------------------------

@pytest.mark.parametrize("outs", ["fixed", "float"])
@pytest.mark.parametrize("fmode", ["fixed", "parabola"])
def test_one_output(torch_dev, outs, fmode):
    H, W = SHAPES[1]
    L, R = _pair(H, W)
    for bs in (9, 11):
        _case(torch_dev, ("random", H, W), L, R, f"block {bs}", bs=bs, fmodes=(fmode,), outs=outs)


def test_batch_of_two_frames(torch_dev):
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    (H, W), NF = SHAPES[1], 2
    fr = [_pair(H, W), (_flat(31, 100, 103), _flat(32, 100, 103))]  # a random frame and one in the denormal range
    dL = torch.from_numpy(np.stack([f[0] for f in fr])).cuda()
    dR = torch.from_numpy(np.stack([f[1] for f in fr])).cuda()
    for bs in (9, 11):
        wants = [fg.want(("batch", i), L, R, M, D, bs, 10) for i, (L, R) in enumerate(fr)]
        for g in GRIDS:
            mt = HipBlockMatcher(grid_blocks=g, uniqueness_ratio=10, min_disp=M, num_disp=D, block_size=bs, **BASE)
            try:
                fx = torch.empty((NF, H, W), dtype=torch.int16, device="cuda")
                fl = torch.empty((NF, H, W), dtype=torch.float32, device="cuda")
                mt.compute_batch_device(dL, dR, out_fixed=fx, out_float=fl)
                torch.cuda.synchronize()
                for i in range(NF):
                    fg.check_maps(fx[i], fl[i], wants[i], f"batch block {bs} grid_blocks={g} frame={i}")
            finally:
                mt.close()


def test_three_handles_in_flight(torch_dev):
    """Three in_flight handles on three streams, three frames each, every output checked."""
    torch = torch_dev
    from depthestimation_amd.matcher import HipBlockMatcher
    (H, W), NF = SHAPES[1], 3
    grids = (0, 5, 0)
    fr = [_pair(H, W, seed=s) for s in range(NF)]
    wants = [fg.want(("random", H, W, i), L, R, M, D, 9, 0) for i, (L, R) in enumerate(fr)]
    dev = [(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in fr]
    mts = [HipBlockMatcher(in_flight=True, grid_blocks=g, uniqueness_ratio=0, min_disp=M, num_disp=D, block_size=9, **BASE)
           for g in grids]
    sts = [torch.cuda.Stream() for _ in grids]
    fx = [[torch.empty((H, W), dtype=torch.int16, device="cuda") for _ in range(NF)] for _ in grids]
    fl = [[torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(NF)] for _ in grids]
    torch.cuda.synchronize()
    try:
        for i in range(NF):
            for h, (mt, st) in enumerate(zip(mts, sts)):
                mt.compute_device(dev[i][0], dev[i][1], out_fixed=fx[h][i], out_float=fl[h][i], stream=st)
        torch.cuda.synchronize()
        for h in range(len(grids)):
            for i in range(NF):
                fg.check_maps(fx[h][i], fl[h][i], wants[i], f"handle {h} (grid_blocks={grids[h]}) frame {i}")
    finally:
        for mt in mts:
            mt.close()


# ---- the primitive alone -------------------------------------------------------------------------------

BOUNDARY = np.array([0, 1, 0x03FF, 0x0400, 0x7887, 0x7BFF], np.uint16)


def test_block_min8_primitive(torch_dev):
    """v_pk_minimum3_f16 of three words and the integer minima of the rest against numpy's minimum of the eight
    costs: all 6^8 blocks of boundary patterns (zero, the smallest and the largest denormal, the smallest normal,
    the largest cost, the padding) and 2^20 seeded blocks of costs below 0x7C00.  One launch, equal bits."""
    torch = torch_dev
    from depthestimation_amd import _dsx
    idx = np.indices((len(BOUNDARY),) * 8, dtype=np.uint8).reshape(8, -1).T
    blocks = np.concatenate([BOUNDARY[idx], np.random.default_rng(950).integers(0, 0x7C00, (1 << 20, 8), dtype=np.uint16)])
    assert blocks.shape == (6 ** 8 + (1 << 20), 8) and blocks.max() == 0x7BFF
    n = blocks.shape[0]
    dev = torch.from_numpy(blocks.view(np.int16)).cuda()
    out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc = _dsx.lib().dsx_block_min8_device(ctypes.c_void_p(dev.data_ptr()), n, ctypes.c_void_p(out.data_ptr()), None)
    assert rc == 0, _dsx.lib().dsx_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    want = blocks.min(axis=1).astype(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (len(bad), blocks[bad[0]].tolist(), int(got[bad[0]]), int(want[bad[0]]))
