"""CPU tests of reconfiguring a matcher: HipBlockMatcher.set_params (the binding of dsx_set_params,
include/dsx.h; configure_sgbm -> _build_sgbm, stereo_core.py:77-123) on a matcher that has no
handle yet, and dsx_set_params' own validation through the C-ABI.  No compute call, no device."""
from __future__ import annotations

import ctypes

import pytest

from depthestimation_amd import _dsx
from depthestimation_amd.matcher import HipBlockMatcher

# rejected combinations and the words dsx_last_error() must name the cause with
REJECTED = [
    (dict(block_size=4), "block_size"),
    (dict(cost="ssd", aggregation="hh"), "SGM aggregation"),
    (dict(sgbm_post=True, float_mode="parabola"), "float_mode must be fixed"),
]


def _state(m):
    return m.params, bytes(m._params), m._h


def test_set_params_without_a_handle_stores_the_set():
    m = HipBlockMatcher(num_disp=48, block_size=5)
    assert m._h is None
    m.set_params(num_disp=128, block_size=9, cost="bt", prefilter_cap=63, aggregation="hh", p1=50, p2=60000,
                 lr_form="sgbm", timing=True, min_disp=-3)
    assert m._h is None  # nothing is created before the first compute call
    p = m.params
    assert (p["num_disp"], p["block_size"], p["cost"], p["prefilter_cap"], p["aggregation"]) == (128, 9, "bt", 63, "hh")
    assert (p["p1"], p["p2"], p["lr_form"], p["timing"], p["min_disp"]) == (50, 60000, "sgbm", True, -3)
    assert (p["uniqueness_ratio"], p["disp12_max_diff"], p["path"]) == (10, 1, "fused")  # untouched keys stay
    s = m._params
    assert (s.num_disp, s.block_size, s.cost, s.prefilter_cap, s.aggregation) == (128, 9, 2, 63, 8)
    assert (s.p1, s.p2, s.lr_form, s.timing, s.min_disp) == (50, 60000, 1, 1, -3)
    assert (s.uniqueness_ratio, s.disp12_max_diff, s.path) == (10, 1, 0)
    assert m.getNumDisparities() == 128 and m.getBlockSize() == 9 and m.getMinDisparity() == -3
    # the struct is the one make_params builds from the merged dict
    assert bytes(s) == bytes(_dsx.make_params(**p))
    m.set_params()  # nothing to merge: still valid, nothing changes
    assert bytes(m._params) == bytes(s) and m.params == p


@pytest.mark.parametrize("kw,cause", REJECTED, ids=[",".join(k) for k, _ in REJECTED])
def test_rejected_sets_raise_and_change_nothing(kw, cause):
    m = HipBlockMatcher(num_disp=48, block_size=5, uniqueness_ratio=7)
    before = _state(m)
    with pytest.raises(ValueError, match=cause):
        m.set_params(**kw)
    assert _state(m) == before
    m.set_params(uniqueness_ratio=3)  # and the matcher still takes a valid set afterwards
    assert m.params["uniqueness_ratio"] == 3 and m._params.uniqueness_ratio == 3
    assert m.params["block_size"] == 5 and m.params["float_mode"] == "fixed" and m.params["cost"] == "sad"


@pytest.mark.parametrize("kw", [dict(device=1), dict(blocksize=7), dict(num_disp=64, focal_length=1.0)],
                         ids=["device", "misspelt", "valid_and_unknown"])
def test_unknown_keys_raise_and_change_nothing(kw):
    m = HipBlockMatcher(num_disp=48)
    before = _state(m)
    with pytest.raises(ValueError, match="unknown parameter"):
        m.set_params(**kw)
    assert _state(m) == before and m.device == 0


@pytest.mark.parametrize("kw", [dict(cost="census"), dict(lr_form="opencv"), dict(aggregation="sgm"),
                                dict(num_disp=None), dict(block_size="nine")])
def test_values_the_struct_cannot_hold_raise_value_error(kw):
    m = HipBlockMatcher(num_disp=48)
    before = _state(m)
    with pytest.raises(ValueError):
        m.set_params(**kw)
    assert _state(m) == before


@pytest.mark.parametrize("kw,cause", REJECTED, ids=[",".join(k) for k, _ in REJECTED])
def test_dsx_set_params_validates_before_it_looks_at_the_handle(kw, cause):
    lib = _dsx.lib()
    bad = _dsx.make_params(**kw)
    assert lib.dsx_set_params(None, ctypes.byref(bad)) == _dsx.DSX_EINVAL
    assert cause in _dsx.last_error()
    # the same words dsx_check_params gives
    msg = _dsx.last_error()
    assert lib.dsx_check_params(ctypes.byref(bad)) == _dsx.DSX_EINVAL and _dsx.last_error() == msg


def test_dsx_set_params_null_arguments():
    lib = _dsx.lib()
    good = _dsx.make_params(num_disp=64)
    assert lib.dsx_set_params(None, ctypes.byref(good)) == _dsx.DSX_EINVAL
    assert "handle is NULL" in _dsx.last_error()
    assert lib.dsx_set_params(None, None) == _dsx.DSX_EINVAL
    assert "params is NULL" in _dsx.last_error()
