"""tests/refit_ref.py, the checker the GPU tests of mrt_update_spheres hold the device's refitted hierarchy to, against the host
builder (no GPU): it accepts what mrt_debug_build_hierarchy / mrt_debug_build_boxes_top_down build for a scene, and it rejects a
hierarchy that is stale or wrong in each of the ways a refit can be wrong."""
import ctypes as C

import numpy as np
import pytest

import refit_ref as R
from myraytracer_amd import _lib
from test_hierarchy_host import build, build_boxes, scenes


def host_hierarchy(mrt, sc, max_levels=4, top_target=0):
    """the host builder's arrays in the form mrt_debug_read_hierarchy reports the device's"""
    L = _lib.load()
    sc = np.ascontiguousarray(sc, mrt.SPHERE_DTYPE)
    h = build(mrt, sc, max_levels, top_target)
    h["box_quad"] = build_boxes(mrt, sc, max_levels, top_target)["quad"]
    info = (C.c_uint32 * 5)()
    assert L.mrt_debug_build_boxes_top_down(sc.ctypes.data, len(sc), max_levels, top_target, 0, None, 0, info) == 0
    for key, wide in (("boxes", 0), ("boxes_open", 1)):
        dev = np.zeros((info[1], 8), np.float32)
        assert L.mrt_debug_build_boxes_top_down(sc.ctypes.data, len(sc), max_levels, top_target, wide, dev.ctypes.data, len(dev), info) == 0
        h[key] = np.ascontiguousarray(dev[:, :6])
        if not wide:
            h["box_kc"] = np.float32(dev[:, 6].max()) if len(dev) else np.float32(0)
    if (max_levels, top_target) == (4, 0):              # (mrt_debug_build_sweep builds with the automatic depth rule)
        axis, org, reach = (C.c_float * 3)(), (C.c_float * 3)(), C.c_double()
        one = (C.c_float * 3)(1.0, 1.0, 1.0)
        assert L.mrt_debug_build_sweep(sc.ctypes.data, len(sc), one, axis, None, 0, None, 0, org, C.byref(reach)) == 0
        assert np.array_equal(np.array(list(org), np.float64), h["origin"])
        h["reach"] = reach.value
    return h


def moved(sc, rng, amount):
    """every sphere displaced by up to `amount` x the scene's size"""
    out = sc.copy()
    c = np.asarray(sc["center"], np.float64).reshape(-1, 3)
    size = float(np.ptp(c, axis=0).max()) if len(c) > 1 else 1.0
    out["center"] = (c + rng.uniform(-amount, amount, c.shape) * max(size, 1.0)).astype(np.float32)
    return out


def test_the_checker_accepts_what_the_host_builder_builds(mrt):
    for name, sc in scenes(mrt):
        for max_levels, target in [(4, 0), (4, 1), (2, 8), (3, 16)]:
            R.check(host_hierarchy(mrt, sc, max_levels, target), R.xyzr_of(sc))


@pytest.fixture(scope="module")
def large(mrt):
    """2,300 random spheres with a ground and negative radii (three levels, boxes): the scene, its hierarchy, the same moved"""
    sc = dict(scenes(mrt))["random 2300"]
    rng = np.random.default_rng(5)
    sc2 = moved(sc, rng, 0.3)
    return sc, host_hierarchy(mrt, sc), sc2, host_hierarchy(mrt, sc2)


def fresh(h):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in h.items()}


def test_a_hierarchy_built_for_the_old_positions_is_rejected(mrt, large):
    sc, h, sc2, h2 = large
    assert h["levels"] >= 2
    for part in (R.check_members, R.check_bounds, R.check_boxes, R.check):          # (the reach may still cover them)
        with pytest.raises(AssertionError):
            part(h, R.xyzr_of(sc2))
    R.check(h2, R.xyzr_of(sc2))


@pytest.mark.parametrize("where", ["top", "inner"])
def test_a_radius_record_shrunk_by_two_percent_is_rejected(mrt, large, where):
    sc, h, _, _ = large
    bad = fresh(h)
    recs = bad["top"] if where == "top" else bad["nodes"][bad["level_base"][1]:]
    j = int(np.nonzero(np.isfinite(recs[:, 3]))[0][3])
    recs[j, 3] *= np.float32(0.98 * 0.98)
    with pytest.raises(AssertionError, match="bounds"):
        R.check(bad, R.xyzr_of(sc))


def test_a_box_extent_short_by_kpad_is_rejected(mrt, large):
    sc, h, _, _ = large
    full = build_boxes(mrt, sc, 4, 0)
    top = full["boxes"][full["base"][h["levels"]]:]          # the top level's boxes: depth 0 of the kernel's numbering, index j
    for axis, j in ((0, int(np.nonzero(top[:, 3] >= 0)[0][0])), (2, int(np.nonzero(top[:, 3] >= 0)[0][-1]))):
        bad = fresh(h)
        assert bad["boxes"][j, 3 + axis] >= top[j, 3 + axis] + top[j, 7] > top[j, 3 + axis]
        bad["boxes"][j, 3 + axis] -= top[j, 7]
        with pytest.raises(AssertionError, match="boxes"):
            R.check(bad, R.xyzr_of(sc))


def test_a_member_record_left_at_its_old_centre_is_rejected(mrt, large):
    sc, h, sc2, h2 = large
    bad = fresh(h2)
    m = 41
    assert np.isfinite(bad["nodes"][m, 3])
    i = int(bad["midx"][m])
    bad["nodes"][m, :3] = np.asarray(sc["center"], np.float32).reshape(-1, 3)[i]
    assert not np.array_equal(bad["nodes"][m], h2["nodes"][m])
    with pytest.raises(AssertionError, match="members"):
        R.check(bad, R.xyzr_of(sc2))


def test_an_operand_ck_rounded_up_instead_of_down_is_rejected(mrt, large):
    sc, h, _, _ = large
    rec, v, raw = R.operand_rows(h)
    real = np.nonzero(np.isfinite(rec[:, 3]))[0]
    ck = v[:, 12:15].sum(axis=1)
    assert np.array_equal(ck.astype(np.float32).astype(np.float64), ck)          # the three pieces add up to one float32
    for row in real[:8]:
        bad = fresh(h)
        up = np.nextafter(np.float32(ck[row]), np.float32(np.inf))
        pieces = R.split3_bits(np.array([up], np.float32))
        mf = bad["mfma"].reshape(-1, 2, 32, 8)
        for q in range(3):
            mf[row // 32, 1, row % 32, 4 + q] = pieces[q][0]
        rec2, v2, _ = R.operand_rows(bad)
        assert v2[row, 12:15].sum() == np.float64(up)
        with pytest.raises(AssertionError, match="operand"):
            R.check(bad, R.xyzr_of(sc))
