"""mrt_set_auto_regroup on the GPU (include/myraytracer_amd.h, "scene"; myraytracer_amd/csrc/regroup_policy.hip): the hierarchy
judged on the device at every check_every-th mrt_update_spheres, the regroup gated by the verdict.

The device is held to tests/regroup_policy_ref.py bit for bit: the figure it stores is the reference's figure of the hierarchy
read back with mrt_debug_read_hierarchy (the same order of additions), and the reference's state machine, fed those figures,
predicts checks, regroups, q_ref, q_last and whether member_index changes.  A regroup the gate lets run is
tests/regroup_ref.py's ordering of the current spheres, as for mrt_regroup_spheres; a check that does not fire leaves every array
what it is with the policy off; frames are the oracle's whatever the gate does.  tests/test_regroup_policy_host.py shows on the
host that the motions used here fire (and do not) as these tests need.  Images are 20 x 12, 2 spp, depth 8; scenes, motions and
layouts are those of tests/test_gpu_update_spheres.py and tests/test_gpu_regroup.py."""
import numpy as np
import pytest

import refit_ref as R
import regroup_policy_ref as P
import regroup_ref as G
from test_gpu_regroup import same_hierarchy, scene_of, state
from test_gpu_update_spheres import DEPTH, H, SEED, SPP, W, assert_same, motion, oracle_frames, scene

pytestmark = pytest.mark.gpu

MRT_ERR_INVALID_ARG, MRT_ERR_NO_SCENE = 1, 4
DEFAULTS = dict(enabled=False, ratio=P.DEFAULT_RATIO, check_every=P.DEFAULT_CHECK_EVERY)


def assert_stats(st, s, what=""):
    """the device's state is the reference machine's state s, bit for bit"""
    got = st.read_regroup_stats()
    want = dict(checks=s["checks"], regroups=s["regroups"], q_ref=s["q_ref"], q_last=s["q_last"], q_level=s["q_level"], pending=s["pending"])
    assert {k: got[k] for k in want} == want, what
    return got


@pytest.mark.parametrize("name", ["small", "ragged", "alone", "large-quad"])
def test_enabling_takes_the_baseline(mrt, name):
    sc = scene_of(mrt, name)
    with state(mrt, name, sc) as st:
        before = st.read_regroup_stats()
        st.set_auto_regroup(True)
        got, h, n_pool = st.read_regroup_stats(), st.debug_read_hierarchy(), st.debug_regroup_info()["n_pool"]
        assert st.debug_check_context() is None
    assert before == dict(checks=0, regroups=0, q_ref=0.0, q_last=0.0, q_level=[0.0] * h["levels"], levels=h["levels"], pending=True)
    levels, q = P.quality(h, n_pool)
    assert got["levels"] == h["levels"] == (3 if name == "large-quad" else 1) and q > 0.0
    assert got["q_level"] == levels and got["q_ref"] == q and got["q_last"] == q          # (floats compared exactly: the same bits)
    assert (got["checks"], got["regroups"], got["pending"]) == (0, 0, False)
    if name == "alone":                                                 # the three clusters behind the pool would dominate the figure
        assert P.quality(h, n_pool, "non_pool")[1] > 10.0 * q


@pytest.mark.parametrize("name,block", [("small", 4), ("large-quad", None)])
def test_a_check_that_does_not_fire_changes_nothing(mrt, name, block):
    sc = scene_of(mrt, name)
    xyzr = R.xyzr_of(sc)
    out = {}
    for on in (True, False):
        with state(mrt, name, sc, block=block) as st:
            if on:
                st.set_auto_regroup(True, check_every=1)
            st.update_spheres(0, xyzr)
            st.update_spheres(0, xyzr)
            out[on] = st.debug_read_hierarchy()
            stats = st.read_regroup_stats()
            assert (stats["checks"], stats["regroups"], stats["pending"]) == ((2, 0, False) if on else (0, 0, True))
            assert st.debug_check_context() is None
    same_hierarchy(out[True], out[False])


FIRING = [("small", 4), ("small", None), ("large-quad", None), ("boxes-4200", None)]


@pytest.mark.parametrize("name,block", FIRING, ids=[f"{n}-{b or 'default'}" for n, b in FIRING])
def test_a_check_that_fires_regroups_the_current_spheres(mrt, name, block):
    sc = scene_of(mrt, name)
    first, upd, sc_new = motion(mrt, sc, "scatter")
    with state(mrt, name, sc, block=block) as st:
        st.set_auto_regroup(True, check_every=1)
        before, n_pool = st.debug_read_hierarchy(), st.debug_regroup_info()["n_pool"]
        s = P.baseline(P.new_state(), *P.quality(before, n_pool), mark=True)
        st.update_spheres(first, upd)                                   # its check sees the build's bounds
        s, fired = P.decide(s, *P.quality(before, n_pool), P.DEFAULT_RATIO)
        loose = st.debug_read_hierarchy()
        assert not fired and np.array_equal(loose["midx"], before["midx"])
        assert_stats(st, s, "the first update")
        st.update_spheres(first, upd)                                   # the same spheres again: its check sees the loosened bounds
        s, fired = P.decide(s, *P.quality(loose, n_pool), P.DEFAULT_RATIO)
        h = st.debug_read_hierarchy()
        assert fired
        s = P.baseline(s, *P.quality(h, n_pool))
        got = assert_stats(st, s, "the second update")
        assert st.debug_check_context() is None
    assert (got["checks"], got["regroups"], got["pending"]) == (2, 1, False) and got["q_ref"] == P.quality(h, n_pool)[1]
    real, xyzr = G.real_slots(before), R.xyzr_of(sc_new)
    want = G.regroup(before["midx"], real, n_pool, xyzr[:, :3])
    bad = np.nonzero(h["midx"] != want)[0]
    assert len(bad) == 0, f"{len(bad)} member slots differ from the reference; first: slot {bad[0]} holds {h['midx'][bad[0]]}, want {want[bad[0]]}"
    assert not np.array_equal(h["midx"], before["midx"])
    R.check(h, xyzr)
    assert got["q_ref"] * P.DEFAULT_RATIO < P.quality(loose, n_pool)[1]


def test_every_third_update_checks(mrt):
    sc = scene(mrt, "small")
    xyzr = R.xyzr_of(sc)
    with state(mrt, "small", sc) as st:
        st.set_auto_regroup(True, check_every=3)
        seen = []
        for _ in range(7):
            st.update_spheres(0, xyzr)
            seen.append(st.read_regroup_stats()["checks"])
        st.update_spheres(0, xyzr[:0])                                  # an empty update is not counted
        st.update_spheres(0, xyzr)
        st.update_spheres(0, xyzr)
        seen.append(st.read_regroup_stats()["checks"])
        assert st.get_auto_regroup() == dict(enabled=True, ratio=P.DEFAULT_RATIO, check_every=3) and st.debug_check_context() is None
    assert seen == [0, 0, 1, 1, 1, 2, 2, 3]


def test_a_walk_is_predicted_step_by_step(mrt):
    """12 steps at ratio 1.05, mrt_regroup_spheres behind step 6: the reference machine, fed the previous read-back, predicts the
    device's state and whether member_index changes"""
    name = "small"
    sc = scene(mrt, name)
    fired = []
    with state(mrt, name, sc) as st:
        st.set_auto_regroup(True, ratio=P.WALK_RATIO, check_every=1)
        h, n_pool = st.debug_read_hierarchy(), st.debug_regroup_info()["n_pool"]
        real = G.real_slots(h)
        s = P.baseline(P.new_state(), *P.quality(h, n_pool), mark=True)
        assert_stats(st, s, "enabling")
        for i, xyzr in enumerate(P.walk_steps(R.xyzr_of(sc), P.WALK_STEPS, P.WALK_AMOUNT)):
            s, f = P.decide(s, *P.quality(h, n_pool), P.WALK_RATIO)
            st.update_spheres(0, xyzr)
            now = st.debug_read_hierarchy()
            want = G.regroup(h["midx"], real, n_pool, xyzr[:, :3]) if f else h["midx"]
            assert np.array_equal(now["midx"], want), f"step {i + 1} ({'fires' if f else 'does not fire'})"
            if f:
                s = P.baseline(s, *P.quality(now, n_pool))
            assert_stats(st, s, f"step {i + 1}")
            h = now
            fired.append(f)
            if i + 1 == P.WALK_MANUAL:
                st.regroup_spheres()
                h = st.debug_read_hierarchy()
                assert np.array_equal(h["midx"], G.regroup(now["midx"], real, n_pool, xyzr[:, :3]))
                s = P.baseline(s, *P.quality(h, n_pool), mark=True)
                assert_stats(st, s, "the manual regroup")
        R.check(h, xyzr)
        assert st.debug_check_context() is None
    print("fired at steps", [i + 1 for i, f in enumerate(fired) if f])
    assert any(fired) and not all(fired) and s["checks"] == P.WALK_STEPS and s["regroups"] == sum(fired)


@pytest.mark.parametrize("rng_mode", [0, 1], ids=["stream-rng", "counter-rng"])
def test_frames_are_the_oracles_while_the_gate_opens_between_frames_in_flight(mrt, oracle, rng_mode):
    """sixteen frames in flight, no sync; updates before frames 2, 4, 5 and 6 at check_every 1: the scatter, the scatter again
    (fires), the build's positions (judged tight: the regrouped bounds), those again (fires)"""
    name = "small"
    sc = scene(mrt, name)
    _, upd, sc_new = motion(mrt, sc, "scatter")
    sends = {2: upd, 4: upd, 5: R.xyzr_of(sc), 6: R.xyzr_of(sc)}
    per_frame = [sc] * 2 + [sc_new] * 3 + [sc] * 3
    with state(mrt, name, sc, rng_mode, block=4) as st:
        st.debug_set_frames_in_flight(16)
        st.set_auto_regroup(True, check_every=1)
        for f in range(8):
            if f in sends:
                st.update_spheres(0, sends[f])
            st.redraw()
        got, counters = st.read_framebuffer(), st.read_counters()
        stats = st.read_regroup_stats()
        assert st.frames_done == 8 and st.debug_check_context() is None
    assert (stats["checks"], stats["regroups"], stats["pending"]) == (4, 2, False)
    ref, ref_counters = oracle_frames(oracle, mrt, ("auto-regroup-ordering",), per_frame, rng_mode)
    assert_same(got, counters, ref, ref_counters, "the gate opening between frames in flight")


def test_every_rank_of_a_sharded_frame_decides_alike(mrt):
    name = "small"
    sc = scene(mrt, name)
    first, upd, _ = motion(mrt, sc, "scatter")
    out = []
    for rank in range(2):
        with state(mrt, name, sc, shard=(rank, 2)) as st:
            st.set_auto_regroup(True, check_every=1)
            st.update_spheres(first, upd)
            st.update_spheres(first, upd)
            st.redraw()
            out.append((st.read_regroup_stats(), st.debug_read_hierarchy()["midx"]))
            assert st.debug_check_context() is None
    assert out[0][0] == out[1][0] and out[0][0]["regroups"] == 1 and np.array_equal(out[0][1], out[1][1])


def test_off_by_default_and_refusals(mrt):
    sc = scene(mrt, "small")
    xyzr = R.xyzr_of(sc)
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=SEED) as st:
        assert st.get_auto_regroup() == DEFAULTS
        with pytest.raises(mrt.MrtError) as e:
            st.read_regroup_stats()
        assert e.value.status == MRT_ERR_NO_SCENE
        st.set_auto_regroup(True, ratio=2.0, check_every=1)             # without a scene: the setting alone
        st.set_auto_regroup(False)
        assert st.get_auto_regroup() == dict(enabled=False, ratio=2.0, check_every=1) and st.debug_check_context() is None
    with state(mrt, "small", sc) as st:
        # off by default: an update checks nothing and the state stays what mrt_set_world uploaded
        st.update_spheres(0, xyzr)
        st.regroup_spheres()
        untouched = st.read_regroup_stats()
        assert (untouched["checks"], untouched["regroups"], untouched["q_ref"], untouched["q_last"], untouched["pending"]) == (0, 0, 0.0, 0.0, True)
        # bad parameters: refused, the setting stays
        st.set_auto_regroup(True, ratio=2.5, check_every=1)
        for bad in (dict(ratio=0.5), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(check_every=0), dict(check_every=1025)):
            with pytest.raises(mrt.MrtError) as e:
                st.set_auto_regroup(True, **bad)
            assert e.value.status == MRT_ERR_INVALID_ARG, bad
        assert st.get_auto_regroup() == dict(enabled=True, ratio=2.5, check_every=1)
        # disabling stops the checks
        st.update_spheres(0, xyzr)
        assert st.read_regroup_stats()["checks"] == 1
        st.set_auto_regroup(False)
        st.update_spheres(0, xyzr)
        stopped = st.read_regroup_stats()
        assert stopped["checks"] == 1
        st.regroup_spheres()                                            # (off: no baseline is queued behind it either)
        assert st.read_regroup_stats() == stopped
        # the setting survives mrt_reset, mrt_set_camera and mrt_set_world; the counters restart with the scene
        st.set_auto_regroup(True)
        st.reset()
        st.set_camera(mrt.Camera(mode=1, lookfrom=(0.0, 3.0, 12.0), lookat=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), vfov_deg=40.0,
                                 defocus_angle_deg=0.0, focus_dist=10.0))
        st.set_world(sc)
        assert st.get_auto_regroup() == dict(enabled=True, ratio=2.5, check_every=1)
        fresh = st.read_regroup_stats()
        assert (fresh["checks"], fresh["regroups"], fresh["pending"]) == (0, 0, True)
        built = P.quality(st.debug_read_hierarchy(), st.debug_regroup_info()["n_pool"])[1]
        st.update_spheres(0, xyzr)                                      # the first check of a scene set with the policy on: a baseline
        first = st.read_regroup_stats()
        assert (first["checks"], first["regroups"], first["pending"]) == (1, 0, False)
        assert first["q_ref"] == first["q_last"] == built > 0.0
        assert st.debug_check_context() is None
    # a pool of one cluster (and a ground): MRT_OK, never checked, all zeros
    few = sc[-5:]
    with state(mrt, "small", few) as st:
        assert st.debug_regroup_info()["n_pool"] == 1
        st.set_auto_regroup(True, check_every=1)
        st.update_spheres(0, R.xyzr_of(few))
        st.regroup_spheres()
        assert st.read_regroup_stats() == dict(checks=0, regroups=0, q_ref=0.0, q_last=0.0, q_level=[], levels=0, pending=False)
        R.check(st.debug_read_hierarchy(), R.xyzr_of(few))
        assert st.debug_check_context() is None
