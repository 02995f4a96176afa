"""tests/regroup_policy_ref.py -- the quality figure and the state machine of mrt_set_auto_regroup that the device reproduces bit
for bit -- held to its definition on the host builder's hierarchies (no GPU): the figure against an independent math.fsum over
the same records, what it skips, when the machine fires; three references broken on purpose are rejected by the same checks; the
expectations tests/test_gpu_auto_regroup.py rests on (the scatter motion fires at the default ratio, unchanged positions do not,
its walk both fires and does not) are established here with the float64 refit of tests/regroup_ref.py; and the C ABI's host-only
part: the defaults, the parameter checks with ctx == NULL, the struct sizes, the export list."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import refit_ref as R
import regroup_policy_ref as P
import regroup_ref as G
from myraytracer_amd import _lib
from test_gpu_update_spheres import LAYOUTS, motion, scene
from test_refit_host import host_hierarchy
from test_regroup_host import _case, n_pool_of

MRT_OK, MRT_ERR_INVALID_ARG = 0, 1
CASES = ["ragged", "alone", "three-levels", "random 2300", "stress 40x40", "pool-8"]


def fsum_quality(h, n_pool):
    """the definition, independently: per level, math.fsum over the records that begin inside the pool and can be hit"""
    levels = []
    for k in range(1, h["levels"] + 1):
        recs = P.level_records(h, k)
        levels.append(math.fsum(-float(recs[j, 3]) for j in range(len(recs)) if j * 4 ** (k - 1) < n_pool and recs[j, 3] != np.inf))
    return levels, math.fsum(levels)


def with_a_never_hit_record(h, n_pool):
    """a copy of h whose second judged cluster record says "never hit" (the builder makes none inside the pool)"""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in h.items()}
    P.level_records(out, 1)[1] = (0.0, 0.0, 0.0, np.inf)
    return out


# ---- the properties, each a function of the reference under test (the broken ones go through the same) ----

def holds_definition(variant=""):
    for name in CASES:
        sc, h, real, n_pool = _case(name)
        levels, q = P.quality(h, n_pool, variant)
        want_levels, want = fsum_quality(h, n_pool)
        assert len(levels) == h["levels"] and want > 0.0
        for got, ref in zip(levels + [q], want_levels + [want]):
            assert abs(got - ref) <= 1e-12 * ref, (name, got, ref)


def holds_never_hit(variant=""):
    sc, h, real, n_pool = _case("ragged")
    bad = with_a_never_hit_record(h, n_pool)
    levels, q = P.quality(bad, n_pool, variant)
    want_levels, want = fsum_quality(bad, n_pool)
    assert math.isfinite(q) and abs(q - want) <= 1e-12 * want, (q, want)
    assert levels[0] < P.quality(h, n_pool, variant)[0][0]


def holds_pool_only(variant=""):
    for name in ("alone", "ragged"):
        sc, h, real, n_pool = _case(name)
        levels, q = P.quality(h, n_pool, variant)
        rec1 = P.level_records(h, 1)
        assert abs(levels[0] - math.fsum(-float(v) for v in rec1[:n_pool, 3])) <= 1e-12 * levels[0], name
        if name == "alone":                     # three huge spheres sit in clusters of their own behind the pool's
            behind = rec1[n_pool:, 3]
            assert np.isfinite(behind).sum() == 3 and levels[0] < 0.1 * math.fsum(-float(v) for v in behind[np.isfinite(behind)])


def run_machine(qs, ratio, variant="", regrouped=None):
    """checks with Q = qs[i] in turn; a check that fires is followed by a baseline at regrouped[i] -> (fired flags, states)"""
    s, fired, states = P.new_state(), [], []
    for i, q in enumerate(qs):
        s, f = P.decide(s, [q], q, ratio, variant)
        if f:
            s = P.baseline(s, [regrouped[i]], regrouped[i], variant=variant)
        else:
            assert P.baseline(s, [q], q, variant=variant) == s          # (not pending: the baseline kernel does nothing)
        fired.append(f)
        states.append(s)
    return fired, states


def holds_machine(variant=""):
    # the first check only takes a baseline, however large Q is
    fired, st = run_machine([100.0], 1.5, variant)
    assert fired == [False] and st[0]["q_ref"] == 100.0 and not st[0]["pending"] and (st[0]["checks"], st[0]["regroups"]) == (1, 0)
    # it fires exactly when Q > ratio * q_ref (ratio 1.5 is exact in float32); after firing the next baseline replaces q_ref
    qs = [100.0, 149.0, 150.0, 150.0000001, 160.0, 180.1, 100.0]
    fired, st = run_machine(qs, 1.5, variant, regrouped=[None, None, None, 120.0, None, 90.0, None])
    assert fired == [False, False, False, True, False, True, False], fired
    assert [s["q_ref"] for s in st] == [100.0, 100.0, 100.0, 120.0, 120.0, 90.0, 90.0]
    assert [s["q_last"] for s in st] == [100.0, 149.0, 150.0, 120.0, 160.0, 90.0, 100.0]
    assert st[-1]["checks"] == 7 and st[-1]["regroups"] == 2 and not st[-1]["pending"]
    # at ratio 1 an equal Q does not fire, the next larger double does
    fired, _ = run_machine([7.0, 7.0, 7.0, math.nextafter(7.0, 8.0)], 1.0, variant, regrouped=[None, None, None, 7.0])
    assert fired == [False, False, False, True]
    # the ratio is the float32 the ABI carries
    fired, _ = run_machine([1.0, 1.1], 1.1, variant, regrouped=[None, 1.0])
    assert fired == [False, float(np.float32(1.1)) < 1.1]
    # a regroup the caller asks for takes q_ref whether pending or not; a baseline without one does nothing unless pending
    s = P.decide(P.new_state(), [5.0], 5.0, 2.0, variant)[0]
    assert P.baseline(s, [3.0], 3.0, variant=variant) == s
    m = P.baseline(s, [3.0], 3.0, mark=True, variant=variant)
    assert (m["q_ref"], m["q_last"], m["pending"], m["checks"], m["regroups"]) == (3.0, 3.0, False, 1, 0)


PROPERTIES = (holds_definition, holds_never_hit, holds_pool_only, holds_machine)


def test_the_figure_is_the_definition_to_rounding():
    holds_definition()


def test_never_hit_records_add_nothing():
    holds_never_hit()


def test_nodes_beginning_behind_the_pool_add_nothing():
    holds_pool_only()


def test_the_state_machine():
    holds_machine()


def test_the_order_of_additions_is_the_stated_one():
    """lane partials of 256, then the lanes in order: on values chosen so that another order gives other bits"""
    n = 1000
    rng = np.random.default_rng(2)
    r2 = (rng.uniform(0.5, 2.0, n) * 10.0 ** rng.integers(-8, 9, n)).astype(np.float32)
    h = dict(levels=1, top=np.concatenate([np.zeros((n, 3), np.float32), -r2[:, None]], axis=1), nodes=np.zeros((0, 4), np.float32), level_base=[0, 0, 0, 0])
    levels, q = P.quality(h, n)
    lanes = []
    for l in range(256):
        s = 0.0
        for j in range(l, n, 256):
            s += float(r2[j])
        lanes.append(s)
    want = 0.0
    for s in lanes:
        want += s
    assert q == want == levels[0]
    plain = 0.0
    for v in r2:
        plain += float(v)
    assert plain != want                                                          # (so the order is observable here)
    assert abs(want - math.fsum(float(v) for v in r2)) <= 1e-12 * want
    assert P.quality(h, 600)[1] < want


@pytest.mark.parametrize("variant", P.BROKEN)
def test_a_reference_broken_on_purpose_is_rejected(variant):
    rejected = []
    for prop in PROPERTIES:
        try:
            prop(variant)
        except AssertionError:
            rejected.append(prop.__name__)
    want = {"never_hit": "holds_never_hit", "non_pool": "holds_pool_only", "stale_ref": "holds_machine"}[variant]
    assert want in rejected, (variant, rejected)
    if variant == "stale_ref":                  # it keeps the build's q_ref, so it fires at every check after the first
        fired, _ = run_machine([100.0, 151.0, 151.0, 151.0], 1.5, variant, regrouped=[None, 120.0, 120.0, 120.0])
        assert fired == [False, True, True, True]
        assert run_machine([100.0, 151.0, 151.0, 151.0], 1.5, regrouped=[None, 120.0, None, None])[0] == [False, True, False, False]


# ---- what tests/test_gpu_auto_regroup.py expects of its scenes, on the host's float64 refit ----

@functools.lru_cache(maxsize=None)
def _layout(name):
    import myraytracer_amd as mrt
    sc = scene(mrt, name)
    levels, target = LAYOUTS[name][1] or (4, 0)
    h = host_hierarchy(mrt, sc, levels, target)
    return sc, h, G.real_slots(h), n_pool_of(mrt, sc, levels, target)


@pytest.mark.parametrize("name", ["small", "large-quad", "boxes-4200"])
def test_the_scatter_motion_fires_at_the_default_ratio_and_unchanged_positions_do_not(mrt, name):
    sc, h, real, n_pool = _layout(name)
    _, _, sc_new = motion(mrt, sc, "scatter")
    q0 = P.quality(h, n_pool)[1]
    kept = G.with_members(h, h["midx"], R.xyzr_of(sc))                  # unchanged positions, refitted
    loose = G.with_members(h, h["midx"], R.xyzr_of(sc_new))
    q_same, q_loose = P.quality(kept, n_pool)[1], P.quality(loose, n_pool)[1]
    print(f"{name}: Q built {q0:.6g}, refitted unchanged {q_same:.6g} (x {q_same / q0:.4f}), after scatter {q_loose:.6g} (x {q_loose / q0:.2f})")
    s = P.baseline(P.new_state(), *P.quality(h, n_pool), mark=True)    # mrt_set_auto_regroup turning the policy on
    s, fired = P.decide(s, *P.quality(kept, n_pool), P.DEFAULT_RATIO)
    assert not fired and q_same <= 1.01 * q0                            # (far from the ratio: the refit's rounding cannot matter)
    s, fired = P.decide(s, *P.quality(loose, n_pool), P.DEFAULT_RATIO)
    assert fired and q_loose > 2.0 * P.DEFAULT_RATIO * q0
    # ... and the regroup it lets run brings the figure back under the ratio
    midx = G.regroup(h["midx"], real, n_pool, R.xyzr_of(sc_new)[:, :3])
    tight = G.with_members(h, midx, R.xyzr_of(sc_new))
    assert P.quality(tight, n_pool)[1] < q_loose / P.DEFAULT_RATIO
    # ... and the build's positions sent again find that grouping as loose as the scatter found the build's
    back = G.with_members(h, midx, R.xyzr_of(sc))
    assert P.quality(back, n_pool)[1] > 2.0 * P.DEFAULT_RATIO * P.quality(tight, n_pool)[1]


def test_the_walk_of_the_gpu_test_fires_at_some_checks_and_not_at_others(mrt):
    sc, h, real, n_pool = _layout("small")
    s = P.baseline(P.new_state(), *P.quality(h, n_pool), mark=True)
    midx, fired, ratios = h["midx"], [], []
    for i, xyzr in enumerate(P.walk_steps(R.xyzr_of(sc), P.WALK_STEPS, P.WALK_AMOUNT)):
        levels, q = P.quality(h, n_pool)                                # the bounds of the previous step
        ratios.append(q / s["q_ref"])
        s, f = P.decide(s, levels, q, P.WALK_RATIO)
        if f:
            midx = G.regroup(midx, real, n_pool, xyzr[:, :3])
        h = G.with_members(h, midx, xyzr)
        if f:
            s = P.baseline(s, *P.quality(h, n_pool))
        if i + 1 == P.WALK_MANUAL:
            midx = G.regroup(midx, real, n_pool, xyzr[:, :3])
            h = G.with_members(h, midx, xyzr)
            s = P.baseline(s, *P.quality(h, n_pool), mark=True)
        fired.append(f)
    print("Q / q_ref at each check: " + ", ".join(f"{r:.3f}{'*' if f else ''}" for r, f in zip(ratios, fired)))
    assert 2 <= sum(fired) <= P.WALK_STEPS - 3 and s["checks"] == P.WALK_STEPS and s["regroups"] == sum(fired)
    # no check sits on the threshold: the device's own refit decides the same way
    assert all(abs(r - P.WALK_RATIO) > 0.004 for r in ratios), ratios


# ---- the C ABI, host only ----

def test_defaults_parameter_checks_and_layout(mrt):
    L = _lib.load()
    assert C.sizeof(_lib.MrtAutoRegroup) == 32 and C.sizeof(_lib.MrtRegroupStats) == 72
    for name in ("mrt_auto_regroup_default", "mrt_set_auto_regroup", "mrt_get_auto_regroup", "mrt_read_regroup_stats"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/myraytracer_amd.h").read()
    for name in ("mrt_auto_regroup", "mrt_regroup_stats", "mrt_set_auto_regroup(", "mrt_read_regroup_stats("):
        assert name in hdr
    p = _lib.MrtAutoRegroup()
    L.mrt_auto_regroup_default(C.byref(p))
    assert (p.size, p.enabled, p.check_every, p.ratio, list(p.reserved)) == (32, 0, P.DEFAULT_CHECK_EVERY, P.DEFAULT_RATIO, [0, 0, 0, 0])
    L.mrt_auto_regroup_default(None)                                        # (tolerated, as its siblings tolerate it)
    assert L.mrt_set_auto_regroup(None, C.byref(p)) == MRT_OK               # ctx NULL: the setting alone
    assert L.mrt_set_auto_regroup(None, None) == MRT_ERR_INVALID_ARG
    assert L.mrt_get_auto_regroup(None, C.byref(p)) == MRT_ERR_INVALID_ARG
    assert L.mrt_read_regroup_stats(None, None) == MRT_ERR_INVALID_ARG

    def check(**kw):
        q = _lib.MrtAutoRegroup()
        L.mrt_auto_regroup_default(C.byref(q))
        for k, v in kw.items():
            if k == "reserved":
                q.reserved[v] = 1
            else:
                setattr(q, k, v)
        return L.mrt_set_auto_regroup(None, C.byref(q))
    for good in (dict(enabled=1), dict(check_every=1), dict(check_every=1024), dict(ratio=1.0), dict(ratio=1e6), dict(enabled=1, ratio=1.5, check_every=2)):
        assert check(**good) == MRT_OK, good
    for bad in (dict(size=28), dict(size=0), dict(enabled=2), dict(check_every=0), dict(check_every=1025), dict(ratio=0.999), dict(ratio=-3.0),
                dict(ratio=float("nan")), dict(ratio=float("inf")), dict(reserved=0), dict(reserved=3)):
        assert check(**bad) == MRT_ERR_INVALID_ARG, bad
