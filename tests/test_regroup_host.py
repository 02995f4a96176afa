"""tests/regroup_ref.py -- the ordering mrt_regroup_spheres reproduces on the device -- held to its properties on the host
builder's hierarchies (no GPU): it permutes the pool over the pool's real slots and nothing else, its splits are aligned to
power-of-two blocks of clusters, ties are stable and -0.0 sorts before +0.0; three references broken on purpose are rejected by
the same checks; and on the moved stress scene it undoes what a kept grouping loses (sum R^2 per level)."""
import ctypes as C
import functools

import numpy as np
import pytest

import refit_ref as R
import regroup_ref as G
from myraytracer_amd import _lib
from test_hierarchy_host import scenes
from test_refit_host import host_hierarchy


def n_pool_of(mrt, sc, max_levels=4, top_target=0):
    sc = np.ascontiguousarray(sc, mrt.SPHERE_DTYPE)
    out = C.c_uint32()
    assert _lib.load().mrt_debug_pool_clusters(sc.ctypes.data, len(sc), max_levels, top_target, C.byref(out)) == 0
    return out.value


def random_scene(mrt, n, seed, big=0, snap=None):
    """n spheres of radius 0.1 .. 0.3 in a flat box, the last `big` of them far larger (radius 40 ..): direct / alone spheres"""
    rng = np.random.default_rng(seed)
    sc = np.zeros(n, mrt.SPHERE_DTYPE)
    c = rng.uniform(-6, 6, (n, 3)) * [1.0, 0.2, 1.0]
    if snap:                                    # few distinct coordinates, both zeros among them
        c = np.round(c / snap) * snap
        c[rng.random((n, 3)) < 0.1] = -0.0
        c[rng.random((n, 3)) < 0.1] = 0.0
    sc["center"] = c.astype(np.float32)
    sc["radius"] = rng.uniform(0.1, 0.3, n)
    sc["material_ty"] = 1
    for q in range(big):
        sc["center"][n - 1 - q] = (30.0 * q, -60.0 - 10.0 * q, 5.0 * q)
        sc["radius"][n - 1 - q] = 40.0 + q
    return sc


@functools.lru_cache(maxsize=None)
def _case(name):
    import myraytracer_amd as mrt
    levels, target = 4, 0
    if name == "ragged":
        sc = random_scene(mrt, 203, 1)
    elif name == "alone":
        sc = random_scene(mrt, 307, 2, big=7)
    elif name == "ties":
        sc = random_scene(mrt, 260, 3, snap=1.5)
    elif name == "three-levels":
        sc, levels, target = random_scene(mrt, 1101, 4, big=1), 4, 32
    elif name.startswith("pool-"):
        sc = random_scene(mrt, int(name[5:]), 5)
    else:
        sc = dict(scenes(mrt))[name]
    h = host_hierarchy(mrt, sc, levels, target)
    return sc, h, G.real_slots(h), n_pool_of(mrt, sc, levels, target)


CASES = ["ragged", "alone", "ties", "three-levels", "random 2300", "stress 40x40", "cover", "pool-4", "pool-8", "pool-12", "pool-20", "pool-32"]


def regrouped(name, variant="", xyz=None, midx=None):
    sc, h, real, n_pool = _case(name)
    xyz = R.xyzr_of(sc)[:, :3] if xyz is None else xyz
    return G.regroup(h["midx"] if midx is None else midx, real, n_pool, xyz, variant)


# ---- the properties, each a function of the ordering under test (the broken references go through the same ones) ----

def holds_permutation(variant=""):
    for name in CASES:
        sc, h, real, n_pool = _case(name)
        out = regrouped(name, variant)
        G.check_permutation(h["midx"], out, real, n_pool)
        assert np.array_equal(regrouped(name, variant, midx=out), out), f"{name}: not idempotent"
        if n_pool <= 1:                         # (a pool of one cluster is left as it is: nothing is queued for it)
            continue
        # the pool's spheres dealt over their slots in another order: the same result
        rng = np.random.default_rng(11)
        pref, rp = G.pool_layout(real, n_pool)
        mask = np.zeros(len(real), bool)
        mask[:4 * n_pool] = rp.ravel()
        dealt = h["midx"].copy()
        dealt[mask] = rng.permutation(dealt[mask])
        assert np.array_equal(regrouped(name, variant, midx=dealt), out), f"{name}: depends on the incoming slot order"


def holds_alignment(variant=""):
    total = 0
    for name in CASES:
        sc, h, real, n_pool = _case(name)
        total += G.check_alignment(regrouped(name, variant), real, n_pool, R.xyzr_of(sc)[:, :3])
    assert total > 1000


def handmade(xyz, variant=""):
    """len(xyz) / 4 full clusters holding the spheres in index order"""
    n = len(xyz)
    return G.regroup(np.arange(n, dtype=np.uint32), np.ones(n, bool), n // 4, np.asarray(xyz, np.float32), variant).reshape(-1, 4).tolist()


def holds_ties(variant=""):
    # depth 0 sorts 16 spheres by x (extent 15) into 15, 14, .. 0; depth 1 sorts the left half -- 15 .. 8 in that order -- by y,
    # where six of them tie at 0: the order depth 0 left decides who shares a cluster
    xyz = np.zeros((16, 3), np.float32)
    xyz[:, 0] = 15 - np.arange(16)
    xyz[[9, 8], 1] = 10.0
    xyz[[0, 1], 1] = 10.0
    assert handmade(xyz, variant) == [[12, 13, 14, 15], [8, 9, 10, 11], [4, 5, 6, 7], [0, 1, 2, 3]]
    # both zeros: spheres 4 .. 7 at -0.0 come before 0 .. 3 at +0.0, on the first axis (every extent is 0)
    xyz = np.zeros((8, 3), np.float32)
    xyz[4:, 0] = -0.0
    assert handmade(xyz, variant) == [[4, 5, 6, 7], [0, 1, 2, 3]]
    # equal keys keep the ascending order the pool starts in
    assert handmade(np.zeros((12, 3), np.float32), variant) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]


def test_the_reference_permutes_the_pool_over_its_real_slots_and_nothing_else():
    holds_permutation()


def test_every_split_is_aligned_to_its_block_of_clusters():
    holds_alignment()


def test_ties_are_stable_and_minus_zero_sorts_first():
    holds_ties()
    sc, h, real, n_pool = _case("ties")
    c = R.xyzr_of(sc)[:, :3]
    bits = c.view(np.uint32)
    assert (bits == 0x80000000).sum() > 20 and (bits == 0).sum() > 20 and len(np.unique(c[:, 0])) < 12


def test_the_depth_by_depth_composite_key_sort_is_the_recursion():
    """what regroup.hip computes: every depth's segments by one sort on (segment, key, rank)"""
    for name in CASES:
        sc, h, real, n_pool = _case(name)
        assert np.array_equal(G.regroup_by_depths(h["midx"], real, n_pool, R.xyzr_of(sc)[:, :3]), regrouped(name)), name


def test_the_slot_patterns_the_builder_makes(mrt):
    sc, h, real, n_pool = _case("ragged")
    pref, rp = G.pool_layout(real, n_pool)
    assert rp.sum(1).min() < 4 and rp.sum(1).min() >= 1, "the ragged scene has no short cluster"
    for k in range(n_pool):                     # a cluster's real slots are its first ones
        assert rp[k, :rp[k].sum()].all()
    sc, h, real, n_pool = _case("alone")
    assert h["n_direct"] == 4 and real[4 * n_pool:h["direct_first"]].reshape(-1, 4).sum(1).tolist()[:3] == [1, 1, 1]
    assert sorted(h["midx"][4 * n_pool:4 * n_pool + 12:4].tolist() + h["midx"][h["direct_first"]:h["direct_first"] + 4].tolist()) == list(range(300, 307))
    assert [_case(f"pool-{n}")[3] for n in (4, 8, 12, 20, 32)] == [1, 2, 3, 5, 8]
    sc, h, real, n_pool = _case("pool-4")
    assert np.array_equal(regrouped("pool-4"), h["midx"])                       # one cluster: nothing to do
    assert n_pool_of(mrt, np.zeros(0, mrt.SPHERE_DTYPE)) == 0


def test_pool_clusters_agrees_with_the_builders_layout():
    """clusters [0, n_pool) hold exactly the spheres of at most 8 x the median radius; the others sit alone behind them or direct"""
    for name in CASES:
        sc, h, real, n_pool = _case(name)
        r = np.abs(R.xyzr_of(sc)[:, 3].astype(np.float64))
        big = 8.0 * np.sort(r)[len(r) // 2] if len(r) > 1 else 1e300
        pref, rp = G.pool_layout(real, n_pool)
        pooled = h["midx"][:4 * n_pool][rp.ravel()]
        assert sorted(pooled.tolist()) == np.nonzero(r <= big)[0].tolist(), name
        n_hier = h["direct_first"] if h["n_direct"] else h["n_members"]
        rest = real[4 * n_pool:n_hier].reshape(-1, 4)
        assert (rest.sum(1) <= 1).all() and rest[:, 1:].sum() == 0, name


def test_the_regrouped_hierarchy_passes_the_refit_checker():
    for name in ("ragged", "alone", "three-levels", "random 2300"):
        sc, h, real, n_pool = _case(name)
        xyzr = R.xyzr_of(sc)
        out = regrouped(name)
        assert not np.array_equal(out, h["midx"]), name
        h2 = G.with_members(h, out, xyzr)
        R.check_members(h2, xyzr)
        R.check_bounds(h2, xyzr)
        stale = {**h2, "top": h["top"], "nodes": h["nodes"]}                    # (the old bounds do not fit the new grouping)
        with pytest.raises(AssertionError):
            R.check(stale, xyzr)


@pytest.mark.parametrize("variant", ["float", "median", "index"])
def test_a_reference_broken_on_purpose_is_rejected(variant):
    rejected = []
    for prop in (holds_permutation, holds_alignment, holds_ties):
        try:
            prop(variant)
        except AssertionError:
            rejected.append(prop.__name__)
    assert rejected, f"no property rejects the reference broken by '{variant}'"
    want = {"float": "holds_ties", "median": "holds_alignment", "index": "holds_ties"}[variant]
    assert want in rejected, (variant, rejected)


# ---- quality on the moved stress scene ----

@functools.lru_cache(maxsize=None)
def _stress_walk():
    """DESIGN.md 7e's walk (scripts/animation_rates.py): every sphere but the ground, 0.0005 x the scene's size a step"""
    import myraytracer_amd as mrt
    sc = mrt.scene_stress(1, 100)[0]
    xyzr = R.xyzr_of(sc)
    size = float(np.ptp(xyzr[:-1, :3], axis=0).max())
    rng = np.random.default_rng(1)
    at = {}
    for step in range(1, 801):
        xyzr = xyzr.copy()
        xyzr[:-1, :3] += (rng.normal(size=(len(xyzr) - 1, 3)) * 0.0005 * size).astype(np.float32)
        if step in (200, 800):
            at[step] = xyzr
    h = host_hierarchy(mrt, sc)
    return sc, h, G.real_slots(h), n_pool_of(mrt, sc), at


# level 1, regrouped / rebuilt, measured with this reference on mrt_scene_stress(1, 100): 1.364 after 200 steps, 1.339 after 800
# (the builder's exhaustive 4 + rest cut and its refinement passes are worth that; a jittered-grid stand-in with spheres of one
# size had given 1.12 .. 1.17); the bound is the larger + 10 %
LEVEL1_BOUND = 1.364 * 1.10


@pytest.mark.parametrize("steps", [200, 800])
def test_regrouping_the_moved_stress_scene_undoes_the_decay(mrt, steps):
    sc, h, real, n_pool, at = _stress_walk()
    xyzr = at[steps]
    n_hier = h["direct_first"] if h["n_direct"] else h["n_members"]
    assert h["levels"] >= 3 and n_pool > 2048
    kept = G.sum_r2(h["midx"], real, n_hier, h["levels"], xyzr)
    new = G.sum_r2(G.regroup(h["midx"], real, n_pool, xyzr[:, :3]), real, n_hier, h["levels"], xyzr)
    moved = sc.copy()
    moved["center"] = xyzr[:, :3]
    hb = host_hierarchy(mrt, moved)
    assert hb["levels"] == h["levels"]
    built = G.sum_r2(hb["midx"], G.real_slots(hb), hb["direct_first"] if hb["n_direct"] else hb["n_members"], hb["levels"], xyzr)
    print(f"{steps} steps: sum R^2 by level  kept {kept}  regrouped {new}  rebuilt {built}  level-1 ratio {new[0] / built[0]:.4f}")
    for k in range(h["levels"]):
        assert new[k] <= kept[k], (k + 1, new[k], kept[k])
        if k >= 1:
            assert new[k] <= built[k], (k + 1, new[k], built[k])
    assert new[0] <= LEVEL1_BOUND * built[0], (new[0] / built[0], LEVEL1_BOUND)
