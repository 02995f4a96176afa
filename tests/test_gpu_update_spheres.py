"""mrt_update_spheres on the GPU (include/myraytracer_amd.h, "scene"): new centres and radii with the hierarchy's grouping kept,
everything derived from them refitted by refit.hip in stream order.

Every update is held to two things: the refitted hierarchy, read back with mrt_debug_read_hierarchy, passes the float64
checker of tests/refit_ref.py against the UPDATED sphere list (tests/test_refit_host.py shows what that checker accepts and
rejects); and the frames rendered afterwards equal the oracle rendering the updated list, on uint32 views, with the samples /
world_hit_calls / rng_draws counters.  Images are 20 x 12, 2 spp, depth 8 -- ragged tiles, two bands -- in both RNG modes.

Layouts (the last sphere is a radius-1000 ground, which the builder keeps out of the hierarchy as a direct sphere):
  small      201 spheres: one level, two tiles of top records, the sweep space the builder chooses for a flat scene
  large-quad 1,100 spheres of one radius, hierarchy forced to (4, 32): three levels, boxes with the quadratic slack
  large-lin  the same with one sphere of radius 1e-4: the linear slack
  boxes-4200 4,200 spheres: the depth rule's own hierarchy, boxes in use by default
  deep-4200  (the hash test only) the same spheres forced to (4, 8): four levels of 1,050, 263, 66 and 17 nodes, the one layout in
             which the refit's 64-lane kernel takes several member slots a lane"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import refit_ref as R
from common import mismatch_report, oracle_render, to_oracle_spheres
from denoise_ref import expected_guides
from myraytracer_amd import _lib
from test_gpu_superset import _rays_for
from test_refit_host import host_hierarchy

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
from record_hierarchy_hashes import FIXTURE, device_hashes  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, SEED = 20, 12, 2, 8, 7
KEYS = ("samples", "world_hit_calls", "rng_draws")
MRT_ERR_INVALID_ARG, MRT_ERR_NO_SCENE, MRT_ERR_BAD_SCENE = 1, 4, 5
LAYOUTS = {"small": (201, None), "large-quad": (1100, (4, 32)), "large-lin": (1100, (4, 32)), "boxes-4200": (4200, None)}
MOTIONS = ("jitter", "scatter", "radii", "partial", "ground", "around-camera")
# tests/golden/hierarchy_hashes.json, "device": layout -> (its scene, the forced hierarchy); the cases as (layout, motion)
HASH_LAYOUTS = {"small": ("small", None), "large-quad": ("large-quad", (4, 32)), "large-lin": ("large-lin", (4, 32)), "deep-4200": ("boxes-4200", (4, 8))}
HASH_CASES = [(name, which) for name in HASH_LAYOUTS for which in ("jitter", "radii", "ground")] + [("large-quad", "scatter+regroup")]


def camera(mrt):
    return mrt.Camera(mode=1, lookfrom=(0.0, 2.5, 13.0), lookat=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), vfov_deg=40.0,
                      defocus_angle_deg=0.0, focus_dist=10.0)


_scenes = {}


def scene(mrt, name):
    if name not in _scenes:
        n, _ = LAYOUTS[name]
        rng = np.random.default_rng(n + len(name))
        sc = np.zeros(n, mrt.SPHERE_DTYPE)
        # (the small layout is flat enough for the builder to choose a scaled sweep space: an update has a space to leave)
        sc["center"][:n - 1] = (rng.uniform(-8, 8, (n - 1, 3)) * [1.0, 0.05 if name == "small" else 0.15, 1.0]).astype(np.float32)
        sc["radius"][:n - 1] = rng.uniform(0.2, 0.5, n - 1) if name == "small" else rng.uniform(0.03, 0.2, n - 1) if name == "boxes-4200" else 0.2
        if name == "large-lin":
            sc["radius"][500] = 1e-4
        sc["material_ty"] = 1 + np.arange(n) % 3                     # lambertian, metal, dielectric
        sc["albedo"] = rng.uniform(0.2, 0.9, (n, 3)).astype(np.float32)
        sc["param"] = np.where(sc["material_ty"] == 3, 1.5, 0.1).astype(np.float32)
        sc["center"][n - 1] = (0.0, -1002.0, 0.0)
        sc["radius"][n - 1] = 1000.0
        sc["material_ty"][n - 1] = 1
        _scenes[name] = sc
    return _scenes[name].copy()


def motion(mrt, sc, which):
    """-> (first, the (count, 4) update, the updated scene)"""
    rng = np.random.default_rng(MOTIONS.index(which) + 100)
    n = len(sc)
    xyzr = R.xyzr_of(sc)
    c = xyzr[:n - 1, :3].astype(np.float64)
    lo, hi = c.min(0), c.max(0)
    size = float((hi - lo).max())
    new, first, count = xyzr.copy(), 0, n
    if which == "jitter":                      # 1 % of the scene's size, the ground included
        new[:, :3] += rng.uniform(-0.01, 0.01, (n, 3)).astype(np.float32) * np.float32(size)
    elif which == "scatter":                   # anywhere in a box twice the scene's size: the groups stop meaning anything
        mid, half = 0.5 * (lo + hi), (hi - lo)
        new[:n - 1, :3] = rng.uniform(mid - half, mid + half, (n - 1, 3)).astype(np.float32)
        # (the ground's top goes anywhere in that box's lower half, so that the camera stays above it)
        top = rng.uniform(mid - half, mid + half * [1.0, 0.0, 1.0])
        new[n - 1, :3] = (top - [0.0, 1000.0, 0.0]).astype(np.float32)
    elif which == "radii":                     # x 3, x 0.1 (below the build's smallest radius), one sign flip on a glass sphere
        third = (n - 1) // 3
        new[:third, 3] *= np.float32(3.0)
        new[third:2 * third, 3] *= np.float32(0.1)
        assert np.abs(new[third:2 * third, 3]).min() < np.abs(xyzr[:n - 1, 3]).min()
        flip = 2 * third + [i for i in range(3) if sc["material_ty"][2 * third + i] == 3][0]
        new[flip, 3] = -new[flip, 3]
    elif which == "partial":
        first, count = 37, 100
        new[37:137, :3] += rng.uniform(-0.1, 0.1, (100, 3)).astype(np.float32) * np.float32(size)
    elif which == "ground":
        first, count = n - 1, 1
        new[n - 1, :3] += np.array([3.0, -2.0, 1.0], np.float32)
        new[n - 1, 3] = 1001.0
    else:                                      # a glass sphere placed around the camera
        first, count = 5, 1
        assert sc["material_ty"][5] == 3
        new[5] = (0.0, 2.5, 13.0, 0.75)
    out = sc.copy()
    out["center"], out["radius"] = new[:, :3], new[:, 3]
    return first, new[first:first + count].copy(), out


def state(mrt, name, sc, rng_mode=0, **kw):
    st = mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=SEED, **kw)
    if LAYOUTS[name][1]:
        st.debug_set_hierarchy(*LAYOUTS[name][1])
    st.debug_set_boxes(2)                      # the walk's box tests on (large scenes)
    st.set_world(sc)
    st.set_camera(camera(mrt))
    if rng_mode:
        st.set_rng_mode(rng_mode)
    return st


def refitted_hierarchy(mrt, name, which):
    """mrt_debug_read_hierarchy after the motion `which` of the hash layout `name` ("+regroup": and mrt_regroup_spheres)"""
    base, forced = HASH_LAYOUTS[name]
    sc = scene(mrt, base)
    first, upd, sc_new = motion(mrt, sc, which.split("+")[0])
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=SEED) as st:
        if forced:
            st.debug_set_hierarchy(*forced)
        st.set_world(sc)
        st.update_spheres(first, upd)
        if which.endswith("+regroup"):
            st.regroup_spheres()
        h = st.debug_read_hierarchy()
    if name == "deep-4200":
        assert h["levels"] == 4
        R.check(h, R.xyzr_of(sc_new))
    return h


_oracle_cache = {}


def oracle_frames(oracle, mrt, key, scenes_per_frame, rng_mode):
    """the oracle's accumulation over len(scenes_per_frame) frames, frame f rendering scenes_per_frame[f]; (image, counters)"""
    key = (key, rng_mode)
    if key not in _oracle_cache:
        cnt = oracle.Counters()
        cam = oracle.lookat_camera((0.0, 2.5, 13.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 0.0, 10.0)
        seeds = oracle.fill_seeds(SEED, W, H)
        fb = np.zeros((H, W, 4), np.float32)
        for f, sc in enumerate(scenes_per_frame):
            packed = oracle.pack_world(to_oracle_spheres(oracle, sc))
            fb = oracle.render_frame(W, H, SPP, DEPTH, packed, cam, seeds, oracle.frame_shuffle(SEED, f), oracle.frame_weight(f, 1.0),
                                     fb, counters=cnt, rng_mode=rng_mode)
        _oracle_cache[key] = (fb, {k: cnt.as_dict()[k] for k in KEYS})
    return _oracle_cache[key]


def assert_same(got, counters, ref, ref_counters, what):
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{what}: " + mismatch_report(got, ref)
    assert {k: counters[k] for k in KEYS} == {k: ref_counters[k] for k in KEYS}, what


def test_the_read_back_is_the_host_builders_arrays_bit_for_bit(mrt):
    """before any update: what mrt_debug_read_hierarchy reads is what mrt_set_world uploaded (this tests the read-back itself)"""
    L = _lib.load()
    for name in LAYOUTS:
        sc = scene(mrt, name)
        levels, target = LAYOUTS[name][1] or (4, 0)
        want = host_hierarchy(mrt, sc, levels, target)
        with state(mrt, name, sc) as st:
            h = st.debug_read_hierarchy()
        for k in ("levels", "n_members", "n_direct", "direct_first"):
            assert h[k] == want[k], (name, k)
        assert h["level_base"][:h["levels"]] == want["level_base"][:h["levels"]]
        for k in ("top", "nodes", "midx"):
            assert np.array_equal(h[k].view(np.uint32), want[k].view(np.uint32)), (name, k)
        axis, org, reach = (C.c_float * 3)(), (C.c_float * 3)(), C.c_double()
        mf = np.zeros(len(want["mfma"]), np.uint16)
        if want["levels"] == 1:                # the sweep's space is the builder's choice: mrt_debug_build_sweep restates it
            assert L.mrt_debug_build_sweep(sc.ctypes.data, len(sc), None, axis, None, 0, mf.ctypes.data, len(mf), org, C.byref(reach)) == 0
            assert h["axes"] == tuple(axis) and h["reach"] == reach.value
            if name == "small":
                assert h["axes"] != (1.0, 1.0, 1.0)          # a flat scene: the case in which an update has a space to leave
        else:
            mf = want["mfma"]
            assert h["axes"] == (1.0, 1.0, 1.0)
        assert np.array_equal(h["mfma"], mf), name
        assert np.array_equal(h["origin"], want["origin"])
        if h["n_members"] > 1024:
            assert h["box_quad"] == want["box_quad"] == (name != "large-lin") and h["box_kc"] == want["box_kc"], name
            for k in ("boxes", "boxes_open"):
                assert np.array_equal(h[k].view(np.uint32), want[k].view(np.uint32)), (name, k)
        else:
            assert len(h["boxes"]) == 0
        assert h["n_direct"] == 1 and h["direct_index"][0] == len(sc) - 1
        if h["axes"] != (1.0, 1.0, 1.0):       # (the checker's operand and reach are statements about D = I)
            del h["mfma"], h["reach"]
        R.check(h, R.xyzr_of(sc))


@pytest.mark.parametrize("rng_mode", [0, 1], ids=["stream-rng", "counter-rng"])
@pytest.mark.parametrize("which", MOTIONS)
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_a_motion_refits_the_hierarchy_and_renders_the_updated_scene(mrt, oracle, name, which, rng_mode):
    sc = scene(mrt, name)
    first, upd, sc_new = motion(mrt, sc, which)
    with state(mrt, name, sc, rng_mode) as st:
        before = st.debug_read_hierarchy()
        st.update_spheres(first, upd)
        h = st.debug_read_hierarchy()
        R.check(h, R.xyzr_of(sc_new))                                   # the checker first
        assert h["axes"] == (1.0, 1.0, 1.0) and np.array_equal(h["origin"], before["origin"])
        assert np.array_equal(h["midx"], before["midx"]) and h["box_quad"] == before["box_quad"] and h["box_kc"] >= before["box_kc"]
        assert np.array_equal(h["shade"][:, 4:], before["shade"][:, 4:]) and np.array_equal(h["centres"][:, 3], before["centres"][:, 3])
        st.render(1)
        st.sync()
        got, counters = st.read_framebuffer(), st.read_counters()
    ref, ref_counters = oracle_frames(oracle, mrt, (name, which), [sc_new], rng_mode)
    assert_same(got, counters, ref, ref_counters, f"{name}, {which}")   # the oracle second


@pytest.mark.parametrize("name,which", HASH_CASES, ids=[f"{n}-{w}" for n, w in HASH_CASES])
def test_the_refitted_arrays_hash_to_the_recorded_ones(mrt, name, which):
    """every array and scalar the device holds after the call, bit for bit, against the build the fixture was recorded from
    (scripts/record_hierarchy_hashes.py): a change that means to leave the refit's arithmetic alone did.  deep-4200 also passes
    the float64 checker."""
    want = json.load(open(FIXTURE))["device"]["hashes"][f"{name}|{which}"]
    got = device_hashes(refitted_hierarchy(mrt, name, which))
    assert got.keys() == want.keys()
    differ = sorted(k for k in got if got[k] != want[k])
    assert not differ, f"{name}, {which}: {differ} differ from the recorded build"


@pytest.mark.parametrize("sweep", [1, 2], ids=["valu-sweep", "matrix-core-sweep"])
@pytest.mark.parametrize("which", ["scatter", "radii"])
@pytest.mark.parametrize("name", ["small", "large-quad"])
def test_candidate_sets_after_an_update(mrt, oracle, name, which, sweep):
    """tests/test_gpu_superset.py's claim for the refitted hierarchy: over 4,096 rays the spheres that reach the root tests contain
    every sphere with a discriminant >= 0 that is not entirely behind the origin, and hold no sphere with a negative one"""
    sc = scene(mrt, name)
    first, upd, sc_new = motion(mrt, sc, which)
    rays = _rays_for(np.random.default_rng(3), sc_new, 2048, 1536, 512)[:4096]
    a2 = (rays[:, 3:].astype(np.float64) ** 2).sum(1)
    rays = rays[np.abs(a2 - 1.0) < 5e-6]
    packed = oracle.pack_world(to_oracle_spheres(oracle, sc_new))
    ref_hit, ref_t, ref_set, required = oracle.world_hit_batch(packed, rays)
    with state(mrt, name, sc) as st:
        st.update_spheres(first, upd)
        st.debug_set_sweep(sweep)
        assert st.debug_sweep_variant() == sweep
        hit, t, cand = st.debug_world_hit(rays, len(sc))
    assert required.sum() > len(rays)
    assert not (required & ~cand).any(), f"{int((required & ~cand).sum())} (ray, sphere) pairs with a discriminant >= 0 never reached the root tests"
    assert not (cand & ~ref_set).any()
    assert np.array_equal(hit, ref_hit) and np.array_equal(t.view(np.uint32)[hit >= 0], ref_t.view(np.uint32)[hit >= 0])


@pytest.mark.parametrize("name", ["small", "large-lin"])
def test_an_update_of_every_sphere_equals_set_world(mrt, name):
    sc = scene(mrt, name)
    _, upd, sc_new = motion(mrt, sc, "scatter")
    with state(mrt, name, sc) as st:
        st.update_spheres(0, upd)
        st.render(2)
        a, ca = st.read_framebuffer(), st.read_counters()
    with state(mrt, name, sc_new) as st:
        st.render(2)
        b, cb = st.read_framebuffer(), st.read_counters()
    assert_same(a, ca, b, cb, name)


@pytest.mark.parametrize("rng_mode", [0, 1], ids=["stream-rng", "counter-rng"])
@pytest.mark.parametrize("every_frame", [False, True], ids=["four-then-four", "an-update-before-every-frame"])
def test_ordering_against_frames_in_flight(mrt, oracle, every_frame, rng_mode):
    """sixteen frames in flight pinned, no sync between the calls: frames queued before an update render the old geometry, frames
    queued after it the new one -- the accumulation is the oracle's blend of the frames' own scenes"""
    name = "small"
    sc = scene(mrt, name)
    rng = np.random.default_rng(9)
    per_frame, updates, cur = [], [], sc
    for f in range(8):
        if (every_frame or f == 4):
            new = R.xyzr_of(cur)
            new[:, :3] += rng.uniform(-0.4, 0.4, (len(sc), 3)).astype(np.float32)
            new[-1, :3] = R.xyzr_of(sc)[-1, :3] + rng.uniform(-0.2, 0.2, 3).astype(np.float32)
            cur = cur.copy()
            cur["center"] = new[:, :3]
            updates.append((f, new))
        per_frame.append(cur)
    with state(mrt, name, sc, rng_mode) as st:
        st.debug_set_frames_in_flight(16)
        pending = dict(updates)
        for f in range(8):
            if f in pending:
                st.update_spheres(0, pending[f])
            st.redraw()
        got, counters = st.read_framebuffer(), st.read_counters()
        assert st.frames_done == 8
    ref, ref_counters = oracle_frames(oracle, mrt, ("ordering", every_frame), per_frame, rng_mode)
    assert_same(got, counters, ref, ref_counters, "ordering")


def test_guides_are_rebuilt_for_the_updated_scene(mrt, oracle):
    name = "small"
    sc = scene(mrt, name)
    first, upd, sc_new = motion(mrt, sc, "scatter")
    with state(mrt, name, sc) as st:
        g0 = st.debug_read_guides()
        st.update_spheres(first, upd)
        g = st.debug_read_guides()
    hit, t, normal, albedo = expected_guides(oracle, sc_new, g["rays"])
    assert not np.array_equal(g0["index"], g["index"]) and (hit >= 0).any() and (hit < 0).any()
    assert np.array_equal(g["index"].ravel(), hit)
    assert np.array_equal(np.ascontiguousarray(g["t"]).view(np.uint32).ravel(), t.view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(g["normal"]).view(np.uint32).reshape(-1, 3), normal.view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(g["albedo"]).view(np.uint32).reshape(-1, 3), albedo.view(np.uint32))


def test_every_refusal_leaves_the_context_untouched(mrt):
    name = "large-quad"
    sc = scene(mrt, name)
    n = len(sc)
    ok = R.xyzr_of(sc)[:4].copy()
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=SEED) as st:
        with pytest.raises(mrt.MrtError) as e:
            st.update_spheres(0, ok)
        assert e.value.status == MRT_ERR_NO_SCENE
    with state(mrt, name, sc) as st:
        st.render(2)
        img, cnt, h0 = st.read_framebuffer(), st.read_counters(), st.debug_read_hierarchy()
        L, ctx = st._L, st._ctx
        bad = []
        for v in (np.nan, np.inf, -np.inf, 1.5e7, -1.5e7):
            for col in (0, 3):
                x = ok.copy()
                x[2, col] = v
                bad.append(x)
        cases = [(n - 3, ok, MRT_ERR_INVALID_ARG), (n, ok[:1], MRT_ERR_INVALID_ARG), (0xFFFFFFFF, ok[:2], MRT_ERR_INVALID_ARG)]
        cases += [(10, x, MRT_ERR_BAD_SCENE) for x in bad]
        for first, x, status in cases:
            with pytest.raises(mrt.MrtError) as e:
                st.update_spheres(first, x)
            assert e.value.status == status, (first, x)
        assert L.mrt_update_spheres(ctx, 0, 3, None) == MRT_ERR_INVALID_ARG
        assert L.mrt_update_spheres(ctx, n, 0, None) == 0 and L.mrt_update_spheres(ctx, n + 1, 0, None) == MRT_ERR_INVALID_ARG
        st.update_spheres(0, np.zeros((0, 4), np.float32))               # count == 0: MRT_OK, nothing queued
        h1 = st.debug_read_hierarchy()
        for k, v in h0.items():
            assert np.array_equal(v, h1[k]) if isinstance(v, np.ndarray) else v == h1[k], k
        assert np.array_equal(st.read_framebuffer().view(np.uint32), img.view(np.uint32)) and st.read_counters() == cnt
        assert st.frames_done == 2 and st.debug_check_context() is None


def test_a_pinned_schedule_and_the_accumulation_survive_an_update(mrt):
    name = "small"
    sc = scene(mrt, name)
    first, upd, _ = motion(mrt, sc, "jitter")
    with state(mrt, name, sc) as st:
        st.set_schedule_hint(4, 1)
        st.redraw()
        sch = st.get_schedule()
        assert (sch["div"], sch["mult"], sch["settled"]) == (4, 1, True)
        st.update_spheres(first, upd)
        assert st.get_schedule() == sch and st.frames_done == 1
        st.redraw()
        after = st.get_schedule()
        assert (after["div"], after["mult"], after["settled"], after["frames_in_flight"]) == (4, 1, True, sch["frames_in_flight"])
        assert st.frames_done == 2
