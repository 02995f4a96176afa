"""mrt_update_materials on the GPU (include/myraytracer_amd.h, "scene"): new materials with everything else kept.

Every image is at the shapes of tests/test_gpu_update_spheres.py -- 20 x 12, 2 spp, depth 8, seed 7: ragged tiles, two bands --
on its "small" (201 spheres, flat, a scaled sweep space) and "large-quad" (1,100 spheres, hierarchy forced to (4, 32), boxes on)
layouts; both end in a radius-1000 ground kept as a direct sphere and their material types cycle L / M / D.  Every comparison is
on uint32 views; none uses a tolerance.

The edits (EDITS, fixed seeds; edit() -> the scene to start from, the calls, the edited scene):
  recolour  every albedo and every fuzz
  types     every sphere's type rotated L -> M -> D -> L with fitting params, sphere 11 set to type 7 (absorbs; mrt_set_world
            refuses such a list, so the fresh context takes it through mrt_set_world_raw)
  ior       every Dielectric's ior, with one glass sphere's radius negative in the scene
  partial   first 37, count 100
  ground    the last sphere alone: a direct sphere, whose geometry the kernel keeps in its arguments
  batch+1   one sphere more than the scatter's batch of 192 rides in one launch
  2batches  exactly two batches (384 spheres: the large layout only)"""
import ctypes as C

import numpy as np
import pytest

from common import mismatch_report
from denoise_ref import expected_guides
from temporal_ref import index_bits, lum
from test_gpu_update_spheres import DEPTH, H, KEYS, LAYOUTS, SEED, SPP, W, assert_same, camera, motion, oracle_frames, scene

pytestmark = pytest.mark.gpu

MRT_ERR_INVALID_ARG, MRT_ERR_NO_SCENE = 1, 4
NAMES = ("small", "large-quad")
EDITS = ("recolour", "types", "ior", "partial", "ground", "batch+1", "2batches")
BATCH = 192                                    # mrt_internal.h, kMaterialBatch
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def rotate_types(sc, idx, rng):
    """L -> M -> D -> L for the spheres idx, with params that fit the new type"""
    ty = sc["material_ty"][idx]
    new = np.where(ty == 1, 2, np.where(ty == 2, 3, 1)).astype(np.int32)
    sc["material_ty"][idx] = new
    sc["param"][idx] = np.where(new == 2, rng.uniform(0.0, 0.5, len(idx)), np.where(new == 3, rng.uniform(1.3, 1.8, len(idx)), 0.0)).astype(F)


def edit(mrt, sc, which):
    """-> (the scene the context is given first, [(first, materials)], the edited scene)"""
    rng = np.random.default_rng(EDITS.index(which) + 300)
    n = len(sc)
    sc = sc.copy()
    first, count = 0, n
    if which == "ior":                          # hollow glass: the sign of the radius is geometry, the ior the material's
        glass = np.nonzero(sc["material_ty"][:n - 1] == 3)[0]
        sc["radius"][glass[7]] = -sc["radius"][glass[7]]
    out = sc.copy()
    if which == "recolour":
        out["albedo"] = rng.uniform(0.05, 0.95, (n, 3)).astype(F)
        out["param"] = np.where(out["material_ty"] == 2, rng.uniform(0.0, 0.6, n), out["param"]).astype(F)
    elif which == "types":
        rotate_types(out, np.arange(n), rng)
        out["albedo"] = rng.uniform(0.1, 0.9, (n, 3)).astype(F)
        out["material_ty"][11] = 7
    elif which == "ior":
        out["param"] = np.where(out["material_ty"] == 3, rng.uniform(1.05, 2.4, n), out["param"]).astype(F)
        out["param"][glass[3]] = 0.8            # (a value below 1)
    elif which == "ground":
        first, count = n - 1, 1
        out["material_ty"][n - 1], out["albedo"][n - 1], out["param"][n - 1] = 2, (0.9, 0.7, 0.3), 0.05
    else:
        first, count = {"partial": (37, 100), "batch+1": (5, BATCH + 1), "2batches": (3, 2 * BATCH)}[which]
        idx = np.arange(first, first + count)
        rotate_types(out, idx, rng)
        out["albedo"][idx] = rng.uniform(0.1, 0.9, (count, 3)).astype(F)
    return sc, [(first, mrt.materials_of(out[first:first + count]))], out


def state(mrt, name, sc, rng_mode=0, max_w=1.0, noise=False, **kw):
    """a context of the layout with the scene; a list with a type outside 1..3 goes through mrt_set_world_raw, as raw::World allows"""
    st = mrt.State(mrt.Args(W, H, SPP, DEPTH, max_w), seed=SEED, **kw)
    if LAYOUTS[name][1]:
        st.debug_set_hierarchy(*LAYOUTS[name][1])
    st.debug_set_boxes(2)
    if noise:
        st.set_noise_tracking(True)
    known = (sc["material_ty"] >= 1) & (sc["material_ty"] <= 3)
    if known.all():
        st.set_world(sc)
    else:
        packable = sc.copy()
        packable["material_ty"][~known] = 1
        w, vec4, f32, i32 = mrt.pack_world(packable)
        i32[w.spheres.material_ty_base_idx + np.nonzero(~known)[0]] = sc["material_ty"][~known]
        st.set_world_raw(w, vec4, f32, i32)
    st.set_camera(camera(mrt))
    if rng_mode:
        st.set_rng_mode(rng_mode)
    return st


def apply(st, calls, **kw):
    for first, m in calls:
        st.update_materials(first, m, **kw)


_fresh = {}


def fresh(mrt, name, which, rng_mode):
    """two frames of a fresh context given the edited list: (shade, counters, framebuffer), computed once"""
    key = (name, which, rng_mode)
    if key not in _fresh:
        _, _, sc_new = edit(mrt, scene(mrt, name), which)
        with state(mrt, name, sc_new, rng_mode) as st:
            shade = st.debug_read_hierarchy()["shade"]
            st.render(2)
            _fresh[key] = (shade, st.read_counters(), st.read_framebuffer())
    return _fresh[key]


# (two batches are 384 spheres: the small layout has 201, so that edit runs on the large one alone)
CASES = [(n, w, 0) for n in NAMES for w in EDITS if (n, w) != ("small", "2batches")] + [("small", "types", 1)]


@pytest.mark.parametrize("name,which,rng_mode", CASES, ids=[f"{n}-{w}-{'counter' if r else 'stream'}" for n, w, r in CASES])
def test_an_edit_equals_set_world_of_the_edited_list(mrt, oracle, name, which, rng_mode):
    sc0, calls, sc_new = edit(mrt, scene(mrt, name), which)
    with state(mrt, name, sc0, rng_mode) as st:
        apply(st, calls)
        shade = st.debug_read_hierarchy()["shade"]
        st.render(2)
        got, counters = st.read_framebuffer(), st.read_counters()
    ref, ref_counters = oracle_frames(oracle, mrt, ("materials", name, which), [sc_new, sc_new], rng_mode)
    assert_same(got, counters, ref, ref_counters, f"{name}, {which}")
    want_shade, want_counters, want_fb = fresh(mrt, name, which, rng_mode)
    assert np.array_equal(_bits(shade), _bits(want_shade)), np.nonzero((_bits(shade) != _bits(want_shade)).any(1))[0][:8]
    assert counters["member_tests"] == want_counters["member_tests"]        # the hierarchy is the same
    assert np.array_equal(_bits(got), _bits(want_fb))
    if which == "types":
        assert np.array_equal(_bits(shade[11, 4:]), _bits([1, 1, 1, 0]))
    if which in ("batch+1", "2batches"):        # the spheres beside the range are the build's
        first, m = calls[0]
        with state(mrt, name, sc0) as before:
            keep = before.debug_read_hierarchy()["shade"]
        outside = np.r_[0:first, first + len(m):len(sc0)]
        assert np.array_equal(_bits(shade[outside]), _bits(keep[outside])) and not np.array_equal(_bits(shade[first + len(m) - 1]), _bits(keep[first + len(m) - 1]))


@pytest.mark.parametrize("rng_mode", [0, 1], ids=["stream-rng", "counter-rng"])
def test_ordering_against_frames_in_flight(mrt, oracle, rng_mode):
    """sixteen frames in flight pinned, no sync anywhere: three frames shade with the old materials, three with the new ones"""
    name = "small"
    sc0, calls, sc_new = edit(mrt, scene(mrt, name), "types")
    with state(mrt, name, sc0, rng_mode) as st:
        st.debug_set_frames_in_flight(16)
        for _ in range(3):
            st.redraw()
        apply(st, calls)
        for _ in range(3):
            st.redraw()
        got, counters = st.read_framebuffer(), st.read_counters()
        assert st.frames_done == 6
    ref, ref_counters = oracle_frames(oracle, mrt, ("materials ordering",), [sc0] * 3 + [sc_new] * 3, rng_mode)
    assert_same(got, counters, ref, ref_counters, "ordering")
    old, _ = oracle_frames(oracle, mrt, ("materials ordering", "old"), [sc0] * 6, rng_mode)
    assert not np.array_equal(_bits(ref), _bits(old))                   # (the edit shows in the picture)


def test_nothing_else_moved(mrt):
    name = "small"
    sc0, calls, _ = edit(mrt, scene(mrt, name), "types")
    with state(mrt, name, sc0) as st:
        st.set_auto_regroup(True, check_every=2)
        st.set_schedule_hint(4, 1)
        st.render(3)
        st.sync()
        h0, sch, stats, masks = st.debug_read_hierarchy(), st.get_schedule(), st.read_regroup_stats(), st.debug_read_camera_masks()
        img, frames = st.read_framebuffer(), st.frames_done
        assert h0["axes"] != (1.0, 1.0, 1.0)
        apply(st, calls)
        st.sync()
        h1 = st.debug_read_hierarchy()
        assert set(h0) == set(h1)
        for k, v in h0.items():
            if k == "shade":
                continue
            same = np.array_equal(np.ascontiguousarray(v).view(np.uint8), np.ascontiguousarray(h1[k]).view(np.uint8)) if isinstance(v, np.ndarray) else v == h1[k]
            assert same, k
        assert np.array_equal(_bits(h0["shade"][:, :4]), _bits(h1["shade"][:, :4]))
        assert not np.array_equal(_bits(h0["shade"][:, 4:]), _bits(h1["shade"][:, 4:]))
        assert st.get_schedule() == sch and st.read_regroup_stats() == stats and st.get_auto_regroup()["enabled"]
        after = st.debug_read_camera_masks()
        assert after["built"] == masks["built"] and after["entries"] == masks["entries"]
        if masks["masks"] is not None:
            assert np.array_equal(after["masks"], masks["masks"])
        # the accumulation is not restarted
        assert st.frames_done == frames and np.array_equal(_bits(st.read_framebuffer()), _bits(img))
        assert st.debug_check_context() is None
        # the policy's update count: the edit was none -- the second geometry update is the one that checks
        xyzr = np.concatenate([sc0["center"], sc0["radius"][:, None]], 1).astype(F)
        st.update_spheres(0, xyzr)
        assert st.read_regroup_stats()["checks"] == 0
        st.update_spheres(0, xyzr)
        assert st.read_regroup_stats()["checks"] == 1


def test_every_refusal_leaves_the_context_untouched(mrt, oracle):
    name = "large-quad"
    sc = scene(mrt, name)
    n = len(sc)
    _, calls, _ = edit(mrt, sc, "recolour")
    m = calls[0][1]
    ref, ref_counters = oracle_frames(oracle, mrt, ("materials refusals",), [sc], 0)
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=SEED) as st:
        with pytest.raises(mrt.MrtError) as e:
            st.update_materials(0, m[:4])
        assert e.value.status == MRT_ERR_NO_SCENE
    with state(mrt, name, sc) as st:
        L, ctx = st._L, st._ctx
        h0 = st.debug_read_hierarchy()

        def untouched(what):
            st.reset()
            st.render(1)
            assert_same(st.read_framebuffer(), st.read_counters(), ref, ref_counters, what)
            assert np.array_equal(_bits(st.debug_read_hierarchy()["shade"]), _bits(h0["shade"])), what

        for first, count in ((n - 3, 4), (n, 1), (0xFFFFFFFF, 2), (n + 1, 0), (0, n + 1)):
            assert L.mrt_update_materials(ctx, first, count, m.ctypes.data, 0) == MRT_ERR_INVALID_ARG, (first, count)
            untouched(f"range {first}, {count}")
        assert L.mrt_update_materials(ctx, 0, 3, None, 0) == MRT_ERR_INVALID_ARG
        untouched("null array")
        for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
            assert L.mrt_update_materials(ctx, 0, 3, m.ctypes.data, flags) == MRT_ERR_INVALID_ARG, flags
            untouched(f"flags {flags:#x}")
        with pytest.raises(mrt.MrtError) as e:
            st.update_materials(n - 1, m[:2])
        assert e.value.status == MRT_ERR_INVALID_ARG and "mrt_update_materials" in str(e.value)
        # count == 0: MRT_OK, nothing queued -- with and without an array, at the end of the list, with the flag
        assert L.mrt_update_materials(ctx, n, 0, None, 0) == 0 and L.mrt_update_materials(ctx, 0, 0, m.ctypes.data, 1) == 0
        st.update_materials(5, m[:0])
        untouched("count 0")
        assert st.debug_check_context() is None


@pytest.mark.parametrize("name", NAMES)
def test_interleaved_with_updates_and_a_regroup(mrt, oracle, name):
    """queued back to back, no wait between them: a scatter, a regroup, the type edit, a partial move"""
    sc = scene(mrt, name)
    first1, upd1, sc1 = motion(mrt, sc, "scatter")
    _, calls, sc2 = edit(mrt, sc1, "types")
    first3, upd3, sc3 = motion(mrt, sc2, "partial")
    with state(mrt, name, sc) as st:
        st.update_spheres(first1, upd1)
        st.regroup_spheres()
        apply(st, calls)
        st.update_spheres(first3, upd3)
        st.render(2)
        got, counters = st.read_framebuffer(), st.read_counters()
    assert np.array_equal(sc3["material_ty"], sc2["material_ty"]) and sc3["material_ty"][11] == 7
    ref, ref_counters = oracle_frames(oracle, mrt, ("materials interleaved", name), [sc3, sc3], 0)
    assert_same(got, counters, ref, ref_counters, name)


def test_guides_are_rebuilt_for_the_edited_materials(mrt, oracle):
    name = "small"
    sc0, calls, sc_new = edit(mrt, scene(mrt, name), "types")
    with state(mrt, name, sc0) as st:
        g0 = st.debug_read_guides()
        apply(st, calls)
        g = st.debug_read_guides()
    hit, t, normal, albedo = expected_guides(oracle, sc_new, g["rays"])
    assert np.array_equal(g0["index"], g["index"]) and (hit >= 0).any() and (hit < 0).any()      # the geometry is the same
    assert not np.array_equal(_bits(g0["albedo"]), _bits(g["albedo"]))
    assert np.array_equal(g["index"].ravel(), hit)
    assert np.array_equal(_bits(g["t"]).ravel(), _bits(t))
    assert np.array_equal(_bits(g["normal"]).reshape(-1, 3), _bits(normal))
    assert np.array_equal(_bits(g["albedo"]).reshape(-1, 3), _bits(albedo))


def test_the_denoised_image_is_the_one_of_the_edited_scene(mrt):
    name = "small"
    sc0, calls, sc_new = edit(mrt, scene(mrt, name), "types")
    with state(mrt, name, sc0, noise=True) as a:
        apply(a, calls)
        a.render(3)
        img_a = a.read_denoised()
    with state(mrt, name, sc_new, noise=True) as b:
        b.render(3)
        img_b = b.read_denoised()
    assert np.array_equal(_bits(img_a), _bits(img_b)), mismatch_report(img_a, img_b)
    # ... also when the guides had been built for the old materials
    with state(mrt, name, sc0, noise=True) as a:
        a.debug_read_guides()
        apply(a, calls)
        a.render(3)
        assert np.array_equal(_bits(a.read_denoised()), _bits(img_b))


TEMPORAL_CAMERA = dict(mode=1, lookfrom=(0.0, 1.5, 5.0), lookat=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), vfov_deg=30.0, defocus_angle_deg=0.0,
                       focus_dist=10.0)


@pytest.mark.parametrize("response", [False, True], ids=["plain", "response-on"])
def test_restart_history_restarts_the_pixels_of_the_edited_spheres_alone(mrt, response):
    """Two contexts through the same four steps; before the fourth both recolour spheres [0, 50), one with
    MRT_MATERIALS_RESTART_HISTORY.  Pixels whose first hit is none of them agree bit for bit; at the others the flagged context
    holds step 4's "without" branch, H0 = (cur, 1), H1 = (Lc, Lc Lc, t, index bits), and the unflagged one a longer history.  A
    fifth step leaves the flagged pixels at length 2: the step's own snapshot had restored "previous"."""
    name = "small"
    sc = scene(mrt, name)
    n = len(sc)
    new = sc[:50].copy()
    new["albedo"] = np.random.default_rng(77).uniform(0.05, 0.95, (50, 3)).astype(F)
    m = mrt.materials_of(new)
    out = []
    for flagged in (False, True):
        with state(mrt, name, sc, max_w=0.0) as st:
            st.set_camera(mrt.Camera(**TEMPORAL_CAMERA))
            st.set_temporal(True)
            if response:
                st.set_temporal_response(True, fast_history=4)
            for k in range(4):
                if k == 3:
                    st.update_materials(0, m, restart_history=flagged)
                    if flagged:                 # the NaN is in "previous" until the step's snapshot
                        pre = st.debug_read_temporal(n)["prev_xyzr"]
                        assert np.isnan(pre[:50, 3]).all() and np.array_equal(_bits(pre[:, :3]), _bits(sc["center"])) \
                            and np.array_equal(_bits(pre[50:, 3]), _bits(sc["radius"][50:]))
                st.redraw()
                st.temporal_step()
            g, fb, t4 = st.debug_read_guides(), st.read_framebuffer(), st.debug_read_temporal(n)
            assert np.array_equal(_bits(t4["prev_xyzr"][:, 3]), _bits(sc["radius"]))      # restored
            st.redraw()
            st.temporal_step()
            t5 = st.debug_read_temporal(n)
            shade = st.debug_read_hierarchy()["shade"]
            assert st.debug_check_context() is None
        out.append((g, fb, t4, t5, shade))
    (g, fb, plain4, plain5, shade_a), (g_b, fb_b, flag4, flag5, shade_b) = out
    assert np.array_equal(g["index"], g_b["index"]) and np.array_equal(_bits(fb), _bits(fb_b)) and np.array_equal(_bits(shade_a), _bits(shade_b))
    fin = np.isfinite(fb[..., :3]).all(-1)
    inside = (g["index"] >= 0) & (g["index"] < 50) & fin
    assert inside.sum() >= 20 and (g["index"] < 0).any() and (g["index"] >= 50).any(), int(inside.sum())
    for k in ("h0", "h1"):
        assert np.array_equal(_bits(plain4[k])[~inside], _bits(flag4[k])[~inside]), k
    Lc = lum(fb)
    want0 = np.concatenate([fb[..., :3], np.ones((H, W, 1), F)], -1)
    want1 = np.stack([Lc, Lc * Lc, g["t"], index_bits(g["index"])], -1).astype(F)
    assert np.array_equal(_bits(flag4["h0"])[inside], _bits(want0)[inside])
    assert np.array_equal(_bits(flag4["h1"])[inside], _bits(want1)[inside])
    assert (plain4["h0"][..., 3][inside] > 1.0).all(), plain4["h0"][..., 3][inside]
    assert (flag5["h0"][..., 3][inside] == 2.0).all(), flag5["h0"][..., 3][inside]
    assert (plain5["h0"][..., 3][inside] > 2.0).all()


def test_both_shards_make_the_edit(mrt):
    name = "small"
    sc0, calls, sc_new = edit(mrt, scene(mrt, name), "recolour")
    states = [state(mrt, name, sc0, shard=(r, 2)) for r in range(2)]
    try:
        for st in states:
            apply(st, calls)
        for _ in range(2):
            for st in states:
                st.redraw()
        mrt.gather(states, 0)
        got = states[0].read_gathered()
    finally:
        for st in states:
            st.close()
    _, _, want = fresh(mrt, name, "recolour", 0)
    assert np.array_equal(_bits(got), _bits(want)), mismatch_report(got, want)
