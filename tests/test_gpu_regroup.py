"""mrt_regroup_spheres on the GPU (include/myraytracer_amd.h, "scene"; myraytracer_amd/csrc/regroup.hip): the grouping made anew
on the device, refitted in stream order.

Every regroup is held to three things: member_index, read back with mrt_debug_read_hierarchy, equals tests/regroup_ref.py's
ordering of the CURRENT spheres bit for bit (tests/test_regroup_host.py holds that reference to its properties); the whole
read-back passes the float64 checker of tests/refit_ref.py; and the frames rendered afterwards equal the oracle's, on uint32
views, with the samples / world_hit_calls / rng_draws counters -- images never depend on the grouping.  Images are 20 x 12,
2 spp, depth 8, as in tests/test_gpu_update_spheres.py, whose scenes and motions these tests share.

Regroup layouts (block = mrt_debug_set_regroup_block; None = the built-in 512 clusters):
  small            201 spheres, 50 pool clusters: the block kernel alone
  small, block 4   the same with blocks of 4 clusters: 4 depths over global memory, 2 in LDS, 13 workgroups
  small, block 16  2 depths over global memory, 4 in LDS
  ragged           203 spheres without a ground: clusters of fewer than 4 members
  alone            307 spheres, 7 of them huge: 4 direct, 3 in clusters of their own behind the pool's
  large-quad       1,100 spheres, three levels, boxes
  boxes-4200       4,200 spheres, 1,050 pool clusters: 2 depths over global memory, 3 blocks"""
import numpy as np
import pytest

import refit_ref as R
import regroup_ref as G
from common import to_oracle_spheres
from myraytracer_amd import _lib
from test_gpu_superset import _rays_for
from test_gpu_update_spheres import DEPTH, H, LAYOUTS, SEED, SPP, W, assert_same, camera, motion, oracle_frames, scene
from test_regroup_host import random_scene

pytestmark = pytest.mark.gpu

MRT_ERR_INVALID_ARG, MRT_ERR_NO_SCENE = 1, 4
REGROUP_LAYOUTS = [("small", None), ("small", 4), ("small", 16), ("ragged", None), ("alone", None), ("large-quad", None), ("boxes-4200", None)]


def scene_of(mrt, name):
    if name == "ragged":
        return random_scene(mrt, 203, 1)
    if name == "alone":
        return random_scene(mrt, 307, 2, big=7)
    return scene(mrt, name)


def state(mrt, name, sc, rng_mode=0, block=None, **kw):
    st = mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=SEED, **kw)
    if LAYOUTS.get(name, (0, None))[1]:
        st.debug_set_hierarchy(*LAYOUTS[name][1])
    st.debug_set_boxes(2)
    st.set_world(sc)
    st.set_camera(camera(mrt))
    if rng_mode:
        st.set_rng_mode(rng_mode)
    if block:
        st.debug_set_regroup_block(block)
    return st


def same_hierarchy(a, b, but=()):
    for k, v in a.items():
        if k not in but:
            assert np.array_equal(v, b[k]) if isinstance(v, np.ndarray) else v == b[k], k


@pytest.mark.parametrize("which", [None, "scatter", "jitter"], ids=["as-built", "scatter", "jitter"])
@pytest.mark.parametrize("name,block", REGROUP_LAYOUTS, ids=[f"{n}-{b or 'default'}" for n, b in REGROUP_LAYOUTS])
def test_member_index_is_the_references_bit_for_bit(mrt, name, block, which):
    sc = scene_of(mrt, name)
    first, upd, sc_new = motion(mrt, sc, which) if which else (0, None, sc)
    with state(mrt, name, sc, block=block) as st:
        before = st.debug_read_hierarchy()
        if which:
            st.update_spheres(first, upd)
        st.regroup_spheres()
        info = st.debug_regroup_info()
        h = st.debug_read_hierarchy()
        assert st.debug_check_context() is None
    real = G.real_slots(before)
    xyzr = R.xyzr_of(sc_new)
    want = G.regroup(before["midx"], real, info["n_pool"], xyzr[:, :3])
    G.check_permutation(before["midx"], h["midx"], real, info["n_pool"])
    bad = np.nonzero(h["midx"] != want)[0]
    assert len(bad) == 0, f"{len(bad)} member slots differ from the reference; first: slot {bad[0]} holds {h['midx'][bad[0]]}, want {want[bad[0]]}"
    assert not np.array_equal(h["midx"], before["midx"])
    assert h["axes"] == (1.0, 1.0, 1.0) and np.array_equal(h["origin"], before["origin"])
    R.check(h, xyzr)
    size0 = 1 << (info["n_pool"] - 1).bit_length()
    assert info["block"] == (block or 512) and info["global_depths"] + info["lds_depths"] == size0.bit_length() - 1
    assert info["global_depths"] == sum(1 for d in range(size0.bit_length() - 1) if (size0 >> d) > info["block"]), info
    assert (info["global_depths"] > 0) == ((name, block) in (("small", 4), ("small", 16), ("boxes-4200", None))) and info["lds_depths"] > 0
    if name == "ragged":
        assert G.pool_layout(real, info["n_pool"])[1].sum(1).min() < 4
    if name == "alone":
        assert h["n_direct"] == 4 and real[4 * info["n_pool"]:4 * info["n_pool"] + 12].reshape(3, 4).sum(1).tolist() == [1, 1, 1]


@pytest.mark.parametrize("rng_mode", [0, 1], ids=["stream-rng", "counter-rng"])
@pytest.mark.parametrize("name", ["small", "large-quad"])
def test_frames_after_update_and_regroup_are_the_oracles(mrt, oracle, name, rng_mode):
    sc = scene(mrt, name)
    first, upd, sc_new = motion(mrt, sc, "scatter")
    with state(mrt, name, sc, rng_mode) as st:
        st.update_spheres(first, upd)
        st.regroup_spheres()
        st.render(1)
        st.sync()
        got, counters = st.read_framebuffer(), st.read_counters()
    ref, ref_counters = oracle_frames(oracle, mrt, (name, "scatter"), [sc_new], rng_mode)
    assert_same(got, counters, ref, ref_counters, name)


def test_a_regroup_between_sixteen_frames_in_flight_changes_no_frame(mrt, oracle):
    """no sync between the calls; an update before frame 4, regroups before frames 2, 5 and 6 (block 4: every kernel of the path)"""
    name = "small"
    sc = scene(mrt, name)
    _, upd, sc_new = motion(mrt, sc, "scatter")
    per_frame = [sc] * 4 + [sc_new] * 4
    with state(mrt, name, sc, block=4) as st:
        st.debug_set_frames_in_flight(16)
        for f in range(8):
            if f == 4:
                st.update_spheres(0, upd)
            if f in (2, 5, 6):
                st.regroup_spheres()
            st.redraw()
        got, counters = st.read_framebuffer(), st.read_counters()
        assert st.frames_done == 8
    ref, ref_counters = oracle_frames(oracle, mrt, ("regroup-ordering",), per_frame, 0)
    assert_same(got, counters, ref, ref_counters, "regroup between frames in flight")


@pytest.mark.parametrize("sweep", [1, 2], ids=["valu-sweep", "matrix-core-sweep"])
@pytest.mark.parametrize("name", ["small", "large-quad"])
def test_candidate_sets_after_a_regroup(mrt, oracle, name, sweep):
    """tests/test_gpu_update_spheres.py's test_candidate_sets_after_an_update, with a regroup behind the update"""
    sc = scene(mrt, name)
    first, upd, sc_new = motion(mrt, sc, "scatter")
    rays = _rays_for(np.random.default_rng(3), sc_new, 2048, 1536, 512)[:4096]
    a2 = (rays[:, 3:].astype(np.float64) ** 2).sum(1)
    rays = rays[np.abs(a2 - 1.0) < 5e-6]
    packed = oracle.pack_world(to_oracle_spheres(oracle, sc_new))
    ref_hit, ref_t, ref_set, required = oracle.world_hit_batch(packed, rays)
    with state(mrt, name, sc) as st:
        st.update_spheres(first, upd)
        st.regroup_spheres()
        st.debug_set_sweep(sweep)
        assert st.debug_sweep_variant() == sweep
        hit, t, cand = st.debug_world_hit(rays, len(sc))
    assert required.sum() > len(rays)
    assert not (required & ~cand).any(), f"{int((required & ~cand).sum())} (ray, sphere) pairs with a discriminant >= 0 never reached the root tests"
    assert not (cand & ~ref_set).any()
    assert np.array_equal(hit, ref_hit) and np.array_equal(t.view(np.uint32)[hit >= 0], ref_t.view(np.uint32)[hit >= 0])


def test_a_regroup_repairs_what_a_scatter_costs(mrt):
    """large-quad after the scatter motion: member tests over the same 4 frames, grouping kept against regrouped"""
    name = "large-quad"
    sc = scene(mrt, name)
    first, upd, _ = motion(mrt, sc, "scatter")
    tests, images = [], []
    for regroup in (False, True):
        with state(mrt, name, sc) as st:
            st.update_spheres(first, upd)
            if regroup:
                st.regroup_spheres()
            st.render(4)
            c = st.read_counters()
            tests.append(c["member_tests"] / c["world_hit_calls"])
            images.append(st.read_framebuffer())
    print(f"large-quad after scatter: member tests per world_hit {tests[0]:.2f} kept, {tests[1]:.2f} regrouped (x {tests[1] / tests[0]:.3f})")
    assert tests[1] < tests[0]
    assert np.array_equal(images[0].view(np.uint32), images[1].view(np.uint32))


@pytest.mark.parametrize("name,block", [("small", 4), ("boxes-4200", None)])
def test_a_second_regroup_changes_nothing(mrt, name, block):
    sc = scene(mrt, name)
    first, upd, _ = motion(mrt, sc, "scatter")
    with state(mrt, name, sc, block=block) as st:
        st.update_spheres(first, upd)
        st.regroup_spheres()
        a = st.debug_read_hierarchy()
        st.regroup_spheres()
        same_hierarchy(a, st.debug_read_hierarchy())


def test_refusals_and_no_ops_leave_the_context_untouched(mrt):
    L = _lib.load()
    assert L.mrt_regroup_spheres(None) == MRT_ERR_INVALID_ARG
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=SEED) as st:
        with pytest.raises(mrt.MrtError) as e:
            st.regroup_spheres()
        assert e.value.status == MRT_ERR_NO_SCENE and st.debug_check_context() is None
        with pytest.raises(mrt.MrtError) as e:
            st.debug_regroup_info()
        assert e.value.status == MRT_ERR_NO_SCENE
        for bad in (1, 2, 3, 6, 1024):
            with pytest.raises(mrt.MrtError):
                st.debug_set_regroup_block(bad)
    # a pool of one cluster (and a ground): MRT_OK, nothing queued -- not even the sweep's space changes
    sc = scene(mrt, "small")[-5:]
    with state(mrt, "small", sc) as st:
        st.render(2)
        img, cnt, h0 = st.read_framebuffer(), st.read_counters(), st.debug_read_hierarchy()
        assert st.debug_regroup_info()["n_pool"] == 1
        st.regroup_spheres()
        same_hierarchy(h0, st.debug_read_hierarchy())
        assert st.debug_regroup_info()["global_depths"] == st.debug_regroup_info()["lds_depths"] == 0
        assert np.array_equal(st.read_framebuffer().view(np.uint32), img.view(np.uint32)) and st.read_counters() == cnt
        assert st.frames_done == 2 and st.debug_check_context() is None
    # factor 0 (no clustering): no pool at all
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=SEED) as st:
        assert L.mrt_debug_set_cluster_factor(st._ctx, 0.0) == 0
        st.set_world(scene(mrt, "small"))
        h0 = st.debug_read_hierarchy()
        assert st.debug_regroup_info()["n_pool"] == 0
        st.regroup_spheres()
        same_hierarchy(h0, st.debug_read_hierarchy())


def test_a_pinned_schedule_the_accumulation_and_the_guides_survive_a_regroup(mrt):
    name = "small"
    sc = scene(mrt, name)
    with state(mrt, name, sc) as st:
        st.set_noise_tracking(True)
        st.set_schedule_hint(4, 1)
        for _ in range(3):
            st.redraw()
        sch, cnt = st.get_schedule(), st.read_counters()
        assert (sch["div"], sch["mult"], sch["settled"]) == (4, 1, True)
        img, den = st.read_framebuffer(), st.read_denoised()
        st.regroup_spheres()
        assert st.get_schedule() == sch and st.frames_done == 3
        assert np.array_equal(st.read_framebuffer().view(np.uint32), img.view(np.uint32))
        assert {k: st.read_counters()[k] for k in ("samples", "world_hit_calls", "rng_draws")} == {k: cnt[k] for k in ("samples", "world_hit_calls", "rng_draws")}
        assert np.array_equal(st.read_denoised().view(np.uint32), den.view(np.uint32))      # the guides were not rebuilt, nor need be
        st.redraw()
        after = st.get_schedule()
        assert (after["div"], after["mult"], after["settled"], after["frames_in_flight"]) == (4, 1, True, sch["frames_in_flight"])
        assert st.frames_done == 4 and st.debug_check_context() is None
