"""The matrix-core sweep in a scaled space on the GPU: the cover scene as it ships (flat in y), turned so that its
flat axis is x, then z, and a scene with no flat axis, each rendered bit-identical to the oracle; the space chosen is the one the
host tests expect; and forcing any other space -- the world's own included -- changes no bit of the image and no counter the
reference has, only how many member tests the walk needs."""
import numpy as np
import pytest

from common import gpu_render, mismatch_report, oracle_render

pytestmark = pytest.mark.gpu


def _turned(mrt, a, b):
    """the cover scene with glass and its camera, coordinates a and b exchanged"""
    sc, cam = mrt.scene_cover(1, True)
    out = sc.copy()
    c = np.asarray(sc["center"]).copy()
    c[:, [a, b]] = c[:, [b, a]]
    out["center"] = c

    def swap(v):
        v = list(v)
        v[a], v[b] = v[b], v[a]
        return tuple(v)
    cam2 = mrt.Camera(cam.mode, swap(cam.lookfrom), swap(cam.lookat), swap(cam.vup), cam.vfov_deg, cam.defocus_angle_deg, cam.focus_dist)
    return out, cam2


def _blob(mrt):
    rng = np.random.default_rng(4)
    sc = np.zeros(400, mrt.SPHERE_DTYPE)
    for i in range(len(sc)):
        sc[i] = (tuple(rng.uniform(-6, 6, 3)), float(rng.uniform(0.15, 0.4)), 1 + i % 3, tuple(rng.uniform(0.2, 0.9, 3)), 0.1 if i % 3 == 1 else 1.5)
    cam = mrt.Camera(mode=1, lookfrom=(14, 5, 9), lookat=(0, 0, 0), vup=(0, 1, 0), vfov_deg=40.0, defocus_angle_deg=0.3, focus_dist=17.0)
    return sc, cam


def _render(mrt, sc, cam, axis, w=160, h=90, spp=4, depth=50, seed=3):
    with mrt.State(mrt.Args(w, h, spp, depth, 1.0), seed=seed) as st:
        if axis is not None:
            st.debug_set_sweep_axes(axis)
            st.debug_set_sweep(2)                            # (a space nobody would choose may fail the camera's slack test)
        st.set_world(sc)
        st.set_camera(cam)
        assert st.debug_sweep_variant() == 2                 # the matrix-core sweep: the one that has a space of its own
        axes = st.debug_sweep_axes()
        st.render(1)
        st.sync()
        return st.read_framebuffer(), st.read_counters(), axes


@pytest.mark.parametrize("case,expect", [("y", (1, 2, 1)), ("x", (2, 1, 1)), ("z", (1, 1, 2)), ("none", (1, 1, 1))])
def test_flat_axis_scenes_render_bit_identical_to_the_oracle(mrt, oracle, case, expect):
    sc, cam = dict(y=lambda: mrt.scene_cover(1, True), x=lambda: _turned(mrt, 0, 1), z=lambda: _turned(mrt, 2, 1), none=lambda: _blob(mrt))[case]()
    cnt = oracle.Counters()
    ref = oracle_render(oracle, sc, cam, 160, 90, 4, 50, 3, counters=cnt)
    got, gcnt, axes = _render(mrt, sc, cam, None)
    assert axes == tuple(float(v) for v in expect)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), mismatch_report(got, ref)
    assert (gcnt["samples"], gcnt["world_hit_calls"], gcnt["rng_draws"]) == (cnt.samples, cnt.world_hit_calls, cnt.rng_draws)


def test_any_forced_space_gives_the_same_frame_and_the_chosen_one_fewer_member_tests(mrt):
    sc, cam = mrt.scene_cover(1, True)
    base, bcnt, axes = _render(mrt, sc, cam, (1, 1, 1))
    assert axes == (1.0, 1.0, 1.0)
    tests = {}
    for axis in [None, (1, 2, 1), (1, 4, 1), (2, 1, 1), (4, 2, 1)]:
        got, cnt, axes = _render(mrt, sc, cam, axis)
        assert axes == tuple(float(v) for v in (axis or (1, 2, 1)))
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (axis, mismatch_report(got, base))
        assert all(cnt[k] == bcnt[k] for k in ("samples", "world_hit_calls", "rng_draws")), axis
        tests[axis] = cnt["member_tests"]
    print("member tests per frame: world space", bcnt["member_tests"], tests)
    assert tests[None] == tests[(1, 2, 1)] < bcnt["member_tests"] < tests[(2, 1, 1)]


@pytest.mark.parametrize("axis", [(1, 2, 1), (1, 4, 1), (4, 1, 2)])
def test_candidate_sets_in_a_scaled_space_are_exactly_the_reference_set(mrt, oracle, axis):
    """tests/test_gpu_superset.py's claim under a forced D, the proven one and two the host would not choose: the spheres that
    reach the root tests are exactly those whose f32 discriminant is not < 0, none missing that is not entirely behind the origin."""
    from common import to_oracle_spheres
    from test_gpu_superset import _normalize, _rays_for
    rng = np.random.default_rng(8)
    sc, cam = mrt.scene_cover(1, True)
    rays = _rays_for(rng, sc, 3000, 3000, 2000)
    cam_o = np.tile(np.asarray(cam.lookfrom, np.float32), (2000, 1))
    cam_d = _normalize(oracle, rng.uniform([-11, 0, -11], [11, 1.5, 11], (2000, 3)) - cam_o)
    rays = np.concatenate([rays, np.concatenate([cam_o, cam_d], 1)], 0)
    ref_hit, ref_t, ref_set, required = oracle.world_hit_batch(oracle.pack_world(to_oracle_spheres(oracle, sc)), rays)
    with mrt.State(mrt.Args(16, 16), seed=1) as st:
        st.debug_set_sweep_axes(axis)
        st.debug_set_sweep(2)
        st.set_world(sc)
        assert st.debug_sweep_variant() == 2 and st.debug_sweep_axes() == tuple(float(v) for v in axis)
        hit, t, cand = st.debug_world_hit(rays, len(sc))
    assert not (required & ~cand).any(), int((required & ~cand).sum())
    assert not (cand & ~ref_set).any()
    assert np.array_equal(hit, ref_hit) and np.array_equal(t.view(np.uint32)[hit >= 0], ref_t.view(np.uint32)[hit >= 0])
