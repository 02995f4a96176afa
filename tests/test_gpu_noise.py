"""The noise estimate on the GPU (include/myraytracer_amd.h, "noise estimate"): the tracked blend's per-texel variance S is
bit-identical to the float32 restatement (tests/noise_ref.py) of the oracle's frames, in every frame schedule; tracking changes
no image; the device reduction's report and tile map equal numpy's; the estimate is close to the real error; lifecycle,
render_until and shards."""
import math

import numpy as np
import pytest

import noise_ref
from common import to_oracle_camera, to_oracle_spheres
from noise_cases import check_report as _check_report, crafted

pytestmark = pytest.mark.gpu

MRT_ERR_STATE = 7
W, H, SPP, DEPTH, FRAMES = 48, 27, 3, 8, 6


def _scene(mrt, name):
    if name == "default":
        return mrt.scene_default(), None
    return mrt.scene_cover(1, name == "cover-glass")


def _setup(mrt, st, name, rng_mode=0):
    spheres, cam = _scene(mrt, name)
    st.set_world(spheres)
    if cam is not None:
        st.set_camera(cam)
    if rng_mode:
        st.set_rng_mode(rng_mode)


def _oracle_means(oracle, mrt, name, seed, w, h, spp, depth, frames, rng_mode=0, start=0):
    spheres, cam = _scene(mrt, name)
    pw = oracle.pack_world(to_oracle_spheres(oracle, spheres))
    seeds = oracle.fill_seeds(seed, w, h)
    return [oracle.render_frame(w, h, spp, depth, pw, to_oracle_camera(oracle, cam), seeds, oracle.frame_shuffle(seed, k), 0.0,
                                rng_mode=rng_mode) for k in range(start, start + frames)]


def _expected(oracle, mrt, name, seed, max_w, rng_mode=0, frames=FRAMES, w=W, h=H, spp=SPP, depth=DEPTH):
    means = _oracle_means(oracle, mrt, name, seed, w, h, spp, depth, frames, rng_mode)
    weights = [oracle.frame_weight(k, max_w) for k in range(frames)]
    return noise_ref.accumulate(means, weights)


def _run(st, schedule, frames=FRAMES):
    if schedule == "redraw":
        for _ in range(frames):
            st.redraw()
    elif schedule in ("batch-lane", "batch-layers"):
        st.debug_set_frame_batching(2 if schedule == "batch-lane" else 3)
        st.render(frames)
    elif schedule == "in-flight-16":
        st.set_schedule_hint(8, 2)
        for _ in range(frames):
            st.redraw()
    st.sync()


@pytest.mark.parametrize("schedule", ["redraw", "batch-lane", "batch-layers", "in-flight-16"])
@pytest.mark.parametrize("max_w", [1.0, 0.75])
@pytest.mark.parametrize("scene,rng_mode", [("default", 0), ("default", 1), ("cover-glass", 0), ("cover", 1)])
def test_tracked_variance_is_bit_exact(mrt, oracle, scene, rng_mode, max_w, schedule):
    fb_want, S_want, K = _expected(oracle, mrt, scene, 5, max_w, rng_mode)
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, max_w), seed=5) as st:
        _setup(mrt, st, scene, rng_mode)
        st.set_noise_tracking(True)
        _run(st, schedule)
        S = st.read_noise()
        fb = st.read_framebuffer()
        st.noise_query(0.05, 0.01)
        rep = st.noise_result(wait=True)
        tiles = st.read_noise_tiles()
    assert np.array_equal(fb.view(np.uint32), fb_want.view(np.uint32))
    bad = np.argwhere(S.view(np.uint32) != S_want.view(np.uint32))
    assert bad.size == 0, (bad[:4].tolist(), S[tuple(bad[0])], S_want[tuple(bad[0])])
    assert rep["frames_done"] == FRAMES and rep["noise_factor"] == mrt.noise_factor(FRAMES, max_w)
    assert rep["noise_factor"] == K
    _check_report(rep, noise_ref.report(S_want, fb_want, K, 0.05, 0.01))
    want_tiles = noise_ref.tiles(S_want, fb_want, K, 0.05, 0.01)
    assert tiles.shape == (4, 6) and np.array_equal(tiles[:want_tiles.shape[0]], want_tiles)


def test_a_shard_tracks_its_packed_rows(mrt, oracle):
    fb_want, S_want, K = _expected(oracle, mrt, "cover-glass", 5, 1.0)
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=5, shard=(1, 3)) as st:
        _setup(mrt, st, "cover-glass")
        st.set_noise_tracking(True)
        _run(st, "redraw")
        S = st.read_noise()
    rows = [mrt.shard_global_row(r, 1, 3) for r in range(S.shape[0])]
    for r, g in enumerate(rows):
        if g < H:
            assert np.array_equal(S[r].view(np.uint32), S_want[g].view(np.uint32)), r
        else:
            assert not S[r].any()                                           # padding rows stay 0


def test_tracking_changes_no_image(mrt, oracle):
    out = []
    for track in (False, True):
        with mrt.State(mrt.Args(96, 54, 2, 50, 1.0), seed=4) as st:
            _setup(mrt, st, "cover-glass")
            st.set_noise_tracking(track)
            for k in range(12):
                st.redraw()
                if track and k % 3 == 0:
                    st.noise_query()
                    st.noise_result(wait=False)
            out.append((st.read_framebuffer(), st.read_counters(), st.frames_done))
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert out[0][1] == out[1][1] and out[0][2] == out[1][2] == 12


def test_reports_agree_across_schedules(mrt):
    reps = []
    for schedule in ("redraw", "batch-lane", "batch-layers", "in-flight-16"):
        with mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=9) as st:
            _setup(mrt, st, "cover")
            st.set_noise_tracking(True)
            _run(st, schedule)
            st.noise_query(0.03, 0.02)
            r = st.noise_result(wait=True)
            reps.append((r, st.read_noise_tiles()))
    for r, t in reps[1:]:
        assert r == reps[0][0] and np.array_equal(t.view(np.uint32), reps[0][1].view(np.uint32))


def _crafted():
    return crafted(((1, 1), (1, 37), (3, 5), (9, 13), (17, 64), (20, 250), (8, 257), (40, 1030)))


@pytest.mark.parametrize("K", [0.05, 1.0 / 63.0, math.inf])
def test_debug_reduction_on_crafted_inputs(mrt, K):
    with mrt.State(mrt.Args(16, 16, 1, 8, 1.0), seed=1) as st:
        for S, rgba in _crafted():
            for thr, floor in ((0.02, 0.01), (0.5, 0.0), (1e-3, 0.3)):
                rep, tiles = st.debug_noise_reduce(S, rgba, K, thr, floor)
                want = noise_ref.report(S, rgba, K, thr, floor)
                assert rep["pixels"] + rep["non_finite"] == S.size
                _check_report(rep, want)
                wt = noise_ref.tiles(S, rgba, K, thr, floor)
                assert np.array_equal(tiles.view(np.uint32), wt.view(np.uint32)), (S.shape, thr, floor)


def test_the_estimate_means_what_it_says(mrt):
    """64 frames x 1 spp of the default scene: the estimated RMSE of the displayed luminance against the actual one, measured
    against a 4,096-spp render with another seed (seeds 1 / 2 checked on the CPU oracle beforehand: ratio 1.018)."""
    args = mrt.Args(64, 36, 1, 8, 1.0)
    with mrt.State(args, seed=1) as st:
        _setup(mrt, st, "default")
        st.set_noise_tracking(True)
        st.render(64)
        st.noise_query()
        rep = st.noise_result(wait=True)
        fb = st.read_framebuffer()
    with mrt.State(mrt.Args(64, 36, 4096, 8, 1.0), seed=2) as st:
        _setup(mrt, st, "default")
        st.redraw()
        ref = st.read_framebuffer()
    actual = math.sqrt(float(np.mean((noise_ref.lum(fb).astype(np.float64) - noise_ref.lum(ref)) ** 2)))
    assert rep["frames_done"] == 64 and rep["pixels"] == 64 * 36
    assert 0.8 * actual <= rep["rmse"] <= 1.25 * actual, (rep["rmse"], actual)


def test_lifecycle(mrt):
    with mrt.State(mrt.Args(64, 40, 2, 8, 1.0), seed=8) as st:
        _setup(mrt, st, "cover")
        with pytest.raises(mrt.MrtError) as e:
            st.noise_query()
        assert e.value.status == MRT_ERR_STATE
        assert st.noise_result(wait=True) is None
        st.redraw()
        with pytest.raises(mrt.MrtError) as e:
            st.set_noise_tracking(True)
        assert e.value.status == MRT_ERR_STATE
        st.reset()
        st.set_noise_tracking(True)
        for _ in range(4):
            st.redraw()
        st.noise_query()
        st.reset()                                                   # unread reports are discarded, tracking stays on
        assert st.noise_result(wait=True) is None
        st.redraw()
        assert not st.read_noise().any()                             # one frame: S == 0 exactly
        st.noise_query()
        r = st.noise_result(wait=True)
        assert math.isinf(r["noise_factor"]) and math.isinf(r["rmse"]) and math.isinf(r["rel_rmse"]) and math.isinf(r["max_se"])
        assert r["above"] == r["pixels"] == 64 * 40
        for _ in range(15):
            st.redraw()
        st.noise_query()
        before = st.noise_result(wait=True)
        spheres, cam = mrt.scene_cover(1, False)
        cam2 = mrt.Camera(cam.mode, tuple(cam.lookfrom), tuple(np.add(cam.lookat, (1.5, 0.0, 0.0))), tuple(cam.vup),
                          cam.vfov_deg, cam.defocus_angle_deg, cam.focus_dist)
        st.set_camera(cam2)                                          # no reset: two pictures blended
        st.redraw()
        st.noise_query()
        after = st.noise_result(wait=True)
        assert after["rmse"] > 1.1 * before["rmse"], (before["rmse"], after["rmse"])
    # reports in seq order; a result before anything finished; destroy with queries outstanding
    st = mrt.State(mrt.Args(1280, 720, 16, 50, 1.0), seed=8)
    _setup(mrt, st, "cover-glass")
    st.set_noise_tracking(True)
    st.redraw()
    st.noise_query()
    r = st.noise_result(wait=False)
    assert r is None or r["seq"] == 1
    seen = []
    for _ in range(12):
        st.redraw()
        st.noise_query()
        r = st.noise_result(wait=False)
        if r is not None:
            seen.append(r["seq"])
    assert seen == sorted(seen)
    st.close()


def test_render_until_stops_at_the_predicted_check(mrt, oracle):
    w, h, spp, depth, every = 32, 18, 2, 8, 4
    frames = 48
    means = _oracle_means(oracle, mrt, "default", 3, w, h, spp, depth, frames)
    weights = [oracle.frame_weight(k, 1.0) for k in range(frames)]
    rel = {}
    for n in range(every, frames + 1, every):
        fb, S, K = noise_ref.accumulate(means[:n], weights[:n])
        rel[n] = noise_ref.report(S, fb, K)["rel_rmse"]
    checks = sorted(rel)
    target = (rel[checks[4]] + rel[checks[5]]) / 2                   # first met at the 6th check (24 frames) ...
    first = next(n for n in checks if rel[n] <= target)
    with mrt.State(mrt.Args(w, h, spp, depth, 1.0), seed=3) as st:
        _setup(mrt, st, "default")
        done, rep = st.render_until(target, max_frames=frames, check_every=every)
        fb_until = st.read_framebuffer()
    assert rep["frames_done"] == first and done == first + every     # ... plus the one lagged chunk
    assert rep["rel_rmse"] <= target
    with mrt.State(mrt.Args(w, h, spp, depth, 1.0), seed=3) as st:
        _setup(mrt, st, "default")
        for _ in range(done):
            st.redraw()
        assert np.array_equal(st.read_framebuffer().view(np.uint32), fb_until.view(np.uint32))
    with mrt.State(mrt.Args(w, h, spp, depth, 1.0), seed=3) as st:   # an unreachable target stops at the cap
        _setup(mrt, st, "default")
        done, rep = st.render_until(0.0, max_frames=10, check_every=every)
        assert done == 10 and rep["frames_done"] == 10


def test_shards_combine_to_the_whole_image(mrt):
    from myraytracer_amd import dist
    args = mrt.Args(70, 45, 2, 50, 1.0)
    with mrt.State(args, seed=6) as whole:
        _setup(mrt, whole, "cover-glass")
        whole.set_noise_tracking(True)
        for _ in range(5):
            whole.redraw()
        whole.noise_query()
        want = whole.noise_result(wait=True)
        S_whole = whole.read_noise()
    states = [mrt.State(args, seed=6, shard=(i, 3)) for i in range(3)]
    try:
        reps = []
        for s in states:
            _setup(mrt, s, "cover-glass")
            s.set_noise_tracking(True)
            for _ in range(5):
                s.redraw()
            s.noise_query()
            reps.append(s.noise_result(wait=True))
        for i, s in enumerate(states):
            S = s.read_noise()
            for r in range(S.shape[0]):
                g = mrt.shard_global_row(r, i, 3)
                if g < 45:
                    assert np.array_equal(S[r].view(np.uint32), S_whole[g].view(np.uint32)), (i, r)
        got = dist.combine_noise_reports(reps)
    finally:
        for s in states:
            s.close()
    for k in ("pixels", "above", "non_finite", "max_se", "frames_done", "noise_factor"):
        assert got[k] == want[k], k
    for k in ("sum_var", "sum_lum", "rmse", "rel_rmse"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k


def test_set_shard_reallocates_tracking(mrt):
    with mrt.State(mrt.Args(40, 30, 1, 8, 1.0), seed=2) as st:
        _setup(mrt, st, "default")
        st.set_noise_tracking(True)
        assert st._L.mrt_set_shard(st._ctx, 1, 2) == 0              # tracking follows the new shard's rows
        for _ in range(3):
            st.redraw()
        S = st.read_noise()
        assert S.shape == (st.shard_info()[2], 40) and S.any()
        st.noise_query()
        assert st.noise_result(wait=True)["pixels"] == sum(1 for r in range(S.shape[0]) if mrt.shard_global_row(r, 1, 2) < 30) * 40
