"""Adaptive sampling on the GPU (include/myraytracer_amd.h, "adaptive sampling"): mixed schedules of whole and subset frames are
bit-identical to the float32 restatement (tests/adaptive_ref.py) of the oracle's frames -- framebuffer, S and the per-tile frame
counts -- in both RNG modes and every frame schedule; a list of every tile before divergence is a plain redraw; reports, tile
maps and render_adaptive's selection follow the restatement; render_until(adaptive=True) is deterministic and spends fewer
samples than uniform rendering to the same stop; refusals and the lifecycle."""
import zlib

import numpy as np
import pytest

import adaptive_ref
from common import to_oracle_camera, to_oracle_spheres
from present_ref import encode_host

pytestmark = pytest.mark.gpu

MRT_ERR_INVALID_ARG, MRT_ERR_NO_SCENE, MRT_ERR_STATE = 1, 4, 7
W, H, SPP, DEPTH = 48, 27, 3, 8


def _scene(mrt, name):
    if name == "default":
        return mrt.scene_default(), None
    return mrt.scene_cover(1, name == "cover-glass")


def _setup(mrt, st, name, rng_mode=0, tracking=True):
    spheres, cam = _scene(mrt, name)
    st.set_world(spheres)
    if cam is not None:
        st.set_camera(cam)
    if rng_mode:
        st.set_rng_mode(rng_mode)
    if tracking:
        st.set_noise_tracking(True)


class Means:
    """The oracle's per-frame means of one scene, frame k with shuffle mrt_frame_shuffle(seed, k), rendered on demand."""

    def __init__(self, oracle, mrt, name, seed, w, h, spp, depth, rng_mode=0):
        spheres, cam = _scene(mrt, name)
        self.o, self.args = oracle, (w, h, spp, depth, oracle.pack_world(to_oracle_spheres(oracle, spheres)), to_oracle_camera(oracle, cam))
        self.seeds, self.seed, self.rng_mode, self.cache = oracle.fill_seeds(seed, w, h), seed, rng_mode, {}

    def __getitem__(self, k):
        if k not in self.cache:
            self.cache[k] = self.o.render_frame(*self.args, self.seeds, self.o.frame_shuffle(self.seed, k), 0.0, rng_mode=self.rng_mode)
        return self.cache[k]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _schedule(rng, n_tiles, steps):
    """A seeded mix: ('full', k) = render(k), ('tiles', list, k) = render_tiles(list, k); the first steps are whole frames."""
    out = [("full", 1)]
    for _ in range(steps):
        if rng.random() < 0.25:
            out.append(("full", int(rng.integers(1, 3))))
        else:
            n = int(rng.integers(1, n_tiles))
            out.append(("tiles", rng.choice(n_tiles, n, replace=False).astype(np.uint32), int(rng.integers(1, 3))))
    return out


def _run_and_expect(st, acc, means, schedule, per_call, after_tiles=None):
    for step in schedule:
        k = step[-1] if per_call else 1
        reps = 1 if per_call else step[-1]
        for _ in range(reps):
            if step[0] == "full":
                st.render(k)
                for _ in range(k):
                    acc.frame(means[acc.frames_done])
            else:
                st.render_tiles(step[1], k)
                for _ in range(k):
                    acc.frame(means[acc.frames_done], step[1])
                if after_tiles is not None:
                    after_tiles(st)


@pytest.mark.parametrize("schedule", ["single", "multi", "pinned-8x2"])
@pytest.mark.parametrize("max_w", [1.0, 0.75])
@pytest.mark.parametrize("scene,rng_mode", [("default", 0), ("cover-glass", 0), ("cover", 1), ("default", 1)])
def test_mixed_schedules_match_the_oracle_bit_for_bit(mrt, oracle, scene, rng_mode, max_w, schedule):
    mixed_schedule_matches_the_oracle(mrt, oracle, scene, rng_mode, max_w, schedule)


def mixed_schedule_matches_the_oracle(mrt, oracle, scene, rng_mode, max_w, schedule, camera_tables=None, after_tiles=None):
    """the body of the test above; camera_tables: mrt_debug_set_camera_masks' value (None: the library's rule, which gives a
    48x27 image the masks); after_tiles(st): called behind every render_tiles (tests/test_gpu_camera_list_launches.py)"""
    means = Means(oracle, mrt, scene, 11, W, H, SPP, DEPTH, rng_mode)
    acc = adaptive_ref.Accum(H, W, max_w)
    sched = _schedule(np.random.default_rng(zlib.crc32(f"{scene} {rng_mode} {max_w} {schedule}".encode())), acc.n_tiles, 5)
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, max_w), seed=11) as st:
        if camera_tables is not None:
            st.debug_set_camera_masks(camera_tables)
        _setup(mrt, st, scene, rng_mode)
        if schedule == "pinned-8x2":
            st.set_schedule_hint(8, 2)
        if schedule == "multi":
            st.debug_set_frame_batching(2)          # k frames of one call in one launch, the in-lane form (stream mode)
        _run_and_expect(st, acc, means, sched, per_call=schedule == "multi", after_tiles=after_tiles)
        st.sync()
        assert st.frames_done == acc.frames_done
        assert np.array_equal(st.tile_frames(), acc.tile_frames())
        assert np.array_equal(_bits(st.read_framebuffer()), _bits(acc.fb))
        assert np.array_equal(_bits(st.read_noise()), _bits(acc.S))


def test_unlisted_tiles_keep_their_texels_and_S(mrt):
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=2) as st:
        _setup(mrt, st, "cover-glass")
        st.render(3)
        fb0, S0 = st.read_framebuffer(), st.read_noise()
        tiles = np.array([0, 7, 8, 20, 23], np.uint32)          # (23: the last band's tile at the image's right edge)
        st.render_tiles(tiles, 2)
        fb1, S1 = st.read_framebuffer(), st.read_noise()
        listed = np.isin(adaptive_ref.tile_of(H, W), tiles)
        assert np.array_equal(_bits(fb1[~listed]), _bits(fb0[~listed]))
        assert np.array_equal(_bits(S1[~listed]), _bits(S0[~listed]))
        assert not np.array_equal(_bits(fb1[listed]), _bits(fb0[listed]))
        n = st.tile_frames().ravel()
        assert (n[tiles] == 5).all() and (np.delete(n, tiles) == 3).all() and st.frames_done == 5


@pytest.mark.parametrize("rng_mode", [0, 1])
def test_every_tile_before_divergence_is_a_redraw(mrt, rng_mode):
    outs = []
    for how in ("tiles", "redraw"):
        with mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=4) as st:
            _setup(mrt, st, "cover", rng_mode, tracking=False)
            all_tiles = np.arange(st.tile_frames().size, dtype=np.uint32)[::-1].copy()
            for _ in range(3):
                if how == "tiles":
                    st.render_tiles(all_tiles, 1)
                else:
                    st.redraw()
            st.sync()
            outs.append((st.read_framebuffer(), st.read_counters(), st.tile_frames(), st.frames_done))
    (fa, ca, ta, na), (fb, cb, tb, nb) = outs
    assert np.array_equal(_bits(fa), _bits(fb)) and na == nb == 3
    for k in ("samples", "world_hit_calls", "rng_draws"):
        assert ca[k] == cb[k], k
    assert (ta == 3).all() and (tb == 3).all()


def test_reports_and_tile_maps_after_divergence(mrt, oracle):
    max_w, thr, fl = 1.0, 0.3, 0.02
    means = Means(oracle, mrt, "cover-glass", 6, W, H, SPP, DEPTH)
    acc = adaptive_ref.Accum(H, W, max_w)
    rng = np.random.default_rng(5)
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, max_w), seed=6) as st:
        _setup(mrt, st, "cover-glass")
        # before divergence: the uniform report
        _run_and_expect(st, acc, means, [("full", 3)], per_call=True)
        st.noise_query(thr, fl)
        rep = st.noise_result(wait=True)
        want = acc.report(thr, fl, diverged=False)
        assert rep["above"] == want["above"] and rep["noise_factor"] == want["noise_factor"]
        # some tiles two frames ahead, then a whole frame; then every tile but the last one frame more
        for sched in ([("tiles", rng.choice(acc.n_tiles, 17, replace=False).astype(np.uint32), 2), ("full", 1)],
                      [("tiles", np.arange(acc.n_tiles - 1, dtype=np.uint32), 1)]):
            _run_and_expect(st, acc, means, sched, per_call=True)
            st.noise_query(thr, fl)
            rep = st.noise_result(wait=True)
            want = acc.report(thr, fl)
            for k in ("pixels", "above", "non_finite", "max_se", "noise_factor"):
                assert rep[k] == want[k], (k, rep[k], want[k])
            assert rep["sum_var"] == pytest.approx(want["sum_var"], rel=1e-12)
            assert rep["rel_rmse"] == pytest.approx(want["rel_rmse"], rel=1e-12)
            assert np.array_equal(_bits(st.read_noise_tiles()), _bits(acc.tiles(thr, fl)))
    # a tile never rendered since divergence began at frames_done = 0 has K = +inf: "no estimate yet"
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, max_w), seed=6) as st:
        _setup(mrt, st, "default")
        st.render_tiles(np.arange(5, dtype=np.uint32), 3)
        st.noise_query(thr, fl)
        rep = st.noise_result(wait=True)
        assert rep["noise_factor"] == float("inf") and rep["rmse"] == float("inf")
        tm = st.read_noise_tiles().ravel()
        assert np.isinf(tm[5:]).all() and np.isfinite(tm[:5]).all()


def test_render_adaptive_selects_from_the_report_it_names(mrt, oracle):
    thr, fl = 0.25, 0.02
    means = Means(oracle, mrt, "cover-glass", 8, W, H, SPP, DEPTH)
    acc = adaptive_ref.Accum(H, W, 1.0)
    with mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=8) as st:
        _setup(mrt, st, "cover-glass")
        # no report: every tile
        used, sel = st.render_adaptive(1, 0)
        assert (used, sel) == (0, acc.n_tiles)
        acc.frame(means[0])
        _run_and_expect(st, acc, means, [("full", 3)], per_call=True)
        st.noise_query(thr, fl)
        maps = [acc.tiles(thr, fl, diverged=False)]
        _run_and_expect(st, acc, means, [("full", 2)], per_call=True)
        st.noise_query(thr, fl)
        maps.append(acc.tiles(thr, fl, diverged=False))
        # explicit: report 1, although report 2 is newer
        want = adaptive_ref.select(maps[0], thr)
        used, sel = st.render_adaptive(2, 1)
        assert used == 1 and sel == len(want) and 0 < sel < acc.n_tiles
        for _ in range(2):
            acc.frame(means[acc.frames_done], want)
        st.sync()
        assert np.array_equal(st.tile_frames(), acc.tile_frames())
        assert np.array_equal(_bits(st.read_framebuffer()), _bits(acc.fb))
        # report_seq 0 = the newest finished: report 2 (finished: the sync above)
        want = adaptive_ref.select(maps[1], thr)
        used, sel = st.render_adaptive(1, 0)
        assert used == 2 and sel == len(want)
        acc.frame(means[acc.frames_done], want)
        # after divergence: the per-tile report's map
        st.noise_query(thr, fl)
        want = adaptive_ref.select(acc.tiles(thr, fl), thr)
        used, sel = st.render_adaptive(1, 3)
        assert used == 3 and sel == len(want)
        acc.frame(means[acc.frames_done], want)
        st.sync()
        assert np.array_equal(_bits(st.read_framebuffer()), _bits(acc.fb))
        assert np.array_equal(st.tile_frames(), acc.tile_frames())
        # not queued, and older than the ring of 8
        for bad in (4, 99):
            with pytest.raises(mrt.MrtError) as e:
                st.render_adaptive(1, bad)
            assert e.value.status == MRT_ERR_STATE
        for _ in range(8):
            st.noise_query(thr, fl)
        with pytest.raises(mrt.MrtError) as e:
            st.render_adaptive(1, 3)
        assert e.value.status == MRT_ERR_STATE
        # a threshold no pixel exceeds: nothing selected, nothing queued
        st.noise_query(1e30, fl)
        n_before = st.frames_done
        used, sel = st.render_adaptive(1, 12)
        assert used == 12 and sel == 0 and st.frames_done == n_before


def _uniform_until_clean(st, thr, fl, every, cap):
    st.set_noise_tracking(True)
    st.render(every)
    st.noise_query(thr, fl)
    while True:
        n = min(every, cap - st.frames_done)
        if n > 0:
            st.render(n)
        rep = st.noise_result(wait=True)
        if rep["above"] == 0 or rep["frames_done"] >= cap:
            return rep
        st.noise_query(thr, fl)


def test_render_until_adaptive_is_deterministic_and_saves_samples(mrt):
    w, h, spp, depth, thr, fl, every, cap = 64, 48, 2, 16, 0.5, 0.05, 8, 1200
    runs = []
    for _ in range(2):
        with mrt.State(mrt.Args(w, h, spp, depth, 1.0), seed=21) as st:
            _setup(mrt, st, "cover-glass", tracking=False)
            frames, rep = st.render_until(0.0, cap, check_every=every, threshold=thr, floor=fl, adaptive=True)
            st.sync()
            runs.append((frames, rep, st.read_framebuffer(), st.read_counters()["samples"], st.tile_frames()))
    (f0, r0, fb0, s0, t0), (f1, r1, fb1, s1, t1) = runs
    assert f0 == f1 and r0["seq"] == r1["seq"] and s0 == s1
    assert np.array_equal(_bits(fb0), _bits(fb1)) and np.array_equal(t0, t1)
    assert r0["above"] == 0, r0
    assert t0.min() < t0.max()                     # it did adapt
    with mrt.State(mrt.Args(w, h, spp, depth, 1.0), seed=21) as st:
        _setup(mrt, st, "cover-glass", tracking=False)
        rep = _uniform_until_clean(st, thr, fl, every, cap)
        st.sync()
        s_uniform = st.read_counters()["samples"]
    assert s0 < s_uniform, (s0, s_uniform, rep["frames_done"], r0["frames_done"])


def test_refusals(mrt):
    args = mrt.Args(W, H, SPP, DEPTH, 1.0)
    with mrt.State(args, seed=1) as st:
        with pytest.raises(mrt.MrtError) as e:
            st.render_tiles([0, 1])
        assert e.value.status == MRT_ERR_NO_SCENE
        _setup(mrt, st, "default", tracking=False)
        st.render_tiles([])                                          # n == 0: nothing
        assert st.frames_done == 0
        with pytest.raises(mrt.MrtError) as e:
            st.render_adaptive(1)                                    # tracking off
        assert e.value.status == MRT_ERR_STATE
        n_tiles = st.tile_frames().size
        for bad in ([n_tiles], [3, 4, 3]):
            with pytest.raises(mrt.MrtError) as e:
                st.render_tiles(bad)
            assert e.value.status == MRT_ERR_INVALID_ARG
        assert st._L.mrt_render_tiles(st._ctx, None, 2, 1) == MRT_ERR_INVALID_ARG
        st.set_rng_mode(1)
        st.set_samples_per_frame(65)
        with pytest.raises(mrt.MrtError) as e:
            st.render_tiles([0])
        assert e.value.status == MRT_ERR_INVALID_ARG
        st.set_samples_per_frame(64)
        st.render_tiles([0])                                         # (<= 64 spp: one layer)
        assert st.frames_done == 1
    with mrt.State(args, seed=1, shard=(0, 2)) as st:
        _setup(mrt, st, "default", tracking=False)
        with pytest.raises(mrt.MrtError) as e:
            st.render_tiles([0])
        assert e.value.status == MRT_ERR_STATE
    with mrt.State(args, seed=1) as st:
        _setup(mrt, st, "default")
        st.render(2)
        st.read_denoised()                                           # (uniform: allowed)
        st.render_tiles([1, 2])
        with pytest.raises(mrt.MrtError) as e:
            st.read_denoised()
        assert e.value.status == MRT_ERR_STATE
        with pytest.raises(mrt.MrtError) as e:
            st.present("rgba8", denoise=True)
        assert e.value.status == MRT_ERR_STATE


def test_reset_returns_to_a_fresh_accumulation_and_presents_work(mrt):
    L = mrt._lib.load()
    args = mrt.Args(W, H, SPP, DEPTH, 0.75)
    with mrt.State(args, seed=3) as st:
        _setup(mrt, st, "cover")
        st.render(2)
        st.render_tiles([0, 5, 9, 10], 3)
        st.redraw()
        st.present("rgba8", flip=True)
        img, info = st.acquire_presented(newest=True, wait=True)
        assert info["frames_done"] == 6
        assert np.array_equal(img, encode_host(L, st.read_framebuffer(), "rgba8", flip=True))
        st.release_presented()
        st.reset()
        assert (st.tile_frames() == 0).all()
        st.render(2)
        st.render_tiles([3, 4], 1)
        st.sync()
        got = (st.read_framebuffer(), st.read_noise(), st.tile_frames())
    with mrt.State(args, seed=3) as st:
        _setup(mrt, st, "cover")
        st.render(2)
        st.render_tiles([3, 4], 1)
        st.sync()
        want = (st.read_framebuffer(), st.read_noise(), st.tile_frames())
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert np.array_equal(got[2], want[2])
