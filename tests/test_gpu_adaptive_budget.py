"""Adaptive sampling by budget on the GPU (include/myraytracer_amd.h, "adaptive sampling by budget"), at 44 x 20: 6 x 3 tiles with
a partial last column and a partial top band.  The summed-S tile map against tests/budget_ref.py bit for bit, with a report equal
to the other kind's (uniform, K = +inf, per tile, a shard); render_budget against the restated allocation rendered by hand through
render_tiles; the mandatory frames; the whole-frame path; render_until(budget=N); nothing to do, the refusals, and
render_adaptive's choice of report left as it was."""
import numpy as np
import pytest

import budget_ref
from noise_cases import check_same_but_kind, raw_report

pytestmark = pytest.mark.gpu

MRT_ERR_NO_SCENE, MRT_ERR_STATE = 4, 7
W, H, SPP, DEPTH = 44, 20, 2, 6
TILES = 18


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _state(mrt, seed=5, max_w=1.0, scene=True, tracking=True, **kw):
    st = mrt.State(mrt.Args(W, H, SPP, DEPTH, max_w), seed=seed, **kw)
    if scene:
        st.set_world(mrt.scene_default())
    if tracking:
        st.set_noise_tracking(True)
    return st


def _both_kinds(mrt, st, thr=0.3, fl=0.02):
    """a kind-0 and a kind-1 query of the same state: the reports are equal in every field but seq and reserved; returns the
    kind-1 query's map"""
    st.noise_query(thr, fl)
    a = raw_report(mrt, st)
    st.noise_query(thr, fl, tile_map="sum_s")
    b = raw_report(mrt, st)
    check_same_but_kind(mrt, a, b)
    return st.read_noise_tiles()


@pytest.mark.parametrize("accumulation", ["uniform", "no-estimate", "per-tile"])
def test_the_summed_s_map_bit_for_bit(mrt, accumulation):
    S, rgba = budget_ref.map_fixture(H, W)
    want = budget_ref.tile_sums(S, rgba)
    with _state(mrt) as st:
        if accumulation == "uniform":
            st.render(3)
        n = np.array([0, 1, 2, 3, 5, 9] * 3, np.uint32) if accumulation == "per-tile" else None
        st.debug_load_accumulation(rgba, S, n)
        got = _both_kinds(mrt, st)
        assert got.shape == (3, 6)
        assert np.array_equal(_bits(got), _bits(want)), (got, want)
        rep = st.noise_result()
        assert rep["non_finite"] == 5 and rep["pixels"] == W * H - 5
        assert np.isinf(rep["noise_factor"]) == (accumulation != "uniform")


def test_a_shards_map_and_report(mrt):
    with _state(mrt, shard=(1, 2)) as st:
        st.render(3)
        got = _both_kinds(mrt, st)
        st.sync()
        assert np.array_equal(_bits(got), _bits(budget_ref.tile_sums(st.read_noise(), st.read_framebuffer())))
        assert (got > 0).any()


def _by_hand(st, max_w, budget, max_frames):
    """the allocation restated from the map and n_t as read back, rendered through render_tiles call by call"""
    k, res = budget_ref.allocate(st.read_noise_tiles(), st.tile_frames(), max_w, budget, max_frames)
    for tiles, run in budget_ref.levels(k):
        st.render_tiles(tiles, run)
    return k, res


@pytest.mark.parametrize("max_w", [1.0, 0.75])
def test_render_budget_is_the_allocation_rendered_by_hand(mrt, max_w):
    with _state(mrt, 9, max_w) as a, _state(mrt, 9, max_w) as b:
        for st in (a, b):
            st.render(4)
            st.noise_query(tile_map="sum_s")
            assert st.noise_result(wait=True)["seq"] == 1
        for chunk, (budget, max_frames, seq) in enumerate(((20, 4, 0), (30, 3, 2))):
            before = a.frames_done
            got = a.render_budget(budget, max_frames, seq)
            k, want = _by_hand(b, max_w, budget, max_frames)
            assert got["used_seq"] == chunk + 1
            assert np.array_equal(got["k"], k), (got["k"], k)
            assert 0 < got["tile_frames"] <= budget and got["k"].min() < got["k"].max()
            for f in ("tile_frames", "tiles", "frames"):
                assert got[f] == want[f], f
            for f in ("var_before", "var_after"):
                assert np.float64(got[f]).view(np.uint64) == np.float64(want[f]).view(np.uint64), f
            a.sync()
            b.sync()
            assert a.frames_done == b.frames_done and a.frames_done - before == got["frames"] > 0
            assert np.array_equal(a.tile_frames(), b.tile_frames())
            assert np.array_equal(_bits(a.read_framebuffer()), _bits(b.read_framebuffer()))
            assert np.array_equal(_bits(a.read_noise()), _bits(b.read_noise()))
            ca, cb = a.read_counters(), b.read_counters()
            for f in ("samples", "world_hit_calls", "rng_draws"):
                assert ca[f] == cb[f], f
            # the second chunk: a diverged accumulation, K per tile, the report named
            for st in (a, b):
                st.noise_query(tile_map="sum_s")
        assert (a.tile_frames() != a.tile_frames().ravel()[0]).any()


def test_mandatory_frames_come_first_and_alone(mrt):
    n = np.array([0, 1, 5] * 6, np.uint32)
    with _state(mrt) as st:
        rng = np.random.default_rng(2)
        S = rng.uniform(0.5, 2.0, (H, W)).astype(np.float32)
        rgba = np.ones((H, W, 4), np.float32)
        st.debug_load_accumulation(rgba, S, n)
        st.noise_query(tile_map="sum_s")
        seq = st.noise_result(wait=True)["seq"]
        got = st.render_budget(8, 4, seq)              # the demand is 6 x 2 + 6 x 1 = 18
        want = np.zeros(TILES, np.uint32)
        want[np.nonzero(n < 2)[0][:8]] = 1             # j = 0 over the tiles with n_t < 2, t ascending, until the budget ends
        assert np.array_equal(got["k"].ravel(), want) and got["tile_frames"] == 8 and got["frames"] == 1
        st.sync()
        assert st.frames_done == 1 and np.array_equal(st.tile_frames().ravel(), n + want)
        k_ref, _ = budget_ref.allocate(budget_ref.tile_sums(S, rgba), n, 1.0, 8, 4)
        assert np.array_equal(k_ref.ravel(), want)


def test_the_same_count_for_every_tile_renders_whole_frames(mrt):
    with _state(mrt, 3) as a, _state(mrt, 3) as b:
        for st in (a, b):
            st.render(3)
        a.noise_query(tile_map="sum_s")
        a.noise_result(wait=True)
        assert (a.read_noise_tiles() > 0).all()           # every gain is positive
        got = a.render_budget(TILES * 3, 3)
        assert (got["k"] == 3).all() and got["frames"] == 3 and got["tile_frames"] == TILES * 3
        b.render(3)
        a.sync()
        b.sync()
        assert a.frames_done == b.frames_done == 6 and (a.tile_frames() == 6).all()
        assert np.array_equal(_bits(a.read_framebuffer()), _bits(b.read_framebuffer()))
        assert np.array_equal(_bits(a.read_noise()), _bits(b.read_noise()))
        a.read_denoised()                                  # still a uniform accumulation: not refused


def test_nothing_to_do(mrt):
    with _state(mrt) as st:
        st.render(3)
        got = st.render_budget(10, 4)                      # no summed-S report yet
        assert got["used_seq"] == 0 and got["tile_frames"] == 0 and st.frames_done == 3
        st.noise_query(tile_map="sum_s")
        st.noise_result(wait=True)
        got = st.render_budget(0, 4)
        assert got["used_seq"] == 1 and got["tile_frames"] == 0 and not got["k"].any() and st.frames_done == 3
        st.sync()
        st.debug_load_accumulation(None, np.zeros((H, W), np.float32), None)
        st.noise_query(tile_map="sum_s")
        got = st.render_budget(50, 4, 2)
        assert got["used_seq"] == 2 and got["tile_frames"] == 0 and got["var_before"] == 0.0 and st.frames_done == 3
        assert (st.tile_frames() == 3).all()


def test_render_until_with_a_budget_is_deterministic_and_adapts(mrt):
    runs = []
    for _ in range(2):
        with _state(mrt, 21, tracking=False) as st:
            frames, rep = st.render_until(0.0, 30, check_every=4, threshold=0.1, floor=0.05, budget=2 * TILES)
            st.sync()
            runs.append((frames, rep["seq"], st.read_framebuffer(), st.tile_frames()))
    (f0, q0, fb0, t0), (f1, q1, fb1, t1) = runs
    assert f0 == f1 >= 30 and q0 == q1 and np.array_equal(t0, t1) and np.array_equal(_bits(fb0), _bits(fb1))
    assert t0.min() >= 8 and t0.min() < t0.max()           # two uniform chunks, then the budget's choice
    assert int(t0.sum()) <= 8 * TILES + (q0 - 1) * 2 * TILES


def _refused(mrt, st, status, *args):
    with pytest.raises(mrt.MrtError) as e:
        st.render_budget(*args)
    assert e.value.status == status


def test_refusals(mrt):
    with _state(mrt, tracking=False) as st:
        _refused(mrt, st, MRT_ERR_STATE, 10, 4)
    with _state(mrt, shard=(0, 2)) as st:
        st.render(2)
        st.noise_query(tile_map="sum_s")
        _refused(mrt, st, MRT_ERR_STATE, 10, 4)
    with _state(mrt, scene=False) as st:
        _refused(mrt, st, MRT_ERR_NO_SCENE, 10, 4)
    with _state(mrt) as st:
        st.render(2)
        for bad in (0, 33):
            with pytest.raises(mrt.MrtError):
                st.render_budget(10, bad)
        st.noise_query()                                   # report 1: the other kind
        st.noise_query(tile_map="sum_s")                   # report 2
        _refused(mrt, st, MRT_ERR_STATE, 10, 4, 1)
        _refused(mrt, st, MRT_ERR_STATE, 10, 4, 3)         # not queued
        for _ in range(8):
            st.noise_query(tile_map="sum_s")
        _refused(mrt, st, MRT_ERR_STATE, 10, 4, 2)         # older than the ring of 8
        assert st.frames_done == 2
        assert st.render_budget(10, 4, 10)["used_seq"] == 10 and st.frames_done > 2


def test_render_adaptive_keeps_choosing_among_its_own_reports(mrt):
    outs = []
    for with_budget_query in (False, True):
        with _state(mrt, 6) as st:
            st.render(4)
            st.noise_query(0.05, 0.02)
            st.noise_result(wait=True)
            if with_budget_query:
                st.noise_query(0.05, 0.02, tile_map="sum_s")
                assert st.noise_result(wait=True)["seq"] == 2
                with pytest.raises(mrt.MrtError) as e:
                    st.render_adaptive(1, 2)
                assert e.value.status == MRT_ERR_STATE and st.frames_done == 4
            used, sel = st.render_adaptive(1, 0)
            assert used == 1 and 0 < sel
            st.sync()
            outs.append((sel, st.read_framebuffer(), st.tile_frames()))
    assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][2], outs[1][2])
    assert np.array_equal(_bits(outs[0][1]), _bits(outs[1][1]))
