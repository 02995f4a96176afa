"""Budget allocation on the device (include/myraytracer_amd.h, "budget allocation on the device"): mrt_noise_query_budget plans
with the query, mrt_read_budget_plan reads the plan, mrt_render_planned renders it.  The yardstick is the host's
mrt_budget_allocate on the map the query left and the n it was queued at: k bit for bit, the integer fields equal, the variance
sums equal to the blocked reference (tests/budget_plan_ref.py) bit for bit.

The image sizes and what each crosses in budget.hip (256 tiles a workgroup, one tile a thread; 64 tiles a block of sums, one
block a wave; the last kernel adds 64 blocks' sums a round; at most 2,048 workgroups, so none handles more than 4,096 tiles below
2^19 tiles):
    8 x 8       1 tile:      one lane of one wave; every pass's tail is 255 idle threads
    24 x 16     6 tiles:     a partial wave, one partial block of sums
    520 x 8     65 tiles:    one over a wave: a second block of sums, of one tile
    520 x 32    260 tiles:   one over a workgroup: two workgroups share the histograms, the second a tail of 4 tiles
    1024 x 512  8,192 tiles: 32 workgroups; 128 blocks of sums, two rounds of the last kernel"""
import ctypes as C
import math

import numpy as np
import pytest

import budget_plan_ref as ref

pytestmark = pytest.mark.gpu

MRT_ERR_INVALID_ARG, MRT_ERR_TOO_SMALL, MRT_ERR_STATE = 1, 6, 7
SIZES = ((8, 8), (24, 16), (520, 8), (520, 32), (1024, 512))
S_KINDS = ("constant", "zero", "random", "nan", "negative", "inf")
MAX_FRAMES = (1, 2, 3, 32)
WEIGHTS = (1.0, 0.9, 0.5)
SPP, DEPTH = 1, 2


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _f64(x):
    return np.float64(x).view(np.uint64)


def _state(mrt, w, h, max_w=1.0, seed=5, scene="default", tracking=True, spp=SPP, depth=DEPTH, **kw):
    st = mrt.State(mrt.Args(w, h, spp, depth, max_w), seed=seed, **kw)
    if scene == "default":
        st.set_world(mrt.scene_default())
    elif scene == "cover":
        spheres, cam = mrt.scene_cover(1, False)
        st.set_world(spheres)
        st.set_camera(cam)
    if tracking:
        st.set_noise_tracking(True)
    return st


def _s_pixels(kind, h, w, rng):
    """S per pixel whose tile sums reach the host test's families: all equal, all 0, log-uniform over 12 decades, and on top of
    that tiles read as 0 (every pixel NaN: excluded by the map's rule; a negative sum) or whose sum's float is +inf"""
    tr, tx = h // 8, w // 8
    if kind == "constant":
        return np.full((h, w), 0.0125, np.float32)
    if kind == "zero":
        return np.zeros((h, w), np.float32)
    scale = np.exp(rng.uniform(math.log(1e-10), math.log(1e2), (tr, tx)))
    S = (np.repeat(np.repeat(scale, 8, 0), 8, 1) * rng.uniform(0.5, 1.5, (h, w))).astype(np.float32)
    some = np.repeat(np.repeat(rng.random((tr, tx)) < 0.3, 8, 0), 8, 1)
    if kind == "nan":
        S[some] = np.nan
        S[::3, 1::5] = np.nan                               # and single pixels of the other tiles
    elif kind == "negative":
        S[some] = -S[some]
    elif kind == "inf":
        S[-8:, -8:] = 3e38                                  # 64 x 3e38 in the last tile
    return S


def _raw_report(mrt, st):
    r = mrt._lib.MrtNoiseReport()
    st._check(st._L.mrt_noise_result(st._ctx, 1, C.byref(r)), "mrt_noise_result")
    return r


def _plan_equals_the_hosts(mrt, st, n_ref, n_host, max_w, max_frames, counted):
    """every budget of the family at the state loaded: the device's plan against mrt_budget_allocate and the blocked sums"""
    st.noise_query(0.3, 0.02, budget=0, max_frames=max_frames)
    seq = _raw_report(mrt, st).seq
    s_map = st.read_noise_tiles()
    ordered = ref.order(s_map, n_ref, max_w, max_frames)
    for budget in ref.budgets(ordered):
        if budget != 0:
            st.noise_query(0.3, 0.02, budget=budget, max_frames=max_frames)
            seq += 1
        got = st.budget_plan(seq)
        what = (s_map.shape, max_frames, budget)
        assert got["used_seq"] == seq, what
        k, want = mrt.State.budget_allocate(s_map, n_host.reshape(s_map.shape), max_w, budget, max_frames)
        assert np.array_equal(got["k"], k), (what, got["k"], k)
        for f in ("tile_frames", "tiles", "frames"):
            assert got[f] == want[f], (what, f, got[f], want[f])
        before, after = ref.blocked_sums(s_map, n_ref, k, max_w)
        assert _f64(got["var_before"]) == _f64(before) and _f64(got["var_after"]) == _f64(after), (what, got, before, after)
        counted[0] += 1
    return ordered


@pytest.mark.parametrize("max_w", WEIGHTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_plan_is_the_hosts_allocation(mrt, size, max_w):
    w, h = size
    tiles = (w // 8) * (h // 8)
    rng = np.random.default_rng(tiles * 10 + int(max_w * 10))
    rgba = np.ones((h, w, 4), np.float32)
    # max_frames: all four for the small images, taken in turn for the large ones (every state still sees every budget)
    per_state = 4 if tiles <= 65 else 2 if tiles == 260 else 1
    turn, counted, cut = 0, [0], 0
    with _state(mrt, w, h, max_w) as st:
        # the undiverged scalar n: frames_done 0, 1, 2, 17; then a loaded per-tile n: random 0 .. 40 with tiles at 0 and 1, all below 2
        states = [0, 1, 2, 17, "random", "below-2"]
        for state in states:
            if isinstance(state, int):
                if state > st.frames_done:
                    st.render(state - st.frames_done)
                n_ref, n_host, load = state, np.full(tiles, state, np.uint32), None
            else:
                n_host = rng.integers(0, 2 if state == "below-2" else 41, tiles).astype(np.uint32)
                if state == "random" and tiles >= 2:
                    n_host[0], n_host[-1] = 0, 1
                n_ref, load = n_host, n_host
            for kind in S_KINDS:                            # (the colour once a state: it only has to be finite)
                st.debug_load_accumulation(rgba if kind == S_KINDS[0] else None, _s_pixels(kind, h, w, rng), load)
                assert st.frames_done == (state if isinstance(state, int) else 17)
                for _ in range(per_state):
                    o = _plan_equals_the_hosts(mrt, st, n_ref, n_host, max_w, MAX_FRAMES[turn % 4], counted)
                    cut += o["tie"] is not None
                    turn += 1
    assert counted[0] >= 36 * per_state * 4 and (cut or tiles == 1)


@pytest.mark.parametrize("size", [(24, 16), (520, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_report_is_the_summed_s_querys(mrt, size):
    w, h = size
    tiles = (w // 8) * (h // 8)
    rng = np.random.default_rng(8)
    S = _s_pixels("nan", h, w, rng)
    with _state(mrt, w, h) as st:
        st.render(3)
        for n in (None, rng.integers(0, 9, tiles).astype(np.uint32)):          # uniform, then per tile
            st.debug_load_accumulation(np.ones((h, w, 4), np.float32), S, n)
            st.noise_query(0.3, 0.02, tile_map="sum_s")
            a, map_a = _raw_report(mrt, st), st.read_noise_tiles()
            st.noise_query(0.3, 0.02, budget=3 * tiles, max_frames=4)
            b, map_b = _raw_report(mrt, st), st.read_noise_tiles()
            assert b.seq == a.seq + 1 and a.reserved == b.reserved == 1 and a.reserved2 == b.reserved2 == 0
            for name, ctype in mrt._lib.MrtNoiseReport._fields_:
                if name == "seq":
                    continue
                x, y = getattr(a, name), getattr(b, name)
                if ctype in (C.c_double, C.c_float):
                    x, y = _f64(x), _f64(y)
                assert x == y, (name, getattr(a, name), getattr(b, name))
            assert np.array_equal(_bits(map_a), _bits(map_b))
            assert st.budget_plan(b.seq)["tile_frames"] > 0


@pytest.mark.parametrize("max_w", [1.0, 0.9])
def test_rendering_the_plan_is_rendering_the_hosts_allocation(mrt, max_w):
    budget, max_frames = 40, 4
    with _state(mrt, 64, 48, max_w, 9, "cover", spp=2, depth=6) as a, _state(mrt, 64, 48, max_w, 9, "cover", spp=2, depth=6) as b:
        for st in (a, b):
            st.render(4)
        for chunk in range(2):                              # the second on the now diverged accumulations
            a.noise_query(budget=budget, max_frames=max_frames)
            b.noise_query(tile_map="sum_s")
            seq = chunk + 1
            before = a.frames_done
            got = a.render_planned(seq)
            want = b.render_budget(budget, max_frames, seq)
            assert got["used_seq"] == want["used_seq"] == seq and got["planned_tile_frames"] == got["tile_frames"]
            assert np.array_equal(got["k"], want["k"]), (got["k"], want["k"])
            assert 0 < got["tile_frames"] <= budget and got["k"].min() < got["k"].max()
            for f in ("tile_frames", "tiles", "frames"):
                assert got[f] == want[f], f
            a.sync()
            b.sync()
            assert a.frames_done == b.frames_done and a.frames_done - before == got["frames"] > 0
            assert np.array_equal(a.tile_frames(), b.tile_frames())
            assert np.array_equal(_bits(a.read_framebuffer()), _bits(b.read_framebuffer()))
            assert np.array_equal(_bits(a.read_noise()), _bits(b.read_noise()))
            ca, cb = a.read_counters(), b.read_counters()
            for f in ("samples", "world_hit_calls", "rng_draws"):
                assert ca[f] == cb[f], f
        assert (a.tile_frames() != a.tile_frames().ravel()[0]).any()


def test_the_target_rule(mrt):
    with _state(mrt, 64, 48, scene="cover", spp=2, depth=6) as st:
        st.render(4)
        st.noise_query(budget=60, max_frames=4)
        seq = st.noise_result(wait=True)["seq"]
        plan = st.budget_plan(seq)
        assert plan["k"].max() >= 2
        st.render_tiles([0, 1, 2, 9, 47], 2)
        st.redraw()
        n_now = st.tile_frames()
        assert n_now.min() == 5 and n_now.max() == 7
        got = st.render_planned(seq)
        want = ref.target(4, plan["k"], n_now)
        assert np.array_equal(got["k"], want) and (want != plan["k"]).any() and want.any()
        assert got["tile_frames"] == int(want.sum()) and got["tiles"] == int((want > 0).sum()) and got["frames"] == int(want.max())
        assert got["planned_tile_frames"] == plan["tile_frames"]
        assert _f64(got["var_before"]) == _f64(plan["var_before"]) and _f64(got["var_after"]) == _f64(plan["var_after"])
        st.sync()
        assert np.array_equal(st.tile_frames(), np.maximum(n_now, 4 + plan["k"]))
        done = st.frames_done
        again = st.render_planned(seq)                     # the plan is met: nothing to render
        assert again["used_seq"] == seq and again["tile_frames"] == 0 and not again["k"].any() and st.frames_done == done


@pytest.mark.parametrize("max_w", [1.0, 0.9])
def test_the_query_grows_the_k_table_with_frames_in_flight(mrt, max_w):
    """n_t of 4,060 .. 4,100 and max_frames 32: n + j + 1 passes the 4,096 entries the first query made, so the query replaces the
    table -- behind its bounded wait, with two frames queued and not waited for.  The plan is the host's on the map the query left
    and on the n it saw (the loaded counts + 2)."""
    w, h = 24, 16
    rng = np.random.default_rng(31)
    loaded = rng.integers(4060, 4101, 6).astype(np.uint32)
    with _state(mrt, w, h, max_w) as st:
        st.render(3)
        st.noise_query(0.3, 0.02, budget=5, max_frames=4)                          # the table's first 4,096 entries
        st.debug_load_accumulation(np.ones((h, w, 4), np.float32), _s_pixels("random", h, w, rng), loaded)
        st.render(2)                                                               # (no sync)
        st.noise_query(0.3, 0.02, budget=70, max_frames=32)
        seq = _raw_report(mrt, st).seq
        assert seq == 2
        got, s_map = st.budget_plan(seq), st.read_noise_tiles()
        n_seen = (loaded + 2).reshape(s_map.shape)
        assert np.array_equal(st.tile_frames(), n_seen)
        k, want = mrt.State.budget_allocate(s_map, n_seen, max_w, 70, 32)
        assert np.array_equal(got["k"], k), (got["k"], k)
        for f in ("tile_frames", "tiles", "frames"):
            assert got[f] == want[f], (f, got[f], want[f])
        assert (want["tile_frames"] == 70) == (max_w == 1.0)                       # (at 0.9 K has stopped falling: no gains)
        before, after = ref.blocked_sums(s_map, n_seen, k, max_w)
        assert _f64(got["var_before"]) == _f64(before) and _f64(got["var_after"]) == _f64(after), (got, before, after)
        assert st.debug_check_context() is None


def test_mandatory_frames_come_first_and_alone(mrt):
    n = np.array([0, 1, 5, 0, 1, 5], np.uint32)
    with _state(mrt, 24, 16) as st:
        rng = np.random.default_rng(2)
        st.debug_load_accumulation(np.ones((16, 24, 4), np.float32), rng.uniform(0.5, 2.0, (16, 24)).astype(np.float32), n)
        for budget, want in ((3, [1, 1, 0, 1, 0, 0]), (5, [2, 1, 0, 1, 1, 0]), (6, [2, 1, 0, 2, 1, 0])):     # the demand is 6
            st.noise_query(budget=budget, max_frames=4)
            got = st.budget_plan(st.noise_result(wait=True)["seq"])
            assert got["k"].ravel().tolist() == want and got["tile_frames"] == budget
        got = st.render_planned(1)
        st.sync()
        assert got["k"].ravel().tolist() == [1, 1, 0, 1, 0, 0] and st.tile_frames().ravel().tolist() == [1, 2, 5, 1, 1, 5]


def _refused(mrt, status, call, *args, **kw):
    with pytest.raises(mrt.MrtError) as e:
        call(*args, **kw)
    assert e.value.status == status, e.value


def test_refusals_leave_everything_as_it_was(mrt):
    """mrt_noise_query_map's refusals, max_frames outside 1 .. 32, a shard; the readers' refusals.  (The refusal of an n_t above
    2^24 cannot be reached here: mrt_debug_load_accumulation takes counts below 2^20 and no test renders 2^24 frames; the check is
    shared with mrt_debug_budget_plan, where tests/test_gpu_budget_select.py reaches it.)"""
    with _state(mrt, 24, 16, tracking=False) as st:
        _refused(mrt, MRT_ERR_STATE, st.noise_query, budget=10, max_frames=4)
        _refused(mrt, MRT_ERR_STATE, st.budget_plan)
        _refused(mrt, MRT_ERR_STATE, st.render_planned)
    with _state(mrt, 24, 16, shard=(0, 2)) as st:
        st.render(2)
        _refused(mrt, MRT_ERR_STATE, st.noise_query, budget=10, max_frames=4)
        assert st.noise_result(wait=False) is None
    with _state(mrt, 24, 16) as st:
        st.render(3)
        st.sync()
        fb, S = st.read_framebuffer(), st.read_noise()
        for bad in (0, 33):
            _refused(mrt, MRT_ERR_INVALID_ARG, st.noise_query, budget=10, max_frames=bad)
        _refused(mrt, MRT_ERR_INVALID_ARG, st.noise_query, float("nan"), 0.01, budget=10, max_frames=4)
        _refused(mrt, MRT_ERR_INVALID_ARG, st.noise_query, 0.02, -1.0, budget=10, max_frames=4)
        assert st.noise_result(wait=False) is None and st.frames_done == 3      # nothing was queued
        assert st.budget_plan()["used_seq"] == 0 and st.render_planned()["used_seq"] == 0 and st.frames_done == 3
        st.noise_query(tile_map="sum_s")                   # report 1: no plan
        st.noise_query(budget=10, max_frames=4)            # report 2
        assert st.noise_result(wait=True)["seq"] == 2
        _refused(mrt, MRT_ERR_STATE, st.budget_plan, 1)
        _refused(mrt, MRT_ERR_STATE, st.render_planned, 1)
        _refused(mrt, MRT_ERR_STATE, st.budget_plan, 3)    # not queued
        r = mrt._lib.MrtBudgetResult()
        small = np.zeros(5, np.uint32)
        assert st._L.mrt_read_budget_plan(st._ctx, 2, small.ctypes.data, small.size, C.byref(r)) == MRT_ERR_TOO_SMALL
        assert st._L.mrt_render_planned(st._ctx, 2, C.byref(r), small.ctypes.data, small.size) == MRT_ERR_TOO_SMALL
        assert st.budget_plan(0)["used_seq"] == 2 and st.frames_done == 3
        st.sync()
        assert np.array_equal(_bits(fb), _bits(st.read_framebuffer())) and np.array_equal(_bits(S), _bits(st.read_noise()))
        # mrt_render_budget still takes a report that carries a plan, named or as the newest
        assert st.render_budget(10, 4)["used_seq"] == 2 and st.frames_done > 3
    with _state(mrt, 24, 16, scene=None) as st:
        _refused(mrt, 4, st.render_planned)                # MRT_ERR_NO_SCENE, before anything else is looked at


def test_a_plan_does_not_survive_a_reset_and_the_ring_holds_eight(mrt):
    with _state(mrt, 24, 16) as st:
        st.render(3)
        st.noise_query(budget=10, max_frames=4)
        assert st.budget_plan(1)["tile_frames"] == 10
        st.reset()
        _refused(mrt, MRT_ERR_STATE, st.budget_plan, 1)
        assert st.budget_plan()["used_seq"] == 0
        st.render(3)
        for i in range(9):                                  # reports 2 .. 10: the ninth takes report 2's entry
            st.noise_query(budget=i + 1, max_frames=4)
        s_map = st.read_noise_tiles()
        _refused(mrt, MRT_ERR_STATE, st.budget_plan, 2)
        for i in range(1, 9):
            got = st.budget_plan(i + 2)
            k, want = mrt.State.budget_allocate(s_map, np.full(s_map.shape, 3, np.uint32), 1.0, i + 1, 4)
            assert got["used_seq"] == i + 2 and np.array_equal(got["k"], k) and got["tile_frames"] == want["tile_frames"] == i + 1


def test_render_until_with_a_device_plan_is_deterministic_and_adapts(mrt):
    runs = []
    tiles = 48
    for _ in range(2):
        with _state(mrt, 64, 48, seed=21, scene="cover", tracking=False, spp=2, depth=6) as st:
            frames, rep = st.render_until(0.0, 30, check_every=4, threshold=0.1, floor=0.05, budget=2 * tiles, plan="device")
            st.sync()
            runs.append((frames, rep["seq"], st.read_framebuffer(), st.tile_frames()))
    (f0, q0, fb0, t0), (f1, q1, fb1, t1) = runs
    assert f0 == f1 and q0 == q1 and np.array_equal(t0, t1) and np.array_equal(_bits(fb0), _bits(fb1))
    assert f0 >= 30                                         # the target 0 is never met: it ends at max_frames
    assert t0.min() >= 8 and t0.min() < t0.max()            # two uniform chunks, then the plans' choice: diverged
