"""Adaptive sampling by budget, host side (no GPU): mrt_budget_allocate against the numpy float64 restatement
(tests/budget_ref.py) bit for bit, on random maps and on built cases; what the allocation promises (it never overspends, and its
modelled variance is no larger than that of other ways to spend the same budget); its refusals; the reference's own summation
order; the new symbols' bindings."""
import inspect
import math
import os

import numpy as np
import pytest

import budget_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MRT_ERR_INVALID_ARG = 1


def _same(mrt, s, n, max_w, budget, max_frames):
    """the library's allocation, after holding it against the restatement: k, and the result's every field, bit for bit"""
    k, res = mrt.State.budget_allocate(s, n, max_w, budget, max_frames)
    k_want, want = budget_ref.allocate(s, n, max_w, budget, max_frames)
    assert np.array_equal(k, k_want), (k, k_want)
    assert res["used_seq"] == 0
    for f in ("tile_frames", "tiles", "frames"):
        assert res[f] == want[f], f
    for f in ("var_before", "var_after"):
        assert np.float64(res[f]).view(np.uint64) == np.float64(want[f]).view(np.uint64), (f, res[f], want[f])
    assert res["tile_frames"] <= budget and k.max(initial=0) <= max_frames
    return k, res


@pytest.mark.parametrize("max_w", [1.0, 0.9, 0.75])
@pytest.mark.parametrize("max_frames", [1, 4, 32])
def test_random_maps_match_the_restatement(mrt, max_w, max_frames):
    rng = np.random.default_rng(int(max_w * 100) * 64 + max_frames)
    for case in range(6):
        tiles = int(rng.integers(1, 200))
        s = (rng.uniform(0.0, 2.0, tiles) * np.exp2(rng.integers(-12, 6, tiles))).astype(np.float32)
        s[rng.random(tiles) < 0.1] = 0
        n = rng.integers(0 if case % 2 else 2, 60, tiles).astype(np.uint32)
        for budget in (0, 1, tiles // 2, 3 * tiles, tiles * max_frames + 5):
            _same(mrt, s, n, max_w, budget, max_frames)


def test_ties_go_to_the_earlier_frame_then_the_lower_tile(mrt):
    s = np.array([1, 2, 1, 2, 1, 2, 2], np.float32)         # equal maps at equal counts: equal gains
    n = np.full(7, 5, np.uint32)
    for budget in range(0, 16):
        k, _ = _same(mrt, s, n, 1.0, budget, 2)
    k, _ = _same(mrt, s, n, 1.0, 3, 2)
    assert k.tolist() == [0, 1, 0, 1, 0, 1, 0]              # the four 2s tie at j = 0: t ascending
    # a tie across j goes to the smaller j: tile 0's second frame and tile 1's first are both 1 * (K(6) - K(7))
    k, _ = _same(mrt, np.ones(2, np.float32), np.array([5, 6], np.uint32), 1.0, 2, 2)
    assert k.tolist() == [1, 1]


def test_tiles_without_an_estimate_come_first(mrt):
    n = np.array([5, 0, 1, 5, 0, 1, 7], np.uint32)
    s = np.array([9, 0, 3, 1, np.nan, np.inf, 2], np.float32)
    # the mandatory demand is 6: j = 0 over tiles 1, 2, 4, 5, then j = 1 over tiles 1, 4
    want = [[0, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0, 0], [0, 1, 1, 0, 1, 0, 0], [0, 1, 1, 0, 1, 1, 0],
            [0, 2, 1, 0, 1, 1, 0], [0, 2, 1, 0, 2, 1, 0]]
    for budget, kw in enumerate(want):
        k, res = _same(mrt, s, n, 1.0, budget, 4)
        assert k.tolist() == kw
    k, _ = _same(mrt, s, n, 1.0, 7, 4)
    assert k.tolist() == [0, 2, 2, 0, 2, 1, 0]              # the first frame with a gain: 3 (K(2) - K(3)) = 1.5 beats 9 (K(5) - K(6)) = 0.45
    k, _ = _same(mrt, s, n, 1.0, 100, 4)
    assert k.tolist() == [4, 2, 4, 4, 2, 1, 4]              # s 0, NaN and inf: the mandatory frames and no more
    k, _ = _same(mrt, s, n, 1.0, 100, 1)                    # max_frames 1: a tile at 0 frames stays without an estimate
    assert k.tolist() == [1, 1, 1, 1, 1, 1, 1]
    k, res = _same(mrt, np.array([1, 1], np.float32), np.array([0, 0], np.uint32), 1.0, 10, 1)
    assert k.tolist() == [1, 1] and res["var_before"] == 0.0 and res["var_after"] == 0.0


def test_values_that_are_no_variance(mrt):
    n = np.full(6, 4, np.uint32)
    s = np.array([0, np.nan, np.inf, -1, -np.inf, 1], np.float32)
    k, res = _same(mrt, s, n, 1.0, 50, 8)
    assert k.tolist() == [0, 0, 0, 0, 0, 8]
    assert math.isinf(res["var_before"]) and math.isinf(res["var_after"])          # (the +inf tile is in both sums)
    k, res = _same(mrt, np.zeros(5, np.float32), n[:5], 1.0, 50, 8)
    assert not k.any() and res["tile_frames"] == 0 and res["frames"] == 0


def test_a_budget_larger_than_every_gain_and_a_saturated_weight(mrt):
    rng = np.random.default_rng(4)
    s = rng.uniform(0.1, 3.0, 40).astype(np.float32)
    n = rng.integers(2, 30, 40).astype(np.uint32)
    k, res = _same(mrt, s, n, 1.0, 10 ** 12, 32)
    assert (k == 32).all() and res["tile_frames"] == 40 * 32
    # max_w 0.9: the EMA's K reaches its fixed point, the gains reach 0 and the rest of the budget stays unspent
    K = budget_ref.k_values(600, 0.9)
    first_flat = int(np.nonzero(np.diff(K[2:]) == 0)[0][0]) + 2
    assert first_flat < 500
    n = np.array([2, 10, first_flat - 3, first_flat, first_flat + 40], np.uint32)
    k, res = _same(mrt, np.ones(5, np.float32), n, 0.9, 10 ** 6, 32)
    assert k[3] == 0 and k[4] == 0 and 0 < k[2] <= 3 and res["tile_frames"] < 5 * 32
    assert res["var_after"] < res["var_before"]


@pytest.mark.parametrize("max_w", [1.0, 0.75])
def test_no_other_way_to_spend_the_budget_models_less_variance(mrt, max_w):
    """Against an even spread, the threshold rule's list (the tiles with the largest modelled variance, `frames` frames each) and
    a random allocation, all within the same budget and max_frames.  In exact arithmetic K(n) - K(n + 1) falls with n, so taking
    the largest gains first is optimal; the sums here have <= 150 terms of float64, so 1e-12 relative covers their rounding."""
    rng = np.random.default_rng(12)
    M = 8
    for _ in range(5):
        tiles = int(rng.integers(20, 150))
        s = (rng.uniform(0.5, 2.0, tiles) * np.exp2(rng.integers(-6, 6, tiles))).astype(np.float32)
        n = rng.integers(2, 40, tiles).astype(np.uint32)
        for budget in (tiles // 3, tiles, 3 * tiles):
            k, res = _same(mrt, s, n, max_w, budget, M)
            assert res["var_after"] == budget_ref.var_after(s, n, k, max_w)
            even = np.full(tiles, min(budget // tiles, M))
            if budget // tiles < M:
                even[:budget % tiles] += 1
            frames = 4
            K = budget_ref.k_values(int(n.max()), max_w)
            listed = np.argsort(-(s.astype(np.float64) * K[n]), kind="stable")[:budget // frames]
            thresh = np.zeros(tiles, np.int64)
            thresh[listed] = frames
            rand = np.zeros(tiles, np.int64)
            for t in rng.integers(0, tiles, budget):
                rand[t] += rand[t] < M
            for name, other in (("even", even), ("threshold", thresh), ("random", rand)):
                assert other.sum() <= budget and other.max() <= M, name
                assert res["var_after"] <= budget_ref.var_after(s, n, other, max_w) * (1 + 1e-12), (name, budget)


def test_refusals_write_nothing(mrt):
    L = mrt._lib.load()
    s, n = np.ones(4, np.float32), np.full(4, 3, np.uint32)
    k = np.full(4, 77, np.uint32)
    r = mrt._lib.MrtBudgetResult()
    r.tiles = 55
    sp, np_, kp = s.ctypes.data, n.ctypes.data, k.ctypes.data
    import ctypes as C
    for args in ((None, np_, 4, 1.0, 8, 4, kp, C.byref(r)), (sp, None, 4, 1.0, 8, 4, kp, C.byref(r)), (sp, np_, 4, 1.0, 8, 4, None, C.byref(r)),
                 (sp, np_, 4, 1.0, 8, 4, kp, None), (sp, np_, 0, 1.0, 8, 4, kp, C.byref(r)), (sp, np_, 4, 1.0, 8, 0, kp, C.byref(r)),
                 (sp, np_, 4, 1.0, 8, 33, kp, C.byref(r)), (sp, np_, 4, 0.0, 8, 4, kp, C.byref(r)), (sp, np_, 4, float("nan"), 8, 4, kp, C.byref(r))):
        assert L.mrt_budget_allocate(*args) == MRT_ERR_INVALID_ARG, args
    big = np.array([3, 3, 2 ** 24 + 1, 3], np.uint32)
    assert L.mrt_budget_allocate(sp, big.ctypes.data, 4, 1.0, 8, 4, kp, C.byref(r)) == MRT_ERR_INVALID_ARG
    assert (k == 77).all() and r.tiles == 55 and r.size == 0
    assert L.mrt_budget_allocate(sp, np_, 4, 1.0, 8, 4, kp, C.byref(r)) == 0
    assert r.size == C.sizeof(mrt._lib.MrtBudgetResult) == 64 and k.sum() == 8


def test_the_map_fixture_tells_the_summation_orders_apart():
    """the reference's own statement of the order: on the fixture of the GPU test (tests/test_gpu_adaptive_budget.py) the tree over
    the columns and the rows from the bottom give another float than 64 additions in row-major order for at least one tile"""
    S, rgba = budget_ref.map_fixture()
    want, other = budget_ref.tile_sums(S, rgba), budget_ref.tile_sums_row_major(S, rgba).reshape(3, 6)
    assert want.shape == (3, 6) and np.isfinite(want).all()
    assert (want.view(np.uint32) != other.view(np.uint32)).sum() >= 1
    # a pixel that is not counted adds nothing: the tiles of the NaN / inf S and of the non-finite colour are finite sums of the rest
    S2 = S.copy()
    S2[~np.isfinite(S)] = 0
    S2[6, 30] = 0
    rgba2 = rgba.copy()
    rgba2[6, 30, 1] = 1
    assert np.array_equal(budget_ref.tile_sums(S2, rgba2).view(np.uint32), want.view(np.uint32))


def test_levels_merge_equal_lists():
    lv = budget_ref.levels(np.array([3, 0, 3, 1, 3]))
    assert [(l.tolist(), r) for l, r in lv] == [([0, 2, 3, 4], 1), ([0, 2, 4], 2)]
    assert budget_ref.levels(np.zeros(4)) == []


def test_budget_symbols_are_bound(mrt):
    L = mrt._lib.load()
    header = open(os.path.join(ROOT, "include", "myraytracer_amd.h")).read()
    for name in ("mrt_noise_query_map", "mrt_budget_allocate", "mrt_render_budget"):
        assert name in mrt._lib.EXPORTS and name + "(" in header
        assert getattr(L, name).argtypes is not None
    assert "MRT_TILE_MAP_MAX_REL = 0, MRT_TILE_MAP_SUM_S = 1" in header
    st = mrt.State
    assert callable(st.render_budget) and callable(st.budget_allocate)
    assert inspect.signature(st.render_until).parameters["budget"].default is None
    assert inspect.signature(st.noise_query).parameters["tile_map"].default == "max_rel"
    assert inspect.signature(st.render_budget).parameters["max_frames"].default == 8
