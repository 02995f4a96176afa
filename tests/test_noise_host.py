"""The noise estimate's host side (no GPU): mrt_noise_factor against a brute-force recursion over mrt_frame_weight, the float32
reference (tests/noise_ref.py) against a float64 weighted variance, dist.combine_noise_reports, and the new symbols' bindings."""
import math

import numpy as np
import pytest

import noise_ref


def _brute_factors(L, max_w, n):
    out, c2 = [], 1.0
    for k in range(n + 1):
        out.append(math.inf if c2 >= 1.0 else c2 / (1.0 - c2))
        w = float(np.float32(L.mrt_frame_weight(k, max_w)))
        c2 = 1.0 if w == 0.0 else w * w * c2 + (1.0 - w) * (1.0 - w)
    return out


@pytest.mark.parametrize("max_w", [1.0, 0.9, 0.5])
def test_noise_factor_is_the_weight_recursion(mrt, max_w):
    L = mrt._lib.load()
    want = _brute_factors(L, max_w, 10_000)
    for n in list(range(0, 40)) + list(range(40, 10_001, 97)) + [10_000]:
        got = L.mrt_noise_factor(n, max_w)
        if n < 2:
            assert math.isinf(got) and got > 0, (n, got)
        else:
            assert abs(got - want[n]) <= 1e-12 * abs(want[n]), (n, got, want[n])
    assert mrt.noise_factor(5, max_w) == L.mrt_noise_factor(5, max_w)


def test_noise_factor_limits(mrt):
    L = mrt._lib.load()
    for n in (2, 3, 10, 100, 1000, 10_000):
        assert L.mrt_noise_factor(n, 1.0) == pytest.approx(1.0 / (n - 1), rel=1e-5)    # (float weights k / (k + 1))
    for w in (0.9, 0.5, 0.75):
        wf = float(np.float32(w))                                                       # (the weight as the blend uses it)
        assert L.mrt_noise_factor(100_000, w) == pytest.approx((1 - wf) / (2 * wf), rel=1e-9)
    assert math.isinf(L.mrt_noise_factor(50, 0.0))                                       # every frame replaces the image


@pytest.mark.parametrize("max_w", [1.0, 0.75])
def test_reference_recursion_is_the_weighted_variance(max_w):
    rng = np.random.default_rng(7)
    frames = 40
    means = [np.concatenate([rng.random((5, 7, 3), np.float32) * 3, np.ones((5, 7, 1), np.float32)], -1) for _ in range(frames)]
    weights = [float(np.float32(min(max_w, k / (k + 1)) if k else 0.0)) for k in range(frames)]
    fb, S, K = noise_ref.accumulate(means, weights)
    # the normalised weights of the frames in the final image, in float64
    c = np.zeros(frames)
    for k, w in enumerate(weights):
        c *= w
        c[k] = 1.0 - w
    lum = np.stack([noise_ref.lum(m).astype(np.float64) for m in means])             # (frames, H, W)
    mu = np.tensordot(c, lum, 1)
    var = np.tensordot(c, (lum - mu) ** 2, 1)
    assert np.allclose(S, var, rtol=2e-4, atol=1e-6)
    c2 = float((c * c).sum())
    assert K == pytest.approx(c2 / (1 - c2), rel=1e-6)
    assert np.allclose(noise_ref.lum(fb), mu, rtol=1e-5)


def _rep(frames_done=10, K=0.1, **kw):
    r = {"seq": 1, "frames_done": frames_done, "noise_factor": K, "threshold": 0.02, "floor": 0.01, "pixels": 100,
         "non_finite": 1, "above": 7, "sum_var": 1.5, "sum_lum": 40.0, "max_se": 0.25, "rmse": 0.0, "rel_rmse": 0.0}
    r.update(kw)
    return r


def test_combine_noise_reports():
    from myraytracer_amd import dist
    parts = [_rep(pixels=100, above=7, non_finite=1, sum_var=1.5, sum_lum=40.0, max_se=0.25),
             _rep(pixels=96, above=0, non_finite=0, sum_var=0.1 + 1e-9, sum_lum=12.5, max_se=0.75, seq=3),
             _rep(pixels=80, above=80, non_finite=5, sum_var=2.0 / 3.0, sum_lum=0.3, max_se=0.5)]
    r = dist.combine_noise_reports(parts)
    assert (r["pixels"], r["above"], r["non_finite"], r["max_se"], r["seq"]) == (276, 87, 6, 0.75, 3)
    sv, sl = 1.5 + 0.1 + 1e-9 + 2.0 / 3.0, 40.0 + 12.5 + 0.3
    assert abs(r["sum_var"] - sv) <= 1e-12 * sv and abs(r["sum_lum"] - sl) <= 1e-12 * sl
    assert abs(r["rmse"] - math.sqrt(sv / 276)) <= 1e-12 * r["rmse"]
    assert abs(r["rel_rmse"] - math.sqrt(sv / 276) / (sl / 276)) <= 1e-12 * r["rel_rmse"]
    with pytest.raises(ValueError):
        dist.combine_noise_reports([_rep(), _rep(K=0.2)])
    with pytest.raises(ValueError):
        dist.combine_noise_reports([_rep(), _rep(frames_done=11)])
    inf = dist.combine_noise_reports([_rep(K=math.inf), _rep(K=math.inf)])
    assert math.isinf(inf["rmse"]) and math.isinf(inf["rel_rmse"]) and math.isinf(inf["max_se"])


def test_noise_symbols_are_exported_and_bound(mrt):
    from myraytracer_amd import _lib
    L = _lib.load()
    for name in ("mrt_set_noise_tracking", "mrt_noise_query", "mrt_noise_result", "mrt_read_noise", "mrt_read_noise_tiles",
                 "mrt_noise_factor", "mrt_debug_noise_reduce"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert getattr(L, name).argtypes
    import ctypes as C
    assert C.sizeof(_lib.MrtNoiseReport) == 96 and _lib.MrtNoiseReport.max_se.offset == 88
    for name in ("set_noise_tracking", "noise_query", "noise_result", "read_noise", "read_noise_tiles", "render_until"):
        assert callable(getattr(mrt.State, name))


@pytest.mark.parametrize("height,world", [(1, 1), (27, 1), (27, 2), (43, 3), (60, 5), (9, 8)])
def test_shard_rows_are_mrt_shard_global_row(mrt, height, world):
    """The packing the shard references use is the library's own index math, and every image row lands in exactly one shard."""
    seen = []
    full = np.arange(height * 3, dtype=np.float32).reshape(height, 3)
    for rank in range(world):
        g = noise_ref.shard_rows(height, rank, world)
        assert len(g) == mrt.shard_local_rows(height, world)
        want = np.array([mrt.shard_global_row(r, rank, world) for r in range(len(g))])
        assert np.array_equal(g, np.where(want < height, want, -1))
        seen += g[g >= 0].tolist()
        packed = noise_ref.pack_rows(full, rank, world)
        assert np.array_equal(packed[g >= 0], full[g[g >= 0]]) and not packed[g < 0].any()
    assert sorted(seen) == list(range(height))


def test_tile_map_skips_rows_marked_invalid():
    """K = +inf gives every finite pixel rel = +inf: a padding row must not put that into its tile."""
    S = np.zeros((16, 10), np.float32)
    rgba = np.ones((16, 10, 4), np.float32)
    valid = np.arange(16) < 8
    assert np.isinf(noise_ref.tiles(S, rgba, math.inf)).all()
    m = noise_ref.tiles(S, rgba, math.inf, valid=valid)
    assert np.isinf(m[0]).all() and (m[1] == 0).all()


@pytest.mark.parametrize("size", __import__("noise_cases").FORM_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_forms_references_agree_on_the_crafted_data(mrt, size):
    """What tests/test_gpu_noise_forms.py expects, checked without a GPU: at every size the per-tile reference with one count for
    every tile is the uniform reference, the specials all landed, a K = +inf tile shows in the map and in the report, and the
    summed-S map holds no K and tells its summation order from the row-major one."""
    import adaptive_ref
    import budget_ref
    import noise_cases
    w, h = size
    S, rgba = noise_cases.form_case(size)
    thr, fl = 0.05, 0.02
    uni = noise_cases.form_expected(size, "uniform", thr, fl)
    acc = adaptive_ref.Accum(h, w, noise_cases.FORM_MAX_W)
    acc.load(rgba, S, np.full(acc.n_tiles, 3))
    assert np.array_equal(acc.tiles(thr, fl).view(np.uint32), uni["max_rel"].view(np.uint32))
    noise_cases.check_report(acc.report(thr, fl), uni["report"])
    assert acc.report(thr, fl)["noise_factor"] == uni["report"]["noise_factor"] == mrt.noise_factor(3, 1.0)
    assert uni["report"]["non_finite"] == 6 and uni["report"]["pixels"] == w * h - 6 and uni["report"]["max_se"] > 1e19
    none = noise_cases.form_expected(size, "no-estimate", thr, fl)
    assert none["report"]["above"] == none["report"]["pixels"] and math.isinf(none["report"]["sum_var"])
    mixed, finite = (noise_cases.form_expected(size, f, thr, fl) for f in ("per-tile-inf", "per-tile"))
    assert math.isinf(mixed["report"]["noise_factor"]) and np.isinf(mixed["max_rel"].ravel()[0])
    assert finite["report"]["noise_factor"] == mrt.noise_factor(2, 1.0) and math.isfinite(finite["report"]["sum_var"])
    assert 0 < finite["report"]["above"] < finite["report"]["pixels"]
    for e in (none, mixed, finite):
        assert np.array_equal(e["sum_s"].view(np.uint32), uni["sum_s"].view(np.uint32))
        assert e["report"]["pixels"] == uni["report"]["pixels"] and e["report"]["sum_lum"] == uni["report"]["sum_lum"]
    if w * h >= 2048:
        assert not np.array_equal(uni["sum_s"], budget_ref.tile_sums_row_major(S, rgba))
