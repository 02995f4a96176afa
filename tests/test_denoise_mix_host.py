"""The denoiser's blend with the accumulation on the host (include/myraytracer_amd.h, "Blend with the accumulation"): the float32
restatement (tests/denoise_mix_ref.py, which the GPU tests compare the device against bit for bit) against the references it is
built on, against a plain float64 form of the same definition and on the cases the definition singles out; two definitions
broken on purpose; the setting's checks that need no context; and what the blend buys on the cover scene at 32 and 64 frames."""
import ctypes as C
import math

import numpy as np
import pytest

from myraytracer_amd import _lib, api
from denoise_mix_ref import (blend, blend_f64, denoise_mix, denoise_mix_tiles, filtered, filtered_tiles, quality_figures_host)
from denoise_ref import denoise, lum, random_case
from denoise_tiles_ref import denoise_tiles, tile_map
from denoise_var_ref import denoise_var

MRT_OK, MRT_ERR_INVALID_ARG = 0, 1
F = np.float32
OTHER = {"sigma_l": 2.5, "normal_exp": 3, "sigma_z": 0.4, "sigma_a": 0.25}
K_OF = lambda n: math.inf if n < 2 else 1.0 / (n - 1)          # (a table of its own: no library call needed for the tile cases)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("K", [0.2, math.inf])
@pytest.mark.parametrize("variance", [0, 1, 2])
def test_the_restated_iterations_are_the_references(K, variance):
    rgba, S, guides = random_case(np.random.default_rng(4 + variance), 21, 26)
    for params in ({}, OTHER):
        for it in (1, 2, 5):
            p = dict(params, iterations=it)
            fu = filtered(rgba, S, K, guides, p, variance)
            assert fu.dtype == np.float32
            assert np.array_equal(_bits(fu[..., :3]), _bits(denoise_var(rgba, S, K, guides, p, variance)[..., :3]))
            if variance == 0:
                assert np.array_equal(_bits(fu[..., :3]), _bits(denoise(rgba, S, K, guides, p)[..., :3]))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_restated_iterations_are_the_tile_reference(mode):
    rng = np.random.default_rng(40 + mode)
    rgba, S, guides = random_case(rng, 21, 26)
    tiles = tile_map(rng, 21, 26, [0, 1, 2, 3, 4, 40])
    for it in (1, 4):
        fu, K = filtered_tiles(rgba, S, tiles, guides, {"iterations": it}, mode, 4, K_OF)
        want = denoise_tiles(rgba, S, tiles, guides, {"iterations": it}, mode, 4, K_OF)
        assert np.array_equal(_bits(fu[..., :3]), _bits(want[..., :3]))
        assert np.isinf(K).any() and np.isfinite(K).any()


# The float32 form against the float64 one.  Both read the same float32 c, S, f and u; the float32 form rounds d (3 operations on
# luminances below 1, so |error| <= 4 * 2^-24), d^2, v, n and the 25-term sums: a relative error of at most ~60 * 2^-24 = 4e-6 in
# a where nothing cancels, times |f - c| <= 1, and the final multiply and add.  2e-5 leaves a factor of 5 for the cancellation in
# d and in v - u of single taps, which the sums over the window dilute.
@pytest.mark.parametrize("variance", [0, 1, 2])
@pytest.mark.parametrize("rows,width", [(13, 17), (2, 3), (1, 1), (4, 2)])
def test_float32_form_matches_float64(variance, rows, width):
    rng = np.random.default_rng(100 * variance + rows * width)
    rgba, S, guides = random_case(rng, rows, width, nonfinite=rows >= 3 and width >= 3, zero_var=rows >= 3 and width >= 3)
    for gain in (0.25, 2.0, 16.0):
        fu = filtered(rgba, S, 1.0 / 7.0, guides, {"iterations": 2}, variance)
        got = blend(rgba, S, fu, 1.0 / 7.0, guides["index"], gain)
        ref = blend_f64(rgba, S, fu, 1.0 / 7.0, guides["index"], gain)
        assert got.dtype == np.float32
        assert np.array_equal(np.isfinite(got), np.isfinite(ref))
        fin = np.isfinite(ref)
        np.testing.assert_allclose(got[fin], ref[fin], rtol=0, atol=2e-5)
        assert np.array_equal(_bits(got[..., 3]), _bits(rgba[..., 3]))
        # out lies between c and f per channel, up to the rounding of c + a (f - c): one ulp of the larger of the two
        c, f = rgba[..., :3], fu[..., :3]
        ok = np.isfinite(c).all(-1) & np.isfinite(f).all(-1)
        lo, hi = np.minimum(c, f)[ok], np.maximum(c, f)[ok]
        slack = np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(F))
        assert (got[..., :3][ok] >= lo - slack).all() and (got[..., :3][ok] <= hi + slack).all()


def test_without_an_estimate_the_image_is_the_filters():
    rgba, S, guides = random_case(np.random.default_rng(9), 14, 19)
    for variance in (0, 1, 2):
        got = denoise_mix(rgba, S, math.inf, guides, None, variance)
        assert np.array_equal(_bits(got), _bits(denoise_var(rgba, S, math.inf, guides, None, variance)))
    # a tile without an estimate inside an adaptive accumulation: its pixels are not valid, as centres and as taps
    tiles = np.array([[5, 1, 5], [5, 5, 0]], np.uint32)
    fu, K = filtered_tiles(rgba, S, tiles, guides, None, 0, 3, K_OF)
    got = denoise_mix_tiles(rgba, S, tiles, guides, None, 0, 3, K_OF)
    none = np.isinf(K)
    assert none[:8, 8:16].all() and none[8:, 16:].all() and none.sum() == 8 * 8 + 6 * 3
    assert np.array_equal(_bits(got[none][:, :3]), _bits(fu[none][:, :3]))
    assert np.array_equal(_bits(got[..., 3]), _bits(rgba[..., 3]))
    other = blend(rgba, S, fu, np.where(none, F(1), K), guides["index"], 2.0)       # (the same with those tiles counted)
    assert not np.array_equal(_bits(got[~none]), _bits(other[~none]))


def test_non_finite_and_zero_variance_texels_pass_through():
    rgba, S, guides = random_case(np.random.default_rng(3), 16, 24)
    for it in (1, 3):
        got = denoise_mix(rgba, S, 0.2, guides, {"iterations": it}, 0)
        want = denoise(rgba, S, 0.2, guides, {"iterations": it})
        for y, x in ((1, 2), (8, 23), (0, 12), (15, 0)):            # NaN / Inf in the colour or in S: the filter's texel, which is c
            assert np.array_equal(_bits(got[y, x]), _bits(want[y, x])) and np.array_equal(_bits(got[y, x]), _bits(rgba[y, x]))
        for y, x in ((8, 8), (2, 1)):                               # S = 0: f = c, so d = 0 and the blend returns c
            assert np.array_equal(_bits(got[y, x]), _bits(rgba[y, x]))
        assert not np.array_equal(_bits(got), _bits(want))


def _synthetic(rng, rows, width):
    rgba = rng.uniform(0.1, 0.9, (rows, width, 4)).astype(F)
    fu = np.empty_like(rgba)
    fu[..., :3] = rgba[..., :3] + rng.uniform(-0.05, 0.05, (rows, width, 3)).astype(F)
    S = rng.uniform(0.01, 0.02, (rows, width)).astype(F)
    fu[..., 3] = rng.uniform(0.0, 0.004, (rows, width)).astype(F)
    return rgba, S, fu, np.zeros((rows, width), np.int32)


def _by_hand(rgba, S, fu, K, taps, p, gain):
    """The definition for one pixel from an explicit list of counted taps, float32, in the order given."""
    e = m = F(0)
    for y, x in taps:
        d = lum(fu[y, x]) - lum(rgba[y, x])
        e = e + d * d
        m = m + np.fmax(S[y, x] * F(K) - fu[y, x, 3], F(0))
    a = np.fmin(m / (F(gain) * e), F(1)) if e > 0 else F(0)
    c, f = rgba[p][:3], fu[p][:3]
    return (c + a * (f - c)).astype(F)


def test_every_way_a_tap_is_refused():
    rng = np.random.default_rng(12)
    rgba, S, fu, index = _synthetic(rng, 7, 7)
    K, gain, p = 0.25, 4.0, (3, 3)
    window = [(y, x) for y in range(1, 6) for x in range(1, 6)]
    full = blend(rgba, S, fu, K, index, gain)
    assert np.array_equal(_bits(full[p][:3]), _bits(_by_hand(rgba, S, fu, K, window, p, gain)))
    a_full = (full[p][0] - rgba[p][0]) / (fu[p][0] - rgba[p][0])
    assert 0.05 < a_full < 0.95                                     # (neither end: every tap's share shows)
    refused = []
    for why, (y, x) in (("c", (1, 1)), ("S", (1, 4)), ("f", (2, 5)), ("u", (3, 1)), ("index", (4, 2)), ("K", (5, 5))):
        if why == "c":
            rgba[y, x, 1] = np.nan
        elif why == "S":
            S[y, x] = np.inf
        elif why == "f":
            fu[y, x, 2] = -np.inf
        elif why == "u":
            fu[y, x, 3] = np.nan
        elif why == "index":
            index[y, x] = 3
        Kp = np.full((7, 7), K, F)
        if why == "K":
            Kp[y, x] = np.inf
        refused.append((y, x))
        before = full
        full = blend(rgba, S, fu, Kp, index, gain)
        want = _by_hand(rgba, S, fu, K, [t for t in window if t not in refused], p, gain)
        assert np.array_equal(_bits(full[p][:3]), _bits(want)), why
        assert not np.array_equal(_bits(full[p]), _bits(before[p])), why
    # the index rule is symmetric and exact: the odd pixel's own window holds itself alone
    q = (4, 2)
    assert np.array_equal(_bits(full[q][:3]), _bits(_by_hand(rgba, S, fu, K, [q], q, gain)))
    # taps outside the image: a corner's window is the 3 x 3 pixels that exist
    corner = [(y, x) for y in range(4, 7) for x in range(4, 7) if (y, x) not in refused]
    assert np.array_equal(_bits(full[6, 6][:3]), _bits(_by_hand(rgba, S, fu, K, corner, (6, 6), gain)))
    # e == 0: a = 0, the accumulated texel
    fu2 = fu.copy()
    fu2[..., :3] = rgba[..., :3]
    fu2[~np.isfinite(fu).all(-1)] = fu[~np.isfinite(fu).all(-1)]
    assert np.array_equal(_bits(blend(rgba, S, fu2, K, index, gain)[p]), _bits(rgba[p]))


def test_a_window_larger_than_the_image():
    rng = np.random.default_rng(5)
    for rows, width in ((1, 1), (2, 3), (1, 4), (5, 1)):
        rgba, S, fu, index = _synthetic(rng, rows, width)
        got = blend(rgba, S, fu, 0.25, index, 2.0)
        everything = [(y, x) for y in range(rows) for x in range(width) if True]
        for p in everything:
            taps = [(y, x) for (y, x) in everything if abs(y - p[0]) <= 2 and abs(x - p[1]) <= 2]
            assert np.array_equal(_bits(got[p][:3]), _bits(_by_hand(rgba, S, fu, 0.25, taps, p, 2.0))), (rows, width, p)


def test_two_broken_definitions_are_rejected():
    rgba, S, guides = random_case(np.random.default_rng(21), 19, 33)
    right = denoise_mix(rgba, S, 0.2, guides, None, 0, gain=2.0)
    ref = blend_f64(rgba, S, filtered(rgba, S, 0.2, guides), 0.2, guides["index"], 2.0)
    fin = np.isfinite(ref)
    # v + u in the place of v - u: beyond the float64 form's tolerance, not only in the bits
    plus = denoise_mix(rgba, S, 0.2, guides, None, 0, gain=2.0, broken="v_plus_u")
    assert np.abs(plus[fin] - ref[fin]).max() > 1e-3 >= 2e-5 > np.abs(right[fin] - ref[fin]).max()
    # the window dx then dy: the same sums in another order -- within the tolerance, so only the bits tell
    order = denoise_mix(rgba, S, 0.2, guides, None, 0, gain=2.0, broken="dx_then_dy")
    assert np.abs(order[fin] - ref[fin]).max() < 2e-5
    assert not np.array_equal(_bits(order), _bits(right))


def test_the_setting_and_null_context():
    L = _lib.load()
    assert C.sizeof(_lib.MrtDenoiseMix) == 32
    for name in ("mrt_denoise_mix_default", "mrt_set_denoise_mix", "mrt_get_denoise_mix", "mrt_debug_denoise_mix"):
        assert name in _lib.EXPORTS
    d = api.denoise_mix_default()
    assert d["enabled"] == 0 and 0.25 <= d["gain"] <= 16.0
    profile = open(__file__.rsplit("/tests/", 1)[0] + "/profiles/denoise_mix_quality.txt").read()
    assert f"chosen default gain: {d['gain']:g} " in profile + " "      # the header cites the file; the file names the value
    p = _lib.MrtDenoiseMix()
    L.mrt_denoise_mix_default(C.byref(p))
    assert p.size == 32 and p.enabled == 0 and list(p.reserved) == [0] * 5
    assert L.mrt_set_denoise_mix(None, C.byref(p)) == MRT_OK           # ctx NULL: the setting alone
    assert L.mrt_set_denoise_mix(None, None) == MRT_ERR_INVALID_ARG
    assert L.mrt_get_denoise_mix(None, C.byref(p)) == MRT_ERR_INVALID_ARG
    L.mrt_denoise_mix_default(None)                                    # (tolerated, as its siblings tolerate it)

    def with_(**kw):
        q = _lib.MrtDenoiseMix()
        L.mrt_denoise_mix_default(C.byref(q))
        for k, v in kw.items():
            if k == "reserved":
                q.reserved[v] = 1
            else:
                setattr(q, k, v)
        return L.mrt_set_denoise_mix(None, C.byref(q))
    for ok in ({"enabled": 0}, {"enabled": 1}, {"gain": 0.25}, {"gain": 16.0}, {"gain": 1.0}):
        assert with_(**ok) == MRT_OK, ok
    for bad in ({"enabled": 2}, {"gain": float(np.nextafter(F(0.25), F(0)))}, {"gain": float(np.nextafter(F(16), F(17)))}, {"gain": 0.0},
                {"gain": -1.0}, {"gain": float("nan")}, {"gain": float("inf")}, {"size": 28}, {"size": 36},
                *({"reserved": i} for i in range(5))):
        assert with_(**bad) == MRT_ERR_INVALID_ARG, bad
    assert L.mrt_debug_denoise_mix(None, None, None, 0.0, None, 0, 0, None, 0, None, None) == MRT_ERR_INVALID_ARG


# What the blend buys (profiles/denoise_mix_quality.txt has the whole table at 320x192): on the cover scene at 160x96, against 512
# frames of another seed, the blend at the default gain is better than both the noisy and the denoised image at 32 and at 64
# frames.  The bound is the issue's: below both; the margin measured at this size is printed.
def test_the_blend_beats_both_images_at_32_and_64_frames(oracle, mrt):
    for n, (noisy, den, mix) in quality_figures_host(oracle, mrt).items():
        print(f"{n} frames: noisy {noisy:.5f}  denoised {den:.5f}  blend {mix:.5f}  ({mix / min(noisy, den):.3f} x the better one)")
    for n, (noisy, den, mix) in quality_figures_host(oracle, mrt).items():
        assert mix < noisy and mix < den, (n, noisy, den, mix)
