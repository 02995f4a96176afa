"""The denoiser's variance modes on the host (include/myraytracer_amd.h, "Variance modes"): the float32 restatement
(tests/denoise_var_ref.py, which the GPU tests compare the device against bit for bit) against denoise_ref for the default mode,
against a plain float64 form of the same definition, and on the cases the definition singles out; the setter's and getter's
checks that need no context."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from myraytracer_amd import _lib, api
from denoise_ref import denoise, random_case
from denoise_var_ref import MODES, denoise_var, denoise_var_f64, prefiltered_var, spatial_variance, variance_of

MRT_ERR_INVALID_ARG = 1
OTHER = {"sigma_l": 2.5, "normal_exp": 3, "sigma_z": 0.4, "sigma_a": 0.25}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("K", [0.2, math.inf])
@pytest.mark.parametrize("params", [{}, OTHER])
def test_variance_0_is_denoise_ref(K, params):
    rgba, S, guides = random_case(np.random.default_rng(4), 21, 26)
    for it in (1, 3, 5):
        p = dict(params, iterations=it)
        assert np.array_equal(_bits(denoise_var(rgba, S, K, guides, p, 0)), _bits(denoise(rgba, S, K, guides, p)))


@pytest.mark.parametrize("variance", [0, 1, 2])
@pytest.mark.parametrize("iterations", [1, 2, 4])
def test_float32_form_matches_float64(variance, iterations):
    rgba, S, guides = random_case(np.random.default_rng(10 * variance + iterations), 13, 17)
    for params in ({}, OTHER):
        p = dict(params, iterations=iterations)
        got = denoise_var(rgba, S, 1.0 / 7.0, guides, p, variance)
        ref = denoise_var_f64(rgba, S, 1.0 / 7.0, guides, p, variance)
        assert got.dtype == np.float32
        # the same texels pass through (NaN / Inf where the input had them) and the rest agree to float32 rounding
        assert np.array_equal(np.isfinite(got), np.isfinite(ref))
        fin = np.isfinite(ref)
        np.testing.assert_allclose(got[fin], ref[fin], rtol=2e-4, atol=2e-6)
        # texels that are not finite pass through in every mode, alpha is the frame's
        for y, x in ((1, 2), (6, 16), (0, 8), (12, 0)):
            assert np.array_equal(_bits(got[y, x]), _bits(rgba[y, x])), (y, x)
        assert np.array_equal(_bits(got[..., 3]), _bits(rgba[..., 3]))


def test_a_zero_variance_texel_is_filtered_when_its_neighbourhood_has_variance():
    # S == 0 at (6, 5) and (2, 1): passed through by the accumulated estimate, not by the prefiltered one (g_p != 0)
    rgba, S, guides = random_case(np.random.default_rng(1), 13, 17)
    acc = denoise_var(rgba, S, 0.25, guides, None, 0)
    pre = denoise_var(rgba, S, 0.25, guides, None, 1)
    for y, x in ((6, 5), (2, 1)):
        assert np.array_equal(_bits(acc[y, x]), _bits(rgba[y, x]))
        assert not np.array_equal(_bits(pre[y, x, :3]), _bits(rgba[y, x, :3]))


def test_prefiltered_without_an_estimate_is_accumulated():
    rgba, S, guides = random_case(np.random.default_rng(2), 19, 23)
    for p in ({"iterations": 1}, {"iterations": 4}, dict(OTHER, iterations=5)):
        assert np.array_equal(_bits(denoise_var(rgba, S, math.inf, guides, p, 1)), _bits(denoise_var(rgba, S, math.inf, guides, p, 0)))


def test_prefilter_of_a_constant_field_changes_nothing():
    # a constant var of few mantissa bits: every 3 x 3 sum (clipped ones too) is exact, so g_p == var_p and the modes agree bit
    # for bit, interior and border.  One iteration: the propagated var of the first is no longer constant, so later iterations
    # may differ by design.
    rgba, S, guides = random_case(np.random.default_rng(3), 20, 24, nonfinite=False, zero_var=False)
    S[:] = 0.25
    cv = np.concatenate([rgba[..., :3], (S * np.float32(0.5))[..., None]], -1).astype(np.float32)
    assert np.array_equal(_bits(prefiltered_var(cv, np.ones(S.shape, bool))), _bits(cv[..., 3]))
    for p in ({"iterations": 1}, dict(OTHER, iterations=1)):
        a = denoise_var(rgba, S, 0.5, guides, p, 0)
        b = denoise_var(rgba, S, 0.5, guides, p, 1)
        assert np.array_equal(_bits(a[1:-1, 1:-1]), _bits(b[1:-1, 1:-1])) and np.array_equal(_bits(a), _bits(b))
        assert not np.array_equal(_bits(a[..., :3]), _bits(rgba[..., :3]))


def test_spatial_variance_of_a_constant_image_is_zero_and_everything_passes_through():
    rgba, S, guides = random_case(np.random.default_rng(6), 15, 18, nonfinite=False, zero_var=False)
    # a constant whose sums are exact whatever the weights (L = 0: m1 = 0, mean = 0, every d = 0): var is exactly 0
    rgba[..., :3] = 0.0
    var = spatial_variance(rgba, S, guides)
    assert np.array_equal(var, np.zeros_like(var))
    for p in ({"iterations": 1}, {"iterations": 5}):
        assert np.array_equal(_bits(denoise_var(rgba, S, 0.25, guides, p, 2)), _bits(rgba))
    # any other constant c: mean = m1 / m0 is c up to the rounding of two 49-term float32 sums and a division, each term's
    # relative error at most 2^-24 -- |mean - c| <= 100 * 2^-24 * c, and var, a weighted mean of (c - mean)^2, at most its square
    rgba[..., :3] = np.float32(0.375)
    var = spatial_variance(rgba, S, guides)
    assert (var >= 0).all() and var.max() <= (100 * 2.0 ** -24 * 0.375) ** 2


def test_spatial_variance_special_texels():
    rgba, S, guides = random_case(np.random.default_rng(8), 13, 17)
    var = spatial_variance(rgba, S, guides)
    assert var[1, 2] == 0 and var[6, 16] == 0                 # colour not finite, S finite
    assert np.isnan(var[0, 8]) and np.isinf(var[12, 0])       # S not finite: kept
    rest = np.isfinite(rgba[..., :3]).all(-1) & np.isfinite(S)
    assert np.isfinite(var[rest]).all() and (var[rest] >= 0).all() and (var[rest] > 0).any()
    # the estimate does not read S's value: another finite S gives the same bits
    assert np.array_equal(_bits(spatial_variance(rgba, np.where(np.isfinite(S), np.float32(1), S), guides)), _bits(var))


def test_mode_schedule():
    assert [variance_of(2, n, 3) for n in (0, 1, 2, 3, 4, 100)] == [2, 2, 2, 1, 1, 1]
    assert [variance_of(2, n, 1) for n in (0, 1, 2)] == [2, 1, 1]
    assert all(variance_of(m, n, 3) == m for m in (0, 1) for n in (0, 1, 5))


def test_interface_constants_and_null_context():
    L = _lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/myraytracer_amd.h").read()
    values = {k: int(v) for k, v in re.findall(r"MRT_DENOISE_VAR_(\w+) = (\d)", hdr)}
    assert values == {"ACCUMULATED": 0, "PREFILTERED": 1, "SPATIAL_EARLY": 2}
    assert (_lib.DENOISE_VAR_ACCUMULATED, _lib.DENOISE_VAR_PREFILTERED, _lib.DENOISE_VAR_SPATIAL_EARLY) == (0, 1, 2)
    assert api.DENOISE_VARIANCE_MODES == MODES == ("accumulated", "prefiltered", "spatial-early")
    mode, frames = C.c_uint32(9), C.c_uint32(9)
    assert L.mrt_set_denoise_variance(None, 1, 3) == MRT_ERR_INVALID_ARG
    assert L.mrt_get_denoise_variance(None, C.byref(mode), C.byref(frames)) == MRT_ERR_INVALID_ARG
    assert (mode.value, frames.value) == (9, 9)
    # mrt_denoise_params is untouched by the modes
    assert C.sizeof(_lib.MrtDenoiseParams) == 48 and "/* 48 bytes */" in hdr
