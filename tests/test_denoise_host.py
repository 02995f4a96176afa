"""The denoiser on the host (include/myraytracer_amd.h, "denoiser"): its parameters' defaults, checks and layout, and the float32
restatement of its filter (tests/denoise_ref.py, which the GPU tests compare the device against bit for bit) checked against a
plain float64 form of the same definition, edge cases included."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import myraytracer_amd as M
from myraytracer_amd import _lib
from denoise_ref import DEFAULTS, denoise, denoise_f64, random_case

MRT_OK, MRT_ERR_INVALID_ARG = 0, 1


def _params(**kw):
    p = _lib.MrtDenoiseParams()
    _lib.load().mrt_denoise_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _check(p):
    return _lib.load().mrt_set_denoise_params(None, C.byref(p))


def test_defaults_and_layout():
    assert C.sizeof(_lib.MrtDenoiseParams) == 48
    p = _params()
    assert p.size == 48 and list(p.reserved) == [0] * 6
    d = M.denoise_params_default()
    assert d == {k: (float(np.float32(v)) if k.startswith("sigma") else v) for k, v in DEFAULTS.items()}
    assert _check(p) == MRT_OK
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/myraytracer_amd.h").read()
    assert re.search(r"\} mrt_denoise_params;", hdr) and "/* 48 bytes */" in hdr


@pytest.mark.parametrize("field,bad", [("iterations", 0), ("iterations", 9), ("normal_exp", 17), ("sigma_l", 0.0),
                                       ("sigma_l", -1.0), ("sigma_l", math.inf), ("sigma_z", math.nan), ("sigma_z", 0.0),
                                       ("sigma_a", -0.5), ("sigma_a", math.inf), ("size", 44), ("size", 0)])
def test_parameter_ranges(field, bad):
    assert _check(_params(**{field: bad})) == MRT_ERR_INVALID_ARG


def test_parameter_range_ends_and_reserved():
    for kw in ({"iterations": 1}, {"iterations": 8}, {"normal_exp": 0}, {"normal_exp": 16}, {"sigma_l": 1e-30},
               {"sigma_z": 1e30}, {"sigma_a": 3.0}):
        assert _check(_params(**kw)) == MRT_OK, kw
    p = _params()
    p.reserved[3] = 1
    assert _check(p) == MRT_ERR_INVALID_ARG
    assert _lib.load().mrt_set_denoise_params(None, None) == MRT_ERR_INVALID_ARG


def _compare(rgba, S, K, guides, params):
    got = denoise(rgba, S, K, guides, params)
    ref = denoise_f64(rgba, S, K, guides, params)
    assert got.dtype == np.float32
    # the same texels pass through (NaN / Inf where the input had them) and the rest agree to float32 rounding
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    fin = np.isfinite(ref)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=2e-4, atol=2e-6)
    return got


@pytest.mark.parametrize("iterations", range(1, 9))
def test_float32_form_matches_float64_every_iteration_count(iterations):
    rng = np.random.default_rng(iterations)
    rgba, S, guides = random_case(rng, 13, 17)
    got = _compare(rgba, S, 1.0 / 7.0, guides, {"iterations": iterations})
    # non-finite texels and var == 0 texels pass through, alpha is the frame's
    for y, x in ((1, 2), (6, 16), (0, 8), (12, 0), (6, 5), (2, 1)):
        assert np.array_equal(got[y, x].view(np.uint32), rgba[y, x].view(np.uint32)), (y, x)
    assert np.array_equal(got[..., 3].view(np.uint32), rgba[..., 3].view(np.uint32))


def test_no_estimate_has_no_luminance_stop_and_no_zero_var_rule():
    rng = np.random.default_rng(11)
    rgba, S, guides = random_case(rng, 12, 10)
    S[:] = 0.0                     # a first frame: S = 0, K = +inf -- filtered by the guides alone, never 0 * inf
    S[3, 3] = np.nan               # ... but a non-finite S still passes through
    got = _compare(rgba, S, math.inf, guides, {"iterations": 3})
    assert not np.array_equal(got[5, 5], rgba[5, 5])
    assert np.array_equal(got[3, 3].view(np.uint32), rgba[3, 3].view(np.uint32))
    assert np.isfinite(got[~np.isnan(rgba).any(-1) & ~np.isinf(rgba).any(-1)]).all()


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (7, 1), (5, 6)])
def test_borders_and_tiny_images(shape):
    rng = np.random.default_rng(sum(shape))
    rgba, S, guides = random_case(rng, *shape, nonfinite=False, zero_var=False)
    for params in ({"iterations": 4}, {"iterations": 2, "sigma_l": 1.5, "normal_exp": 2, "sigma_z": 0.5, "sigma_a": 0.3}):
        _compare(rgba, S, 0.25, guides, params)


def test_a_flat_surface_is_smoothed_and_an_edge_is_kept():
    rng = np.random.default_rng(5)
    rows, width = 16, 16
    idx = np.where(np.arange(width)[None, :] < 8, 0, 1).repeat(rows, 0).astype(np.int32)
    guides = {"index": idx, "t": np.full((rows, width), 2.0, np.float32),
              "normal": np.tile(np.array([0, 0, 1], np.float32), (rows, width, 1)),
              "albedo": np.where(idx[..., None] == 0, np.float32(0.2), np.float32(0.8)).astype(np.float32) * np.ones(3, np.float32)}
    truth = np.where(idx == 0, 0.1, 0.6).astype(np.float32)
    noise = rng.normal(scale=0.05, size=(rows, width)).astype(np.float32)
    rgba = np.ones((rows, width, 4), np.float32)
    rgba[..., :3] = (truth + noise)[..., None]
    S = np.full((rows, width), np.float32(0.05 ** 2 * 3), np.float32)
    out = denoise(rgba, S, 1.0 / 3.0, guides)
    err_in = np.sqrt(np.mean((rgba[..., 0] - truth) ** 2))
    err_out = np.sqrt(np.mean((out[..., 0] - truth) ** 2))
    assert err_out < 0.5 * err_in
    # nothing leaks across the albedo edge
    assert out[:, :8, 0].max() < 0.3 and out[:, 8:, 0].min() > 0.4


def test_fma32_is_correctly_rounded():
    from fractions import Fraction
    from denoise_ref import fma32
    rng = np.random.default_rng(3)
    a = rng.normal(size=4000).astype(np.float32)
    b = rng.normal(size=4000).astype(np.float32)
    c = rng.normal(size=4000).astype(np.float32) * np.float32(1e-3)
    # halfway cases: a * b lands exactly between two floats near c, with a tiny remainder either way
    a[:4] = np.float32(1 + 2 ** -12); b[:4] = np.float32(1 + 2 ** -12); c[:4] = np.float32(0)
    got = fma32(a, b, c)

    def exact(x, y, z):
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(v))
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        # the nearest; a tie goes to the even significand
        return min(cands, key=lambda q: (abs(Fraction(float(q)) - v), int(np.array(q, np.float32).view(np.uint32)) & 1))

    want = np.array([exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
