"""The denoise of an adaptive accumulation on the host (include/myraytracer_amd.h, "Adaptive accumulations"): the float32
restatement (tests/denoise_tiles_ref.py, which the GPU tests compare the device against bit for bit) reduces to denoise_var_ref
when every tile has the same count, agrees with a plain float64 form of the same rule, and behaves as the definition says on the
cases it singles out; the interface's names and the checks that need no context."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from myraytracer_amd import _lib, api
from denoise_ref import random_case
from denoise_tiles_ref import denoise_tiles, denoise_tiles_f64, library_k, pixel_frames, pixel_state, tile_map
from denoise_var_ref import denoise_var, variance_of

MRT_ERR_INVALID_ARG = 1
OTHER = {"sigma_l": 2.5, "normal_exp": 3, "sigma_z": 0.4, "sigma_a": 0.25}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# rows x width: whole tiles, ragged in both axes, one band shorter than a tile, ragged with several bands
SHAPES = [(16, 24), (13, 17), (3, 70), (21, 26)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _uniform(rows, width, n):
    return np.full(((rows + 7) // 8, (width + 7) // 8), n, np.uint32)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("max_w", [1.0, 0.25])
def test_a_uniform_map_is_the_uniform_filter(shape, max_w):
    rows, width = shape
    rgba, S, guides = random_case(np.random.default_rng(rows * width), rows, width)
    k_of = library_k(max_w)
    checked = 0
    for mode in (0, 1, 2):
        for n in (0, 1, 2, 3, 7):
            for spatial_frames in (1, 3):
                for p in ({"iterations": 5}, dict(OTHER, iterations=2)):
                    got = denoise_tiles(rgba, S, _uniform(rows, width, n), guides, p, mode, spatial_frames, k_of)
                    ref = denoise_var(rgba, S, api.noise_factor(n, max_w), guides, p, variance_of(mode, n, spatial_frames))
                    assert np.array_equal(_bits(got), _bits(ref)), (mode, n, spatial_frames, p)
                    checked += 1
    assert checked == 60
    assert math.isinf(api.noise_factor(1, max_w)) and math.isfinite(api.noise_factor(2, max_w))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("iterations", [1, 2, 4])
def test_float32_form_matches_float64(mode, iterations):
    rows, width = 13, 17
    rng = np.random.default_rng(10 * mode + iterations)
    rgba, S, guides = random_case(rng, rows, width)
    tiles = tile_map(rng, rows, width, [0, 1, 2, 3, 7, 40])             # 2 x 3 tiles: every value once
    assert sorted(tiles.ravel()) == [0, 1, 2, 3, 7, 40]
    for params in ({}, OTHER):
        p = dict(params, iterations=iterations)
        got = denoise_tiles(rgba, S, tiles, guides, p, mode, 3)
        ref = denoise_tiles_f64(rgba, S, tiles, guides, p, mode, 3)
        assert got.dtype == np.float32
        # exactly the texels that are not finite stay so, and the rest agree to float32 rounding
        assert np.array_equal(np.isfinite(got), np.isfinite(ref))
        assert np.array_equal(np.isfinite(got[..., :3]).all(-1), np.isfinite(rgba[..., :3]).all(-1))
        fin = np.isfinite(ref)
        np.testing.assert_allclose(got[fin], ref[fin], rtol=2e-4, atol=2e-6)
        for y, x in ((1, 2), (6, 16)):                                    # a colour that is not finite passes through
            assert np.array_equal(_bits(got[y, x]), _bits(rgba[y, x])), (y, x)
        assert np.array_equal(_bits(got[..., 3]), _bits(rgba[..., 3]))


def test_the_centre_decides_and_tiles_do_not_leak_their_stop():
    # one iteration of ACCUMULATED reads its taps' colours and the CENTRE's variance alone: every pixel's colour is what the uniform
    # filter with its own tile's count gives there, whatever the neighbouring tiles' counts are
    rows, width = 21, 26
    rng = np.random.default_rng(5)
    rgba, S, guides = random_case(rng, rows, width)
    tiles = tile_map(rng, rows, width, [1, 7, 1, 7, 0, 2])
    n = pixel_frames(tiles, rows, width)
    p = {"iterations": 1}
    got = denoise_tiles(rgba, S, tiles, guides, p, 0, 3)
    for count in (0, 1, 2, 7):
        ref = denoise_var(rgba, S, api.noise_factor(count, 1.0), guides, p, 0)
        here = n == count
        assert here.any() and np.array_equal(_bits(got[here]), _bits(ref[here])), count
    # ... and a centre without a stop ignores luminance: no finite S anywhere changes its colour, a centre with one reads its own
    _, _, stop = pixel_state(tiles, rows, width, 0, 3, library_k())
    other = denoise_tiles(rgba, np.where(np.isfinite(S), np.float32(3) * S + np.float32(0.01), S), tiles, guides, p, 0, 3)
    assert np.array_equal(_bits(other[~stop]), _bits(got[~stop]))
    assert not np.array_equal(_bits(other[stop]), _bits(got[stop]))


def test_zero_variance_texels():
    # S == 0 at (6, 5) and (2, 1), both in tile 0
    rows, width = 13, 17
    rgba, S, guides = random_case(np.random.default_rng(1), rows, width)
    tiles = np.array([[7, 1, 40], [2, 7, 0]], np.uint32)
    acc = denoise_tiles(rgba, S, tiles, guides, None, 0)
    pre = denoise_tiles(rgba, S, tiles, guides, None, 1)
    for y, x in ((6, 5), (2, 1)):
        # in a tile with a stop: passed through by ACCUMULATED, filtered when its g_p != 0
        assert np.array_equal(_bits(acc[y, x]), _bits(rgba[y, x]))
        assert not np.array_equal(_bits(pre[y, x, :3]), _bits(rgba[y, x, :3]))
    # in a tile without one every finite S gives var 0, and nothing passes through for it
    tiles[0, 0] = 1
    for mode in (0, 1, 2):
        out = denoise_tiles(rgba, S, tiles, guides, None, mode, 1)
        for y, x in ((6, 5), (2, 1), (3, 3)):
            assert not np.array_equal(_bits(out[y, x, :3]), _bits(rgba[y, x, :3])), (mode, y, x)


def test_a_tile_without_frames_takes_its_neighbours_colour():
    rows, width = 16, 24
    rgba, S, guides = random_case(np.random.default_rng(9), rows, width, nonfinite=False, zero_var=False)
    tiles = np.full((2, 3), 12, np.uint32)
    tiles[0, 1] = 0
    rgba[0:8, 8:16, :3] = 0.0
    S[0:8, 8:16] = 0.0
    # one surface, so that the edge stops pass
    guides["index"][:] = 0
    guides["t"][:] = 2.0
    guides["normal"][:] = (0.0, 0.0, 1.0)
    guides["albedo"][:] = 0.5
    out = denoise_tiles(rgba, S, tiles, guides, None, 0)
    assert (out[0:8, 8:16, :3] > 0).all()


def test_the_map_of_pixel_counts():
    n = pixel_frames(np.arange(15, dtype=np.uint32), 19, 37)            # 3 x 5 tiles
    assert n.shape == (19, 37) and n[0, 0] == 0 and n[7, 7] == 0 and n[8, 7] == 5 and n[7, 8] == 1 and n[18, 36] == 14
    K, spatial, stop = pixel_state(np.array([[0, 1, 2, 3]], np.uint32), 8, 32, 2, 3, library_k())
    assert np.isinf(K[0, 0]) and np.isinf(K[0, 8]) and np.isfinite(K[0, 16]) and np.isfinite(K[0, 24])
    assert [bool(spatial[0, x]) for x in (0, 8, 16, 24)] == [True, True, True, False]
    assert stop.all()
    _, spatial, stop = pixel_state(np.array([[0, 1, 2, 3]], np.uint32), 8, 32, 1, 3, library_k())
    assert not spatial.any() and [bool(stop[0, x]) for x in (0, 8, 16, 24)] == [False, False, True, True]


def test_interface_names_and_null_arguments():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "myraytracer_amd.h")).read()
    dbg = open(os.path.join(ROOT, "include", "myraytracer_amd_debug.h")).read()
    assert re.search(r"#define MRT_ABI_VERSION 4\b", hdr) and L.mrt_abi_version() == 4
    assert re.search(r"\bint mrt_set_denoise_adaptive\(mrt_ctx\* ctx, int enabled\);", hdr)
    assert re.search(r"\bint mrt_get_denoise_adaptive\(mrt_ctx\* ctx, int\* enabled\);", hdr)
    assert re.search(r"\bint mrt_debug_load_accumulation\(mrt_ctx\* ctx, const float\* rgba, const float\* S, const uint32_t\* tile_frames\);", dbg)
    version_4 = hdr[hdr.index("/* 4: round 5"):hdr.index("#define MRT_ABI_VERSION")]
    assert "mrt_set_denoise_adaptive" in version_4 and "mrt_get_denoise_adaptive" in version_4
    for name in ("mrt_set_denoise_adaptive", "mrt_get_denoise_adaptive", "mrt_debug_load_accumulation"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    for name in ("set_denoise_adaptive", "denoise_adaptive", "debug_load_accumulation"):
        assert callable(getattr(api.State, name))
    on = C.c_int(9)
    assert L.mrt_set_denoise_adaptive(None, 1) == MRT_ERR_INVALID_ARG
    assert L.mrt_get_denoise_adaptive(None, C.byref(on)) == MRT_ERR_INVALID_ARG and on.value == 9
    assert L.mrt_get_denoise_adaptive(None, None) == MRT_ERR_INVALID_ARG
    assert L.mrt_debug_load_accumulation(None, None, None, None) == MRT_ERR_INVALID_ARG
