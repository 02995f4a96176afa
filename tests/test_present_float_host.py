"""The host side of the present pass's linear formats, without a GPU: mrt_half_bits / mrt_half_from_floats (the one definition
of the RGBA16F_LINEAR channel, which present.hip compiles too) against numpy's float32 -> float16 at every rounding boundary,
the specials and the NaN rule, and the Python surface of the two formats."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from present_float_ref import HALF_NAN, NAN_PAYLOADS, boundary_set, half_bits_numpy, midpoints, specials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(L, x):
    return int(L.mrt_half_bits(C.c_float(float(x))))


def _bits(u):
    return np.array([u], np.uint32).view(np.float32)


def test_half_bits_equals_numpy_at_every_rounding_boundary(mrt):
    """For each of the 31,744 finite non-negative halves: the half, its float32 successor, the midpoint to the next half and
    that midpoint's two float32 neighbours, both signs: 317,440 floats.  The conversion is monotone (non-decreasing in the
    value), and each of its steps lies between one of these adjacent pairs -- the last float that gives a half and the first
    that gives the next one -- so agreement with a correct conversion at every such pair fixes it for every finite float in
    between, which then must give the half both ends of its run give."""
    v = boundary_set()
    assert v.shape == (317440,) and v.dtype == np.float32
    got = mrt._lib.half_bits(v)
    assert got.dtype == np.uint16 and got.shape == v.shape
    want = half_bits_numpy(v)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(float(v[i]), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]
    # monotone over the non-negative half of the set, and every finite half is reached
    pos = np.sort(v[: len(v) // 2])
    codes = mrt._lib.half_bits(pos).astype(np.int64)
    assert np.all(np.diff(codes) >= 0) and set(range(0x7C01)) <= set(codes.tolist())


def test_the_batch_and_the_scalar_form_agree_and_random_patterns_match_numpy(mrt):
    L = mrt._lib.load()
    rng = np.random.default_rng(16)
    u = rng.integers(0, 1 << 32, 1_000_000, dtype=np.uint64).astype(np.uint32)
    v = u.view(np.float32)
    got = mrt._lib.half_bits(v)
    assert np.array_equal(got, half_bits_numpy(v))
    for x in np.concatenate([v[:2000], boundary_set()[::997], specials()]):
        want = int(mrt._lib.half_bits(np.array([x], np.float32))[0])
        assert _one(L, x) == want, (float(x), want)
    assert mrt._lib.half_bits(np.zeros((3, 5, 4), np.float32)).shape == (3, 5, 4)
    assert L.mrt_half_from_floats(None, 0, None) == 0 and L.mrt_half_from_floats(None, 4, None) == 1


def test_specials(mrt):
    L = mrt._lib.load()
    s = specials()
    finite_or_inf = s[~np.isnan(s)]
    assert np.array_equal(mrt._lib.half_bits(finite_or_inf), half_bits_numpy(finite_or_inf))
    f32 = np.float32
    table = [(0.0, 0x0000), (-0.0, 0x8000), (np.inf, 0x7C00), (-np.inf, 0xFC00), (1e-45, 0x0000), (-1e-45, 0x8000),
             (1.1754942e-38, 0x0000), (3.4028235e38, 0x7C00), (-3.4028235e38, 0xFC00), (65504.0, 0x7BFF),
             (f32(65519.996), 0x7BFF), (65520.0, 0x7C00), (-f32(65519.996), 0xFBFF), (-65520.0, 0xFC00),
             (2.0 ** -25, 0x0000), (-(2.0 ** -25), 0x8000), (np.nextafter(f32(2.0 ** -25), f32(1)), 0x0001),
             (2.0 ** -24, 0x0001), (np.nextafter(f32(2.0 ** -14), f32(0)), 0x0400), (2.0 ** -14, 0x0400), (1.0, 0x3C00), (-2.0, 0xC000)]
    assert f32(65519.996) == np.nextafter(f32(65520), f32(0))
    for x, want in table:
        assert _one(L, x) == want, (x, hex(_one(L, x)), hex(want))
    ties = mrt._lib.half_bits(midpoints())
    assert ties.shape == (31744,) and not np.any(ties & 1)                  # ties to even
    assert np.array_equal(mrt._lib.half_bits(-midpoints()), ties | 0x8000)


def test_every_nan_is_one_half(mrt):
    L = mrt._lib.load()
    required = (0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFF800001, 0x7FA00000)
    assert set(required) <= set(NAN_PAYLOADS)
    rng = np.random.default_rng(5)
    more = (rng.integers(1, 1 << 23, 4096, dtype=np.uint64).astype(np.uint32) | 0x7F800000 |
            (rng.integers(0, 2, 4096, dtype=np.uint64).astype(np.uint32) << 31))
    u = np.concatenate([np.array(NAN_PAYLOADS, np.uint32), more])
    v = u.view(np.float32)
    assert np.all(np.isnan(v))
    assert np.all(mrt._lib.half_bits(v) == HALF_NAN)
    for p in NAN_PAYLOADS:
        assert int(L.mrt_half_bits(C.c_float.from_buffer(C.c_uint32(p)))) == HALF_NAN, hex(p)


def test_python_surface_and_header(mrt):
    from myraytracer_amd import _lib, api
    assert (_lib.PRESENT_RGBA16F_LINEAR, _lib.PRESENT_RGBA32F_LINEAR) == (16, 32)
    assert api.State._PRESENT_FORMATS == {"rgba8": 1, "bgra8": 2, "rgba16f": 16, "rgba32f": 32}
    st = object.__new__(api.State)                      # (no context: the name is refused before the library is called)
    with pytest.raises(ValueError):
        st.present("rgba4")
    hdr = open(os.path.join(ROOT, "include", "myraytracer_amd.h")).read()
    assert re.search(r"^#define MRT_PRESENT_RGBA16F_LINEAR 16\b", hdr, re.M) and re.search(r"^#define MRT_PRESENT_RGBA32F_LINEAR 32\b", hdr, re.M)
    assert re.search(r"^#define MRT_ABI_VERSION 4$", hdr, re.M)
    version_4 = hdr[hdr.index("/* 4: round 5"):hdr.index("#define MRT_ABI_VERSION")]
    for name in ("MRT_PRESENT_RGBA16F_LINEAR", "MRT_PRESENT_RGBA32F_LINEAR", "mrt_half_bits", "mrt_half_from_floats"):
        assert name in version_4, name
    assert re.search(r"^uint16_t mrt_half_bits\(float v\);", hdr, re.M)
    assert re.search(r"^int mrt_half_from_floats\(const float\* in, size_t n, uint16_t\* out\);", hdr, re.M)
    assert C.sizeof(_lib.MrtPresentInfo) == 40
