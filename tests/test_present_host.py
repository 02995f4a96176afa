"""The present pass's host side, without a GPU: the threshold table the kernel searches reproduces mrt_srgb8 for every float
(code boundaries, random bit patterns, specials), and mrt_present_info has the header's layout."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _codes_by_threshold(t, v):
    """What the device computes: the number of t[1..255] that are <= v (NaN reaches none)."""
    v = np.asarray(v, np.float32)
    k = np.searchsorted(t[1:], v, side="right").astype(np.int64)
    return np.where(np.isnan(v), 0, k)


def test_thresholds_are_the_code_boundaries(mrt):
    L = mrt._lib.load()
    t = mrt.srgb8_thresholds()
    assert t.dtype == np.float32 and t.shape == (256,) and t[0] == -np.inf
    assert np.all(np.diff(t[1:]) > 0)
    for k in range(1, 256):
        assert L.mrt_srgb8(float(t[k])) == k, k
        below = np.nextafter(t[k], np.float32(0))
        assert L.mrt_srgb8(float(below)) == k - 1, k


def test_threshold_search_equals_srgb8_on_a_million_floats(mrt):
    L = mrt._lib.load()
    t = mrt.srgb8_thresholds()
    rng = np.random.default_rng(7)
    parts = [
        rng.integers(0, 0x3F800001, 600_000, dtype=np.uint32).view(np.float32),            # every bit pattern of [0, 1]
        rng.random(300_000, dtype=np.float32),                                                # uniform in [0, 1)
        rng.normal(0.5, 2.0, 100_000).astype(np.float32),                                     # negatives and values above 1
    ]
    thr = t[1:]
    near = np.concatenate([thr, np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(2))])
    specials = np.array([0.0, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), np.inf, -np.inf, np.nan,
                         1e-45, -1e-45, 1.1754942e-38, 1.1754944e-38, 0.0031308, 3.4028235e38, -3.4028235e38], np.float32)
    nan_payloads = np.array([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0xFF800001], np.uint32).view(np.float32)
    v = np.concatenate(parts + [near.astype(np.float32), specials, nan_payloads])
    got = _codes_by_threshold(t, v)
    want = np.array([L.mrt_srgb8(float(x)) for x in v], np.int64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(float(v[i]), int(got[i]), int(want[i])) for i in bad[:5]]


def test_present_info_layout_matches_the_header(mrt):
    from myraytracer_amd import _lib
    I = _lib.MrtPresentInfo
    assert C.sizeof(I) == 40
    assert I.seq.offset == 0 and I.frames_done.offset == 8 and I.dropped.offset == 32 and I.ring_depth.offset == 36
    text = open(os.path.join(ROOT, "include", "myraytracer_amd.h")).read()
    consts = dict((n, int(v)) for n, v in re.findall(r"\b(MRT_(?:PRESENT|ACQUIRE)_[A-Z0-9_]+)\s*=\s*(\d+)", text))
    assert consts == {"MRT_PRESENT_RGBA8_SRGB": _lib.PRESENT_RGBA8_SRGB, "MRT_PRESENT_BGRA8_SRGB": _lib.PRESENT_BGRA8_SRGB,
                      "MRT_PRESENT_FLIP_Y": _lib.PRESENT_FLIP_Y, "MRT_PRESENT_GATHERED": _lib.PRESENT_GATHERED,
                      "MRT_ACQUIRE_NEWEST": _lib.ACQUIRE_NEWEST, "MRT_ACQUIRE_OLDEST": _lib.ACQUIRE_OLDEST}


def test_host_reference_alpha_rule():
    from present_ref import alpha8_host
    a = np.array([np.nan, -1.0, -0.0, 0.0, 1.0 / 510, np.nextafter(np.float32(1.0 / 510), np.float32(0)), 0.5, 1.0, 2.0,
                  np.inf, -np.inf], np.float32)
    assert alpha8_host(a).tolist() == [0, 0, 0, 0, 1 if np.float64(np.float32(1.0 / 510)) * 255 >= 0.5 else 0, 0, 128, 255,
                                       255, 255, 0]
