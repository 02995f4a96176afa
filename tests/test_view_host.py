"""The diagnostic views' host side (include/myraytracer_amd.h, "diagnostic views"; no GPU needed): the setting's defaults and
validation through mrt_set_view(NULL, ...), the new names in the binding and the header, and the reference ramp of
tests/view_ref.py -- its stops, its monotone channels between them and the NaN colour."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import view_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("mrt_view_default", "mrt_set_view", "mrt_get_view", "mrt_read_view")
INVALID_ARG = 1


def _default(mrt):
    v = mrt._lib.MrtView()
    mrt._lib.load().mrt_view_default(C.byref(v))
    return v


def test_defaults_size_and_names(mrt):
    L = mrt._lib
    v = _default(mrt)
    assert C.sizeof(L.MrtView) == 32 == v.size
    assert (v.kind, v.ramp) == (L.VIEW_NOISE_REL, L.VIEW_RAMP_HEAT) == (2, 1)
    assert (v.lo, v.hi) == (0.0, float(F(0.1))) and list(v.reserved) == [0, 0]
    # rel_floor: the floor State.render_until passes to mrt_noise_query
    floor = inspect.signature(mrt.State.render_until).parameters["floor"].default
    assert v.rel_floor == float(F(floor))
    assert mrt.view_default() == {"kind": "noise_rel", "ramp": "heat", "lo": 0.0, "hi": float(F(0.1)), "rel_floor": float(F(floor))}
    assert L.PRESENT_VIEW == 128 and L.VIEW_KINDS == {"noise_se": 1, "noise_rel": 2, "tile_frames": 3, "depth": 4, "normal": 5,
                                                     "albedo": 6, "sphere": 7} and L.VIEW_RAMPS == {"grey": 0, "heat": 1}
    header = open(os.path.join(ROOT, "include", "myraytracer_amd.h")).read()
    for name in NAMES:
        assert name in L.EXPORTS and re.search(r"\b%s\s*\(" % name, header), name
    for text in ("#define MRT_PRESENT_VIEW 128u", "MRT_VIEW_NOISE_SE = 1", "MRT_VIEW_SPHERE = 7", "MRT_VIEW_RAMP_GREY = 0", "MRT_VIEW_RAMP_HEAT = 1",
                 "#define MRT_ABI_VERSION 4"):
        assert text in header, text
    assert L.load().mrt_abi_version() == 4


TINY = float(np.finfo(F).smallest_subnormal)          # 1 / TINY overflows float32
BIG = float(np.finfo(F).max)
VALID = [{}, {"kind": 1}, {"kind": 7}, {"ramp": 0}, {"lo": 0.3, "hi": 0.02}, {"lo": 0.0, "hi": 1e-38},
         {"rel_floor": 0.0}, {"rel_floor": BIG}, {"lo": -0.0, "hi": 1.0}]
INVALID = [{"kind": 0}, {"kind": 8}, {"kind": 0xFFFFFFFF}, {"ramp": 2}, {"ramp": 0xFFFFFFFF},
           {"lo": 0.25, "hi": 0.25}, {"lo": 0.0, "hi": -0.0}, {"lo": 0.0, "hi": TINY}, {"lo": TINY, "hi": 0.0}, {"lo": 1.0, "hi": 1.0},
           {"lo": math.nan}, {"hi": math.nan}, {"lo": math.inf}, {"hi": -math.inf}, {"lo": -math.inf, "hi": math.inf},
           {"rel_floor": -1e-30}, {"rel_floor": math.nan}, {"rel_floor": math.inf},
           {"size": 28}, {"size": 36}, {"size": 0}, {"reserved": (1, 0)}, {"reserved": (0, 1)}]


def _with(mrt, fields):
    v = _default(mrt)
    for k, x in fields.items():
        if k == "reserved":
            v.reserved[0], v.reserved[1] = x
        else:
            setattr(v, k, x)
    return v


@pytest.mark.parametrize("fields", VALID, ids=lambda f: ",".join(f"{k}={v}" for k, v in f.items()) or "default")
def test_valid_settings_pass_the_host_check(mrt, fields):
    assert mrt._lib.load().mrt_set_view(None, C.byref(_with(mrt, fields))) == 0


@pytest.mark.parametrize("fields", INVALID, ids=lambda f: ",".join(f"{k}={v}" for k, v in f.items()))
def test_invalid_settings_are_refused_on_the_host(mrt, fields):
    assert mrt._lib.load().mrt_set_view(None, C.byref(_with(mrt, fields))) == INVALID_ARG


def test_null_pointers(mrt):
    L = mrt._lib.load()
    assert L.mrt_set_view(None, None) == INVALID_ARG
    assert L.mrt_get_view(None, C.byref(mrt._lib.MrtView())) == INVALID_ARG
    assert L.mrt_read_view(None, None, 0) == INVALID_ARG
    L.mrt_view_default(None)


def test_the_reference_ramp_stops_monotone_channels_and_nan():
    for u, rgb in view_ref.HEAT_STOPS:
        assert view_ref.ramp(F(u), "heat", 0.0, 1.0).tolist() == [*map(float, rgb), 1.0], u
    # lo / hi: the stops move with them, a reversed pair reverses the ramp, and the ends clamp (+-inf included)
    assert view_ref.ramp(F([0.0, 1.0, -np.inf, np.inf]), "heat", 0.02, 0.3)[:, :3].tolist() == [[0, 0, 1], [1, 0, 0], [0, 0, 1], [1, 0, 0]]
    assert view_ref.ramp(F([0.0, 1.0, np.inf]), "heat", 0.3, 0.02)[:, :3].tolist() == [[1, 0, 0], [0, 0, 1], [0, 0, 1]]
    # between adjacent stops every channel is non-decreasing or non-increasing, and it runs from the one stop's value to the other's
    for (u0, c0), (u1, c1) in zip(view_ref.HEAT_STOPS, view_ref.HEAT_STOPS[1:]):
        u = np.linspace(u0, u1, 1025, dtype=F)
        rgb = view_ref.ramp(u, "heat", 0.0, 1.0)[:, :3]
        for ch in range(3):
            d = np.diff(rgb[:, ch])
            assert (d >= 0).all() if c1[ch] >= c0[ch] else (d <= 0).all(), (u0, ch)
            assert (rgb[0, ch], rgb[-1, ch]) == (c0[ch], c1[ch])
        assert (rgb >= 0).all() and (rgb <= 1).all()
    assert view_ref.ramp(F(np.nan), "heat", 0.0, 1.0).tolist() == [*view_ref.NAN_COLOUR, 1.0]
    grey = view_ref.ramp(F([np.nan, -2.5, 7.0, np.inf, -0.0]), "grey", 0.0, 1.0)
    assert np.isnan(grey[0, :3]).all() and grey[1:, 0].tolist() == [-2.5, 7.0, np.inf, 0.0] and (grey[:, 3] == 1).all()
    assert np.signbit(grey[4, 0])                       # (lo 0, hi 1: q's bits, the sign of a zero included)


def test_the_reference_sphere_colours():
    c = view_ref.sphere_colour(np.array([-1, 0, 1, 2 ** 31 - 2], np.int32))
    assert c[0].tolist() == [0, 0, 0, 1]
    h = 2654435761
    h ^= h >> 15
    assert c[1].tolist() == [((h >> 24) + 0.5) / 256, (((h >> 16) & 255) + 0.5) / 256, (((h >> 8) & 255) + 0.5) / 256, 1.0]
    assert ((c[1:, :3] > 0) & (c[1:, :3] < 1)).all()
    assert len({tuple(x) for x in view_ref.sphere_colour(np.arange(488, dtype=np.int32))[:, :3].tolist()}) > 480
