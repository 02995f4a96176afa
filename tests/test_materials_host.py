"""mrt_update_materials without a GPU (include/myraytracer_amd.h, "scene"): the struct's size, the refusal that needs no context,
the shared derivation of the shade words (mrt_debug_material_shade) against a numpy float32 restatement, and that the new
symbols are declared, exported and bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from myraytracer_amd import _lib

F = np.float32
MRT_ERR_INVALID_ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def restated(ty, albedo, param):
    """floats 4..7 of the shade record, each operation rounded to float32 in the header's order"""
    albedo, param = np.asarray(albedo, F), F(param)
    if ty == 1:
        return np.array([albedo[0], albedo[1], albedo[2], F(0)], F)
    if ty == 2:
        return np.array([albedo[0], albedo[1], albedo[2], param], F)
    if ty == 3:
        with np.errstate(all="ignore"):
            ri = F(1) / param

            def r0(x):
                q = (F(1) - x) / (F(1) + x)
                return q * q
            return np.array([ri, r0(ri), r0(param), param], F)
    return np.array([1, 1, 1, 0], F)


def test_the_struct_is_twenty_bytes_and_the_tail_of_a_sphere(mrt):
    assert C.sizeof(_lib.MrtMaterial) == 20 == mrt.MATERIAL_DTYPE.itemsize
    assert [(n, mrt.SPHERE_DTYPE.fields[n][1] - 16) for n in mrt.MATERIAL_DTYPE.names] == \
           [(n, mrt.MATERIAL_DTYPE.fields[n][1]) for n in mrt.MATERIAL_DTYPE.names]
    assert _lib.MATERIALS_RESTART_HISTORY == 1


def test_a_null_context_is_refused(mrt):
    L = _lib.load()
    m = np.zeros(2, mrt.MATERIAL_DTYPE)
    assert L.mrt_update_materials(None, 0, 2, m.ctypes.data, 0) == MRT_ERR_INVALID_ARG
    assert L.mrt_update_materials(None, 0, 0, None, 0) == MRT_ERR_INVALID_ARG
    out = (C.c_float * 4)()
    assert L.mrt_debug_material_shade(None, out) == MRT_ERR_INVALID_ARG
    assert L.mrt_debug_material_shade(C.cast(m.ctypes.data, C.POINTER(_lib.MrtMaterial)), None) == MRT_ERR_INVALID_ARG


CASES = [(1, (0.25, 0.5, 0.75), 0.0), (1, (0.1, 0.9, 0.3), 0.7),           # a Lambertian's param is not read
         (2, (0.8, 0.6, 0.2), 0.0), (2, (0.33, 0.66, 0.99), 0.35), (2, (1.0, 1.0, 1.0), 1.0),
         (3, (0.5, 0.5, 0.5), 1.5), (3, (0.0, 0.0, 0.0), 1.0), (3, (1.0, 1.0, 1.0), 2.4), (3, (0.2, 0.3, 0.4), 0.75),
         (3, (0.2, 0.3, 0.4), 1.33), (3, (0.2, 0.3, 0.4), 1.0 / 3.0),
         (7, (0.3, 0.4, 0.5), 0.6), (0, (0.3, 0.4, 0.5), 0.6), (-1, (0.3, 0.4, 0.5), 0.6), (4, (0.0, 0.0, 0.0), 0.0)]


@pytest.mark.parametrize("ty,albedo,param", CASES)
def test_the_shared_derivation_is_the_restatement_bit_for_bit(mrt, ty, albedo, param):
    m = np.zeros(1, mrt.MATERIAL_DTYPE)
    m[0] = (ty, albedo, param)
    got = mrt.material_shade(m[0])
    assert np.array_equal(_bits(got), _bits(restated(ty, albedo, param))), (got, restated(ty, albedo, param))
    if ty == 3 and param == 1.5:                # the figures DESIGN.md gives for glass: 1/1.5, r0 = 0.04 either way round
        assert got[0] == F(1) / F(1.5) and abs(float(got[1]) - 0.04) < 1e-7 and abs(float(got[2]) - 0.04) < 1e-7 and got[3] == F(1.5)


def test_a_sphere_array_gives_its_material_fields(mrt):
    sc = np.zeros(3, mrt.SPHERE_DTYPE)
    sc["center"], sc["radius"] = 5.0, 2.0
    sc["material_ty"], sc["albedo"], sc["param"] = [1, 2, 3], [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9]], [0.0, 0.25, 1.5]
    m = mrt.materials_of(sc)
    assert m.dtype == mrt.MATERIAL_DTYPE and m.flags["C_CONTIGUOUS"] and len(m) == 3
    for k in mrt.MATERIAL_DTYPE.names:
        assert np.array_equal(m[k], sc[k])
    assert mrt.materials_of(m) is not None and np.array_equal(mrt.materials_of(m), m)
    with pytest.raises(TypeError):
        mrt.materials_of(np.zeros((2, 5), np.float32))


def test_the_symbols_are_declared_exported_and_bound(mrt):
    L = _lib.load()
    public = open(os.path.join(ROOT, "include", "myraytracer_amd.h")).read()
    debug = open(os.path.join(ROOT, "include", "myraytracer_amd_debug.h")).read()
    assert re.search(r"\bint mrt_update_materials\(mrt_ctx\* ctx, uint32_t first, uint32_t count, const mrt_material\* materials, uint32_t flags\);", public)
    assert re.search(r"typedef struct \{ int32_t material_ty; float albedo\[3\]; float param; \} mrt_material;", public)
    assert "MRT_MATERIALS_RESTART_HISTORY = 1u" in public and "#define MRT_ABI_VERSION 4" in public
    assert re.search(r"\bint mrt_debug_material_shade\(const mrt_material\* material, float out\[4\]\);", debug)
    assert L.mrt_abi_version() == 4
    for name in ("mrt_update_materials", "mrt_debug_material_shade"):
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None
    assert hasattr(mrt.State, "update_materials")
