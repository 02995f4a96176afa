"""Host reference of the present pass's linear formats (MRT_PRESENT_RGBA16F_LINEAR / RGBA32F_LINEAR): the float32 values at
which the conversion to binary16 (mrt_half_bits, include/myraytracer_amd.h) can go wrong, numpy's conversion as the reference
for every float but NaN, and the texel sets the GPU tests present.  Shared by tests/test_present_float_host.py (no GPU) and
tests/test_gpu_present_float.py."""
import functools

import numpy as np

HALF_NAN = 0x7E00                       # what every NaN becomes, whatever its sign or payload
NAN_PAYLOADS = (0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFF800001, 0x7FA00000, 0xFFC00000, 0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def _boundary_set():
    h = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)      # the 31,744 finite non-negative halves
    nxt = np.append(h[1:], 65536.0)                                                  # (the half after 65504, were there one)
    inf = np.float32(np.inf)
    own = h.astype(np.float32)                          # exact
    mid = ((h + nxt) / 2).astype(np.float32)            # exact: one more mantissa bit than a half; 65520 above 65504
    assert np.array_equal(mid.astype(np.float64), (h + nxt) / 2) and mid[-1] == 65520.0
    pos = np.concatenate([own, np.nextafter(own, inf), mid, np.nextafter(mid, -inf), np.nextafter(mid, inf)])
    v = np.concatenate([pos, -pos])
    v.setflags(write=False)
    return v


def boundary_set():
    """317,440 float32: for each finite non-negative half h -- h, the float32 after it, the midpoint to the next half (65520 above
    65504: the threshold to inf) and the midpoint's two float32 neighbours -- and all of these negated."""
    return _boundary_set()


def midpoints():
    """the 31,744 non-negative midpoints of boundary_set(): the ties"""
    return _boundary_set()[2 * 0x7C00:3 * 0x7C00]


def specials():
    """zeros, infinities, float32 subnormals, FLT_MAX, the thresholds to inf and to zero, NaNs of both signs"""
    f = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 5e-39, 3.4028235e38, -3.4028235e38,
                  65519.996, 65520.0, -65519.996, -65520.0, 65504.0, 2.0 ** -25, -(2.0 ** -25), 2.0 ** -24, 2.0 ** -14, 1.0, -1.0,
                  0.1, 1e5], np.float32)
    after_tie = np.nextafter(np.float32(2.0 ** -25), np.float32(1))
    return np.concatenate([f, [after_tie, -after_tie], np.array(NAN_PAYLOADS, np.uint32).view(np.float32)]).astype(np.float32)


def half_bits_numpy(v):
    """uint16 bits of numpy's float32 -> float16 (round to nearest even, subnormals kept, inf from 65520), NaN -> HALF_NAN:
    numpy is not the reference for NaN (it carries the payload's top bits and the sign over)."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        bits = v.astype(np.float16).view(np.uint16)
    return np.where(np.isnan(v), np.uint16(HALF_NAN), bits)


def rolled_texels(values):
    """[n, 4] float32 texels in which every value of `values` appears in every channel"""
    v = np.asarray(values, np.float32)
    v = np.concatenate([v, np.zeros(-len(v) % 4, np.float32)])
    return np.stack([np.roll(v, k) for k in range(4)], axis=1).copy()


def image_of(texels, width):
    """[rows, width, 4]: the texels in row-major order, zero-padded to whole rows"""
    rows = -(-len(texels) // width)
    img = np.zeros((rows * width, 4), np.float32)
    img[:len(texels)] = texels
    return img.reshape(rows, width, 4)
