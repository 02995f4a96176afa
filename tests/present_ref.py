"""Host reference of the present pass (mrt_present): colour through the library's own mrt_srgb8, alpha stored linearly as an
sRGB-format target stores it, round(255 clamp(a, 0, 1)) with NaN -> 0, rows flipped to top-down on request."""
import numpy as np


def srgb8_host(L, x: np.ndarray) -> np.ndarray:
    """mrt_srgb8 of every element (called once per distinct bit pattern)."""
    x = np.ascontiguousarray(x, np.float32)
    bits, inv = np.unique(x.view(np.uint32).ravel(), return_inverse=True)
    codes = np.array([L.mrt_srgb8(float(v)) for v in bits.view(np.float32)], np.uint8)
    return codes[inv.ravel()].reshape(x.shape)


def alpha8_host(a: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):                      # (signalling NaN payloads)
        a = np.asarray(a, np.float32).astype(np.float64)    # (255 a is exact in double, so is + 0.5)
        a = np.where(a > 0, np.minimum(a, 1.0), 0.0)         # clamp; NaN -> 0
    return np.floor(a * 255.0 + 0.5).astype(np.uint8)


def encode_host(L, rgba: np.ndarray, fmt: str = "rgba8", flip: bool = False) -> np.ndarray:
    """float32 [rows, width, 4] -> uint8 [rows, width, 4] in the byte order of `fmt`."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    out = np.empty(rgba.shape, np.uint8)
    rgb = srgb8_host(L, rgba[..., :3])
    out[..., :3] = rgb[..., ::-1] if fmt == "bgra8" else rgb
    out[..., 3] = alpha8_host(rgba[..., 3])
    return out[::-1].copy() if flip else out
