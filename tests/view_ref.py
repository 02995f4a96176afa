"""Host reference of the diagnostic views (include/myraytracer_amd.h, "diagnostic views"), restated in float32 numpy in the
header's operation order.  Everything is (H, W) or (H, W, c) float32, row 0 = bottom, as the read-backs give it."""
import numpy as np

from noise_ref import lum

F = np.float32
SCALAR_KINDS = ("noise_se", "noise_rel", "tile_frames", "depth")
VECTOR_KINDS = ("normal", "albedo", "sphere")
HEAT_STOPS = ((0.0, (0, 0, 1)), (0.25, (0, 1, 1)), (0.5, (0, 1, 0)), (0.75, (1, 1, 0)), (1.0, (1, 0, 0)))     # u, rgb
NAN_COLOUR = (1.0, 0.0, 1.0)


def per_pixel(tile_values, height, width):
    """A value per 8x8 tile (tile rows x tile columns, or flat in that order) -> the value of every pixel's tile."""
    tr, tx = -(-height // 8), -(-width // 8)
    t = np.asarray(tile_values).reshape(tr, tx)
    return np.repeat(np.repeat(t, 8, axis=0), 8, axis=1)[:height, :width]


def noise_q(S, rgba, K, rel_floor, relative):
    """NOISE_SE / NOISE_REL's q.  K: one factor, or one per pixel (an adaptive accumulation: float32(K(n_t)) of the pixel's tile)."""
    S = np.asarray(S, F)
    L = lum(rgba)
    K = np.broadcast_to(np.asarray(K, F), S.shape)
    with np.errstate(all="ignore"):
        se = np.where(np.isinf(K), F(np.inf), np.sqrt(S * np.where(np.isinf(K), F(1), K))).astype(F)
        q = se / np.fmax(L, F(rel_floor)) if relative else se
    return np.where(np.isfinite(S) & np.isfinite(L), q, F(np.nan)).astype(F)


def c01(y):
    return np.fmin(np.fmax(y, F(0)), F(1))


def ramp(q, kind, lo, hi):
    """A scalar through the ramp: (..., 4) float32."""
    q = np.asarray(q, F)
    with np.errstate(all="ignore"):
        inv = F(1) / (F(hi) - F(lo))
        u = ((q - F(lo)) * inv).astype(F)
        out = np.empty(q.shape + (4,), F)
        if kind == "grey":
            out[..., 0] = out[..., 1] = out[..., 2] = u
        else:
            assert kind == "heat"
            v = np.fmin(np.fmax(u, F(0)), F(1))
            x = v * F(4)
            rgb = np.stack([c01(x - F(2)), c01(np.fmin(x, F(4) - x)), c01(F(2) - x)], axis=-1)
            out[..., :3] = np.where(np.isnan(q)[..., None], np.asarray(NAN_COLOUR, F), rgb)
    out[..., 3] = F(1)
    return out


def sphere_colour(index):
    i = np.asarray(index, np.int32)
    h = ((i.astype(np.int64) + 1) * 2654435761) & 0xFFFFFFFF
    h ^= h >> 15
    out = np.empty(i.shape + (4,), F)
    for c, shift in enumerate((24, 16, 8)):
        out[..., c] = (((h >> shift) & 255).astype(F) + F(0.5)) * F(1.0 / 256.0)
    out[i == -1, :3] = F(0)
    out[..., 3] = F(1)
    return out


def guide_view(kind, guides, ramp_kind="heat", lo=0.0, hi=0.1):
    """DEPTH, NORMAL, ALBEDO and SPHERE of State.debug_read_guides()'s dict."""
    if kind == "depth":
        return ramp(guides["t"], ramp_kind, lo, hi)
    if kind == "sphere":
        return sphere_colour(guides["index"])
    h, w = guides["t"].shape
    out = np.ones((h, w, 4), F)
    out[..., :3] = guides["normal"] * F(0.5) + F(0.5) if kind == "normal" else guides["albedo"]
    assert kind in ("normal", "albedo")
    return out


def same(got, want):
    """bit equality, or -- where the reference holds a NaN -- a NaN in the same position"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
