"""Host reference of the noise estimate (include/myraytracer_amd.h, "noise estimate"), restated in float32 numpy in the library's
operation order (it is built with -ffp-contract=off, so every step is one correctly rounded float32 operation): the per-texel
recursion the tracked blend runs, the blend itself, c2 / K, and the per-pixel maths and sums of a report."""
import math

import numpy as np

F = np.float32


def lum(rgb: np.ndarray) -> np.ndarray:
    rgb = np.asarray(rgb, np.float32)
    return (F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]


def blend(mean: np.ndarray, prev: np.ndarray, w: float) -> np.ndarray:
    """mixf(mean, prev, w) per channel, alpha from 1 (blend.h, blend_texel)."""
    w = F(w)
    out = np.empty_like(prev)
    out[..., :3] = mean[..., :3] * (F(1) - w) + prev[..., :3] * w
    out[..., 3] = F(1) * (F(1) - w) + prev[..., 3] * w
    return out


def s_update(S: np.ndarray, mean: np.ndarray, prev: np.ndarray, w: float) -> np.ndarray:
    """S' = (w == 0) ? 0 : w * (S + (1 - w) * (d * d)), d = lum(mean) - lum(prev.rgb)."""
    w = F(w)
    if w == F(0):
        return np.zeros_like(S)
    d = lum(mean) - lum(prev)
    with np.errstate(all="ignore"):
        return w * (S + (F(1) - w) * (d * d))


def c2_next(c2: float, w: float) -> float:
    w = float(np.float32(w))
    return 1.0 if w == 0.0 else w * w * c2 + (1.0 - w) * (1.0 - w)


def factor(c2: float) -> float:
    return math.inf if c2 >= 1.0 else c2 / (1.0 - c2)


def accumulate(means, weights, S=None, fb=None):
    """Blend the frames' means (each (H, W, 4) f32) with the given float weights; returns (fb, S, K)."""
    fb = np.zeros_like(means[0]) if fb is None else fb
    S = np.zeros(fb.shape[:-1], np.float32) if S is None else S
    c2 = 1.0
    for m, w in zip(means, weights):
        S = s_update(S, m, fb, w)
        fb = blend(m, fb, w)
        c2 = c2_next(c2, w)
    return fb, S, factor(c2)


def per_pixel(S: np.ndarray, rgba: np.ndarray, K: float, threshold: float, floor: float):
    """(finite mask, se, L, rel, above) in float32."""
    S = np.asarray(S, np.float32)
    L = lum(rgba)
    with np.errstate(all="ignore"):
        finite = np.isfinite(S) & np.isfinite(L)
        if math.isinf(K):
            se = np.full(S.shape, np.inf, np.float32)
        else:
            se = np.sqrt(S * F(K))
        rel = se / np.fmax(L, F(floor))
        above = finite & (rel > F(threshold))
    return finite, se, L, rel, above


def report(S: np.ndarray, rgba: np.ndarray, K: float, threshold: float = 0.02, floor: float = 0.01) -> dict:
    """The report the reduction gives for these buffers (rows x width; every row an image row)."""
    finite, se, L, rel, above = per_pixel(S, rgba, K, threshold, floor)
    n = int(finite.sum())
    sum_s = math.fsum(S[finite].astype(np.float64))
    sum_l = math.fsum(L[finite].astype(np.float64))
    out = {"pixels": n, "non_finite": int((~finite).sum()), "above": int(above.sum()), "noise_factor": K, "sum_lum": sum_l}
    if math.isinf(K):
        out.update(sum_var=math.inf, rmse=math.inf, rel_rmse=math.inf, max_se=math.inf)
        return out
    out["sum_var"] = sum_s * K
    out["max_se"] = float(np.max(se[finite], initial=np.float32(0)))
    out["rmse"] = math.sqrt(out["sum_var"] / n) if n else 0.0
    mean_l = sum_l / n if n else 0.0
    out["rel_rmse"] = 0.0 if out["rmse"] <= 0.0 else (out["rmse"] / mean_l if mean_l else math.inf)
    return out


def tiles(S: np.ndarray, rgba: np.ndarray, K: float, threshold: float = 0.02, floor: float = 0.01, valid=None) -> np.ndarray:
    """Per-8x8-tile maximum of rel over finite pixels (0 for a tile without one; NaN rel ignored).  valid: a (rows,) mask of the
    rows that are image rows -- a shard's packed rows end in padding, which the reduction skips (shard_rows)."""
    finite, se, L, rel, above = per_pixel(S, rgba, K, threshold, floor)
    rows, width = S.shape
    if valid is not None:
        finite = finite & np.asarray(valid, bool)[:, None]
    v = np.where(finite & ~np.isnan(rel), rel, np.float32(0)).astype(np.float32)
    tr, tx = -(-rows // 8), -(-width // 8)
    pad = np.zeros((tr * 8, tx * 8), np.float32)
    pad[:rows, :width] = v
    return pad.reshape(tr, 8, tx, 8).max(axis=(1, 3))


def shard_rows(height: int, rank: int, world: int) -> np.ndarray:
    """The image row of every packed local row of shard (rank, world) -- local row r is global row ((r / 8) world + rank) 8 + r % 8
    (mrt_shard_global_row), ceil(ceil(height / 8) / world) bands on every rank -- or -1 where that is >= height (padding)."""
    bands = -(-(-(-height // 8)) // world)
    r = np.arange(bands * 8)
    g = ((r // 8) * world + rank) * 8 + r % 8
    return np.where(g < height, g, -1)


def pack_rows(a: np.ndarray, rank: int, world: int) -> np.ndarray:
    """A full bottom-up image (H, ...) -> shard (rank, world)'s packed rows, padding rows zero (what the read-backs of a shard give)."""
    g = shard_rows(a.shape[0], rank, world)
    out = np.zeros((len(g),) + a.shape[1:], a.dtype)
    out[g >= 0] = a[g[g >= 0]]
    return out
