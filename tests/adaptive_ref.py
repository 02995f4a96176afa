"""Host reference of adaptive sampling (include/myraytracer_amd.h, "adaptive sampling"), in float32 numpy on top of
tests/noise_ref.py: every 8x8 tile has its own frame count n_t; a frame blends the listed tiles (all tiles for a whole frame) at
w = mrt_frame_weight(n_t, max_w) with the same blend and S recursion as a uniform frame; the report takes K(n_t) per pixel; the
tile map and the selection render_adaptive makes from it."""
import math

import numpy as np

import noise_ref

F = np.float32
TILE = 8


def frame_weight(n: int, max_w: float) -> np.float32:
    """mrt_frame_weight(n, max_w): 0 at n == 0, else min(max_w, (float)n / (float)(n + 1)) (u32 wrap at UINT32_MAX)."""
    if n == 0:
        return F(0)
    with np.errstate(divide="ignore"):
        w = F(n) / F((n + 1) & 0xFFFFFFFF)
    return F(max_w) if F(max_w) < w else w


def k_table(n_max: int, max_w: float) -> list:
    """K(n) for n = 0 .. n_max: c2 over the float weights of frames 0 .. n - 1 (noise_ref.c2_next), K = c2 / (1 - c2)."""
    out, c2 = [], 1.0
    for n in range(n_max + 1):
        out.append(noise_ref.factor(c2))
        c2 = noise_ref.c2_next(c2, frame_weight(n, max_w))
    return out


def tile_of(rows: int, width: int) -> np.ndarray:
    """(rows, width) -> the tile id of every pixel: band * tiles_x + column."""
    tx = -(-width // TILE)
    y, x = np.mgrid[0:rows, 0:width]
    return (y // TILE) * tx + x // TILE


class Accum:
    """The framebuffer, S and n_t of one context (world 1), blended frame by frame."""

    def __init__(self, height: int, width: int, max_w: float):
        self.h, self.w, self.max_w = height, width, max_w
        self.tx, self.tr = -(-width // TILE), -(-height // TILE)
        self.fb = np.zeros((height, width, 4), np.float32)
        self.S = np.zeros((height, width), np.float32)
        self.n = np.zeros(self.tr * self.tx, np.int64)
        self.frames_done = 0
        self.diverged = False                      # a subset frame since the last reset: blends and reports are per tile
        self.tile = tile_of(height, width)

    def reset(self):
        """mrt_reset: framebuffer, S and every n_t zero, the accumulation uniform again."""
        self.fb[:] = 0
        self.S[:] = 0
        self.n[:] = 0
        self.frames_done = 0
        self.diverged = False

    def load(self, fb: np.ndarray, S: np.ndarray, n):
        """mrt_debug_load_accumulation with all three parts: the framebuffer, S and n_t per tile as given, the accumulation
        adaptive from here on."""
        assert fb.shape == self.fb.shape and S.shape == self.S.shape and np.size(n) == self.n_tiles
        self.fb, self.S = np.array(fb, np.float32), np.array(S, np.float32)
        self.n = np.asarray(n, np.int64).reshape(-1).copy()
        self.diverged = True

    @property
    def n_tiles(self) -> int:
        return self.tr * self.tx

    def frame(self, mean: np.ndarray, tiles=None):
        """Blend one frame's mean (H, W, 4) into the listed tiles (None: every tile) at their own weights."""
        listed = np.ones(self.n_tiles, bool) if tiles is None else np.isin(np.arange(self.n_tiles), np.asarray(tiles, np.int64))
        self.diverged = self.diverged or not listed.all()
        wt = np.array([frame_weight(int(k), self.max_w) for k in self.n], np.float32)
        for t in np.unique(wt[listed]):            # tiles that share a weight share one vectorised blend
            m = listed[self.tile] & (wt[self.tile] == t)
            self.S[m] = noise_ref.s_update(self.S[m], mean[m], self.fb[m], t)
            self.fb[m] = noise_ref.blend(mean[m], self.fb[m], t)
        self.n[listed] = np.minimum(self.n[listed] + 1, 0xFFFFFFFF)
        self.frames_done = min(self.frames_done + 1, 0xFFFFFFFF)

    def tile_frames(self) -> np.ndarray:
        return self.n.reshape(self.tr, self.tx).astype(np.uint32)

    def k_per_pixel(self):
        """(K per tile as float64, the report's noise_factor: the largest)."""
        table = k_table(int(self.n.max()), self.max_w)
        kt = np.array([table[k] for k in self.n], np.float64)
        return kt, float(kt.max())

    def report(self, threshold: float = 0.02, floor: float = 0.01, diverged: bool = True) -> dict:
        """The report of the current state.  diverged=False: the uniform report (noise_ref.report with K(frames_done))."""
        if not diverged:
            return noise_ref.report(self.S, self.fb, k_table(self.frames_done, self.max_w)[-1], threshold, floor)
        kt, kmax = self.k_per_pixel()
        finite, se, L, rel, above = self.per_pixel(kt, threshold, floor)
        n = int(finite.sum())
        sum_l = math.fsum(L[finite].astype(np.float64))
        out = {"pixels": n, "non_finite": int((~finite).sum()), "above": int(above.sum()), "noise_factor": kmax, "sum_lum": sum_l}
        if math.isinf(kmax):
            out.update(sum_var=math.inf, rmse=math.inf, rel_rmse=math.inf, max_se=math.inf)
            return out
        kp = kt[self.tile]
        out["sum_var"] = math.fsum((self.S[finite].astype(np.float64) * kp[finite]).tolist())
        out["max_se"] = float(np.max(se[finite], initial=np.float32(0)))
        out["rmse"] = math.sqrt(out["sum_var"] / n) if n else 0.0
        mean_l = sum_l / n if n else 0.0
        out["rel_rmse"] = 0.0 if out["rmse"] <= 0.0 else (out["rmse"] / mean_l if mean_l else math.inf)
        return out

    def per_pixel(self, kt, threshold, floor):
        """noise_ref.per_pixel with K per tile: var = S * (float)K_t, K_t = +inf -> se = +inf."""
        kp = kt[self.tile]
        L = noise_ref.lum(self.fb)
        with np.errstate(all="ignore"):
            finite = np.isfinite(self.S) & np.isfinite(L)
            se = np.where(np.isinf(kp), np.float32(np.inf), np.sqrt(self.S * kp.astype(np.float32))).astype(np.float32)
            rel = se / np.fmax(L, F(floor))
            above = finite & (rel > F(threshold))
        return finite, se, L, rel, above

    def tiles(self, threshold: float = 0.02, floor: float = 0.01, diverged: bool = True) -> np.ndarray:
        """The report's tile map: the per-8x8-tile maximum of rel over finite pixels (NaN ignored, 0 for none)."""
        if not diverged:
            return noise_ref.tiles(self.S, self.fb, k_table(self.frames_done, self.max_w)[-1], threshold, floor)
        kt, _ = self.k_per_pixel()
        finite, se, L, rel, above = self.per_pixel(kt, threshold, floor)
        v = np.where(finite & ~np.isnan(rel), rel, np.float32(0)).astype(np.float32)
        pad = np.zeros((self.tr * TILE, self.tx * TILE), np.float32)
        pad[:self.h, :self.w] = v
        return pad.reshape(self.tr, TILE, self.tx, TILE).max(axis=(1, 3))


def select(tile_map: np.ndarray, threshold: float) -> np.ndarray:
    """render_adaptive's selection: the tiles whose map entry is > the report's threshold, in id order."""
    return np.nonzero(np.asarray(tile_map, np.float32).ravel() > F(threshold))[0].astype(np.uint32)
