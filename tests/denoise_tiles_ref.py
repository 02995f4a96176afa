"""Host reference of the denoise of an adaptive accumulation (include/myraytracer_amd.h, "Adaptive accumulations"): every 8 x 8 tile
has its own frame count n_t, hence its own K and its own choice between the spatial estimate and S * K.  Restated in float32 numpy
in the library's operation order on top of tests/denoise_var_ref.py, and a plain float64 per-pixel form of the same rule that the
float32 one is checked against (tests/test_denoise_tiles_host.py).

`mode` is mrt_set_denoise_variance's (0 accumulated, 1 prefiltered, 2 spatial-early); `tile_frames` the map of n_t, (tile rows,
tiles_x) or flat; `k_of(n)` gives K(n) (default: mrt_noise_factor(n, max_w) through the library's host-only entry point)."""
import math

import numpy as np

from denoise_ref import DEFAULTS, EPS, F, KERN, _shift, lum, tukey
from denoise_var_ref import _stops, prefiltered_var, spatial_variance

TILE = 8


def pixel_frames(tile_frames, rows, width):
    """n_p per pixel: tile (y // 8) * tiles_x + x // 8."""
    tx, ty = (width + TILE - 1) // TILE, (rows + TILE - 1) // TILE
    t = np.asarray(tile_frames, np.uint32).reshape(ty, tx)
    return np.repeat(np.repeat(t, TILE, axis=0), TILE, axis=1)[:rows, :width]


def library_k(max_w=1.0):
    from myraytracer_amd import api
    return lambda n: api.noise_factor(int(n), max_w)


def pixel_state(tile_frames, rows, width, mode, spatial_frames, k_of):
    """(K_p as float32, spatial_p, stop_p) per pixel."""
    n = pixel_frames(tile_frames, rows, width)
    table = {int(v): F(k_of(int(v))) for v in np.unique(n)}
    K = np.vectorize(lambda v: table[int(v)], otypes=[F])(n)
    spatial = (n < spatial_frames) if mode == 2 else np.zeros(n.shape, bool)
    return K, spatial, spatial | np.isfinite(K)


def initial_variance(rgba, S, guides, p, K, spatial):
    """Iteration 0's var per pixel, float32."""
    with np.errstate(all="ignore"):
        kfin = np.isfinite(K)
        var = np.where(kfin, S * np.where(kfin, K, F(0)).astype(F), np.where(np.isfinite(S), F(0), S)).astype(F)
        if spatial.any():
            var = np.where(spatial, spatial_variance(rgba, S, guides, p), var).astype(F)
    return var


def denoise_tiles(rgba, S, tile_frames, guides, params=None, mode=0, spatial_frames=3, k_of=None):
    """Bit for bit what mrt_read_denoised computes for a diverged accumulation with mrt_set_denoise_adaptive on."""
    p = dict(DEFAULTS, **(params or {}))
    rgba = np.asarray(rgba, F)
    S = np.asarray(S, F)
    rows, width = S.shape
    K, spatial, stop = pixel_state(tile_frames, rows, width, mode, spatial_frames, k_of or library_k())
    prefilter = mode != 0
    sl = F(p["sigma_l"])
    stops = _stops(guides, p)
    with np.errstate(all="ignore"):
        cv = np.empty(rgba.shape, F)
        cv[..., :3] = rgba[..., :3]
        cv[..., 3] = initial_variance(rgba, S, guides, p, K, spatial)
        for it in range(p["iterations"]):
            h = 1 << it
            fin = np.isfinite(cv).all(-1)
            g = np.where(stop, prefiltered_var(cv, fin), cv[..., 3]).astype(F) if prefilter else cv[..., 3]
            active = fin & ~(stop & (g == 0))
            lp = lum(cv)
            inv_l = (F(1) / (sl * np.sqrt(g) + EPS)).astype(F)
            sw = np.zeros(S.shape, F)
            sc = np.zeros(S.shape + (3,), F)
            sv = np.zeros(S.shape, F)
            for ty in range(5):
                for tx in range(5):
                    dy, dx = (ty - 2) * h, (tx - 2) * h
                    kxy = KERN[tx] * KERN[ty]
                    if dx == 0 and dy == 0:
                        w = np.full(S.shape, kxy, F)
                        cq = cv
                    else:
                        cq = _shift(cv, dy, dx, F(0))
                        valid = _shift(fin, dy, dx, False)
                        wl = np.where(stop, tukey(np.abs(lp - lum(cq)) * inv_l), F(1)).astype(F)      # the centre decides
                        wn, wz, wa = stops(dy, dx)
                        w = kxy * wl
                        w = (w * wn).astype(F)
                        w = w * wz
                        w = w * wa
                        w = np.where(valid, w, F(0)).astype(F)
                        cq = np.where(valid[..., None], cq, F(0)).astype(F)
                    sw = sw + w
                    sc = sc + w[..., None] * cq[..., :3]
                    sv = sv + (w * w) * cq[..., 3]
            res = np.empty_like(cv)
            res[..., :3] = sc / sw[..., None]
            res[..., 3] = sv / (sw * sw)
            cv = np.where(active[..., None], res, cv).astype(F)
    out = cv.copy()
    out[..., 3] = rgba[..., 3]
    return out


def denoise_tiles_f64(rgba, S, tile_frames, guides, params=None, mode=0, spatial_frames=3, k_of=None):
    """The same rule per pixel in float64 (no float32 rounding): what denoise_tiles() approximates."""
    p = dict(DEFAULTS, **(params or {}))
    rows, width = S.shape
    k_of = k_of or library_k()
    n = pixel_frames(tile_frames, rows, width)
    k = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    k3 = [1 / 4, 1 / 2, 1 / 4]
    tk = lambda x: (1 - x * x) ** 2 if x < 1 else 0.0
    L = lambda c: (0.2126 * c[0] + 0.7152 * c[1]) + 0.0722 * c[2]
    nrm = np.asarray(guides["normal"], np.float64)
    t = np.asarray(guides["t"], np.float64)
    alb = np.asarray(guides["albedo"], np.float64)
    miss = np.asarray(guides["index"]) < 0
    inside = lambda y, x: 0 <= y < rows and 0 <= x < width

    def edge_stops(y, x, yq, xq):
        wn = max(0.0, float(nrm[y, x] @ nrm[yq, xq])) ** (2 ** p["normal_exp"])
        if miss[y, x] != miss[yq, xq]:
            wz = 0.0
        elif miss[y, x]:
            wz = 1.0
        else:
            wz = tk(abs(t[y, x] - t[yq, xq]) / (p["sigma_z"] * t[y, x]))
        wa = tk(float(np.max(np.abs(alb[y, x] - alb[yq, xq]))) / p["sigma_a"])
        return wn * wz * wa

    S64 = np.asarray(S, np.float64)
    cv = np.empty((rows, width, 4))
    cv[..., :3] = rgba[..., :3]
    ok = np.isfinite(cv[..., :3]).all(-1) & np.isfinite(S64)
    stop = np.zeros((rows, width), bool)
    with np.errstate(all="ignore"):
        for y in range(rows):
            for x in range(width):
                Kp = float(F(k_of(int(n[y, x]))))
                spatial = mode == 2 and n[y, x] < spatial_frames
                stop[y, x] = spatial or math.isfinite(Kp)
                s = S64[y, x]
                if not spatial:
                    cv[y, x, 3] = s * Kp if math.isfinite(Kp) else (0.0 if math.isfinite(s) else s)
                elif not ok[y, x]:
                    cv[y, x, 3] = 0.0 if math.isfinite(s) else s
                else:
                    taps = [(1.0 if (dy, dx) == (0, 0) else edge_stops(y, x, y + dy, x + dx), L(cv[y + dy, x + dx]))
                            for dy in range(-3, 4) for dx in range(-3, 4) if inside(y + dy, x + dx) and ok[y + dy, x + dx]]
                    m0 = sum(w for w, _ in taps)
                    mean = sum(w * l for w, l in taps) / m0
                    cv[y, x, 3] = sum(w * (l - mean) ** 2 for w, l in taps) / m0
    for it in range(p["iterations"]):
        h = 1 << it
        nxt = cv.copy()
        fin = np.isfinite(cv).all(-1)
        for y in range(rows):
            for x in range(width):
                c = cv[y, x]
                if not fin[y, x]:
                    continue
                g = c[3]
                if mode != 0 and stop[y, x]:
                    near = [(k3[dx + 1] * k3[dy + 1], cv[y + dy, x + dx, 3]) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                            if inside(y + dy, x + dx) and fin[y + dy, x + dx]]
                    g = sum(w * v for w, v in near) / sum(w for w, _ in near)
                if stop[y, x] and g == 0:
                    continue
                sw = sv = 0.0
                sc = np.zeros(3)
                for ty in range(5):
                    for tx in range(5):
                        yq, xq = y + (ty - 2) * h, x + (tx - 2) * h
                        if not inside(yq, xq) or not fin[yq, xq]:
                            continue
                        q = cv[yq, xq]
                        w = k[tx] * k[ty]
                        if (yq, xq) != (y, x):
                            wl = tk(abs(L(c) - L(q)) / (p["sigma_l"] * math.sqrt(g) + 1e-6)) if stop[y, x] else 1.0
                            w *= wl * edge_stops(y, x, yq, xq)
                        sw += w
                        sc += w * q[:3]
                        sv += w * w * q[3]
                nxt[y, x, :3] = sc / sw
                nxt[y, x, 3] = sv / (sw * sw)
        cv = nxt
    out = cv.copy()
    out[..., 3] = rgba[..., 3]
    return out


def tile_map(rng, rows, width, values):
    """A map of n_t that holds every value of `values` at least once where there are tiles enough, the rest drawn from them."""
    tx, ty = (width + TILE - 1) // TILE, (rows + TILE - 1) // TILE
    values = np.asarray(values, np.uint32)
    m = rng.choice(values, size=tx * ty).astype(np.uint32)
    slots = rng.permutation(tx * ty)[:len(values)]
    m[slots] = values[:len(slots)]
    return m.reshape(ty, tx)
