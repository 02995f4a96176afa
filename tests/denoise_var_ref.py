"""Host reference of the denoiser's variance modes (include/myraytracer_amd.h, "Variance modes"): the prefiltered luminance stop
and the spatial initial variance, restated in float32 numpy in the library's operation order on top of tests/denoise_ref.py, and a
plain float64 per-pixel form of the same definition that the float32 one is checked against (tests/test_denoise_var_host.py).

`variance` is mrt_debug_denoise_variance's: 0 accumulated (denoise_ref.denoise exactly), 1 prefiltered, 2 prefiltered with the
spatial initial variance (K is not read)."""
import math

import numpy as np

from denoise_ref import DEFAULTS, EPS, F, KERN, _shift, lum, tukey

K3 = np.array([1 / 4, 1 / 2, 1 / 4], F)
MODES = ("accumulated", "prefiltered", "spatial-early")


def variance_of(mode, frames_done, spatial_frames=3):
    """The `variance` a context in `mode` (0 .. 2) denoises its frames_done-th frame with."""
    if mode == 2:
        return 2 if frames_done < spatial_frames else 1
    return mode


def _stops(guides, p):
    """(dy, dx) -> (w_normal, w_depth, w_albedo) of the tap p + (dy, dx), float32, as the filter forms them."""
    sz, sa = F(p["sigma_z"]), F(p["sigma_a"])
    inv_a = F(1) / sa
    n = np.asarray(guides["normal"], F)
    t = np.asarray(guides["t"], F)
    alb = np.asarray(guides["albedo"], F)
    miss = np.asarray(guides["index"]) < 0
    with np.errstate(all="ignore"):
        inv_z = np.where(miss, F(0), F(1) / (sz * t)).astype(F)

    def at(dy, dx):
        nq = _shift(n, dy, dx, F(0))
        wn = np.fmax(F(0), (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
        for _ in range(p["normal_exp"]):
            wn = wn * wn
        mq = _shift(miss, dy, dx, False)
        tq = _shift(t, dy, dx, F(0))
        wz = np.where(miss != mq, F(0), np.where(miss, F(1), tukey(np.abs(t - tq) * inv_z))).astype(F)
        aq = _shift(alb, dy, dx, F(0))
        da = np.fmax(np.fmax(np.abs(alb[..., 0] - aq[..., 0]), np.abs(alb[..., 1] - aq[..., 1])), np.abs(alb[..., 2] - aq[..., 2]))
        return wn.astype(F), wz, tukey(da * inv_a)
    return at


def prefiltered_var(cv, fin):
    """g_p: the {1/4, 1/2, 1/4}^2 mean of var over the finite texels of the 3 x 3 window (meaningful where fin)."""
    num = np.zeros(fin.shape, F)
    den = np.zeros(fin.shape, F)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            k = K3[dx + 1] * K3[dy + 1]
            valid = _shift(fin, dy, dx, False)
            vq = np.where(valid, _shift(cv[..., 3], dy, dx, F(0)), F(0)).astype(F)
            num = num + np.where(valid, k * vq, F(0)).astype(F)
            den = den + np.where(valid, k, F(0)).astype(F)
    return (num / den).astype(F)


def spatial_variance(rgba, S, guides, params=None):
    """Iteration 0's var of the spatial estimate: the weighted variance of L over the 7 x 7 window, float32 [rows, W]."""
    p = dict(DEFAULTS, **(params or {}))
    rgba = np.asarray(rgba, F)
    S = np.asarray(S, F)
    stops = _stops(guides, p)
    with np.errstate(all="ignore"):
        sfin = np.isfinite(S)
        ok = np.isfinite(rgba[..., :3]).all(-1) & sfin
        L = lum(rgba)
        taps = []
        m0 = np.zeros(S.shape, F)
        m1 = np.zeros(S.shape, F)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                if dx == 0 and dy == 0:
                    valid, w, lq = ok, np.ones(S.shape, F), L
                else:
                    valid = _shift(ok, dy, dx, False)
                    wn, wz, wa = stops(dy, dx)
                    w = (wn * wz) * wa
                    lq = _shift(L, dy, dx, F(0))
                w = np.where(valid, w, F(0)).astype(F)
                lq = np.where(valid, lq, F(0)).astype(F)
                taps.append((valid, w, lq))
                m0 = m0 + w
                m1 = m1 + w * lq
        mean = m1 / m0
        m2 = np.zeros(S.shape, F)
        for valid, w, lq in taps:
            d = lq - mean
            m2 = m2 + np.where(valid, w * (d * d), F(0)).astype(F)
        var = m2 / m0
        return np.where(ok, var, np.where(sfin, F(0), S)).astype(F)


def denoise_var(rgba, S, K, guides, params=None, variance=0):
    """denoise_ref.denoise with a variance estimate: bit for bit what mrt_debug_denoise_variance computes."""
    p = dict(DEFAULTS, **(params or {}))
    rgba = np.asarray(rgba, F)
    S = np.asarray(S, F)
    spatial = variance == 2
    lum_stop = spatial or not math.isinf(K)
    prefilter = variance != 0 and lum_stop
    sl = F(p["sigma_l"])
    stops = _stops(guides, p)
    with np.errstate(all="ignore"):
        cv = np.empty(rgba.shape, F)
        cv[..., :3] = rgba[..., :3]
        if spatial:
            cv[..., 3] = spatial_variance(rgba, S, guides, p)
        else:
            cv[..., 3] = S * F(K) if lum_stop else np.where(np.isfinite(S), F(0), S)
        for it in range(p["iterations"]):
            h = 1 << it
            fin = np.isfinite(cv).all(-1)
            g = prefiltered_var(cv, fin) if prefilter else cv[..., 3]
            active = fin & ~(lum_stop & (g == 0))
            lp = lum(cv)
            inv_l = (F(1) / (sl * np.sqrt(g) + EPS)).astype(F) if lum_stop else None
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
                        wl = tukey(np.abs(lp - lum(cq)) * inv_l) if lum_stop else F(1)
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


def denoise_var_f64(rgba, S, K, guides, params=None, variance=0):
    """The same definition per pixel in float64 (no float32 rounding): what denoise_var() approximates."""
    p = dict(DEFAULTS, **(params or {}))
    rows, width = S.shape
    spatial = variance == 2
    lum_stop = spatial or not math.isinf(K)
    prefilter = variance != 0 and lum_stop
    k = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    k3 = [1 / 4, 1 / 2, 1 / 4]
    tk = lambda x: (1 - x * x) ** 2 if x < 1 else 0.0
    L = lambda c: (0.2126 * c[0] + 0.7152 * c[1]) + 0.0722 * c[2]
    n = np.asarray(guides["normal"], np.float64)
    t = np.asarray(guides["t"], np.float64)
    alb = np.asarray(guides["albedo"], np.float64)
    miss = np.asarray(guides["index"]) < 0
    inside = lambda y, x: 0 <= y < rows and 0 <= x < width

    def edge_stops(y, x, yq, xq):
        wn = max(0.0, float(n[y, x] @ n[yq, xq])) ** (2 ** p["normal_exp"])
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
    with np.errstate(all="ignore"):
        if spatial:
            ok = np.isfinite(cv[..., :3]).all(-1) & np.isfinite(S64)
            var = np.where(np.isfinite(S64), 0.0, S64)
            for y in range(rows):
                for x in range(width):
                    if not ok[y, x]:
                        continue
                    taps = [(1.0 if (dy, dx) == (0, 0) else edge_stops(y, x, y + dy, x + dx), L(cv[y + dy, x + dx]))
                            for dy in range(-3, 4) for dx in range(-3, 4) if inside(y + dy, x + dx) and ok[y + dy, x + dx]]
                    m0 = sum(w for w, _ in taps)
                    mean = sum(w * l for w, l in taps) / m0
                    var[y, x] = sum(w * (l - mean) ** 2 for w, l in taps) / m0
            cv[..., 3] = var
        else:
            cv[..., 3] = S64 * float(F(K)) if lum_stop else np.where(np.isfinite(S), 0.0, S)
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
                if prefilter:
                    near = [(k3[dx + 1] * k3[dy + 1], cv[y + dy, x + dx, 3]) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                            if inside(y + dy, x + dx) and fin[y + dy, x + dx]]
                    g = sum(w * v for w, v in near) / sum(w for w, _ in near)
                if lum_stop and g == 0:
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
                            wl = tk(abs(L(c) - L(q)) / (p["sigma_l"] * math.sqrt(g) + 1e-6)) if lum_stop else 1.0
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
