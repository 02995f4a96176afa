"""Host reference of temporal reprojection (include/myraytracer_amd.h, "temporal reprojection"): one step of the history, its
variance and the filter over it, restated in float32 numpy in the library's operation order (temporal.hip and denoise.hip are
built with -ffp-contract=off, so every step is one correctly rounded float32 operation), and a plain float64 per-pixel form of
the step that the float32 one is checked against (tests/test_temporal_host.py).

Arrays: cur (H, W, 4) the framebuffer; rays (H, W, 6), index (H, W) i32, t (H, W) the guides (State.debug_read_guides); xyzr1 /
xyzr0 (n, 4) the spheres as they are / as they were at the previous step; M (3, 3), o_prev (3,) from camera_matrix() of the
previous derived camera; h0 = (r, g, b, len), h1 = (m1, m2, t, index bits), (H, W, 4) each."""
import math

import numpy as np

from denoise_ref import DEFAULTS, EPS, F, KERN, _shift, lum, tukey
from denoise_var_ref import _stops, prefiltered_var, spatial_variance

T_DEFAULTS = {"max_history": 32, "spatial_len": 4, "depth_tol": 0.05}
BROKEN = ("no_scale", "tap_order", "depth_t")      # references broken on purpose (tests/test_temporal_host.py)


def camera_matrix(raw=None):
    """(M, o') of a derived camera (an object with mode, origin, su, sv, fw; None: the pinhole): the inverse of the matrix with
    the columns su, sv, -fw by cofactors in double, rounded to float32 -- the host's own expression, operation for operation."""
    A = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]]
    o = np.zeros(3, F)
    if raw is not None and raw.mode != 0:
        for k in range(3):
            A[k] = [float(raw.su[k]), float(raw.sv[k]), -float(raw.fw[k])]
            o[k] = raw.origin[k]
    C = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            C[i][j] = A[i1][j1] * A[i2][j2] - A[i1][j2] * A[i2][j1]
    det = (A[0][0] * C[0][0] + A[0][1] * C[0][1]) + A[0][2] * C[0][2]
    M = np.array([[C[j][i] / det for j in range(3)] for i in range(3)], np.float64).astype(F)
    return M, o


def index_bits(index):
    return np.ascontiguousarray(index, np.int32).view(F)


def step(cur, rays, index, t, xyzr1, xyzr0, M, o_prev, h0, h1, params=None, broken=None):
    """One mrt_temporal_step: (h0', h1', info), bit for bit what the device computes.  info: "taps" (H, W, 4) bool, the taps that
    counted (j then i), "found" = any of them, "finite" = cur's colour is finite."""
    assert broken is None or broken in BROKEN
    p = dict(T_DEFAULTS, **(params or {}))
    cur = np.asarray(cur, F)
    rays = np.asarray(rays, F)
    t = np.asarray(t, F)
    s = np.ascontiguousarray(index, np.int32)
    h0 = np.asarray(h0, F)
    h1 = np.asarray(h1, F)
    xyzr1 = np.asarray(xyzr1, F).reshape(-1, 4)
    xyzr0 = np.asarray(xyzr0, F).reshape(-1, 4)
    M = np.asarray(M, F)
    o_prev = np.asarray(o_prev, F)
    H, W = s.shape
    Hf, Wf = F(H), F(W)
    hit = s >= 0
    si = np.where(hit, s, 0)
    sbits = h1[..., 3].view(np.int32)
    with np.errstate(all="ignore"):
        o, d = rays[..., 0:3], rays[..., 3:6]
        X = o + t[..., None] * d
        k = xyzr0[si, 3] / xyzr1[si, 3]
        if broken == "no_scale":
            k = np.ones_like(k)
        Xp = np.where(hit[..., None], xyzr0[si, :3] + (X - xyzr1[si, :3]) * k[..., None], o_prev + d).astype(F)
        v = Xp - o_prev
        a, b, l = ((M[r, 0] * v[..., 0] + M[r, 1] * v[..., 1]) + M[r, 2] * v[..., 2] for r in range(3))
        front = l > 0
        fx = (a / l) * (F(0.5) * Hf) + (F(0.5) * Wf - F(1))
        fy = (b / l) * (F(0.5) * Hf) + (F(0.5) * Hf - F(1))
        te = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        tol = F(p["depth_tol"]) * te
        x0, y0 = np.floor(fx), np.floor(fy)
        wx, wy = fx - x0, fy - y0
        sw = np.zeros((H, W), F)
        sc = np.zeros((H, W, 3), F)
        s1 = np.zeros((H, W), F)
        s2 = np.zeros((H, W), F)
        lmin = np.full((H, W), np.inf, F)
        taps = np.zeros((H, W, 4), bool)
        for j, i in [(j, i) for j in (0, 1) for i in (0, 1)]:
            xq, yq = x0 + F(i), y0 + F(j)
            inside = (xq >= 0) & (xq < Wf) & (yq >= 0) & (yq < Hf)
            bi, bj = (j, i) if broken == "tap_order" else (i, j)
            bw = (wx if bi else F(1) - wx) * (wy if bj else F(1) - wy)
            xi = np.where(inside, xq, F(0)).astype(np.int64)
            yi = np.where(inside, yq, F(0)).astype(np.int64)
            q0, q1, qs = h0[yi, xi], h1[yi, xi], sbits[yi, xi]
            depth = np.abs(q1[..., 2] - (t if broken == "depth_t" else te)) <= tol
            cnt = (front & inside & (bw > 0) & (q0[..., 3] >= 1) & np.isfinite(q0[..., :3]).all(-1) & (qs == s) & (~hit | depth))
            taps[..., 2 * j + i] = cnt
            sw = sw + np.where(cnt, bw, F(0))
            sc = sc + np.where(cnt[..., None], bw[..., None] * q0[..., :3], F(0))
            s1 = s1 + np.where(cnt, bw * q1[..., 0], F(0))
            s2 = s2 + np.where(cnt, bw * q1[..., 1], F(0))
            lmin = np.where(cnt, np.fmin(lmin, q0[..., 3]), lmin)
        Lc = lum(cur)
        found = sw > 0
        cp, m1p, m2p = sc / sw[..., None], s1 / sw, s2 / sw
        N = np.fmin(lmin + F(1), F(p["max_history"]))
        alpha = F(1) / N
        c_hist = cp + alpha[..., None] * (cur[..., :3] - cp)
        m1_hist = m1p + alpha * (Lc - m1p)
        m2_hist = m2p + alpha * (Lc * Lc - m2p)
        fin = np.isfinite(cur[..., :3]).all(-1)
        found = found & fin
        o0 = np.empty((H, W, 4), F)
        o1 = np.empty((H, W, 4), F)
        o0[..., :3] = np.where(found[..., None], c_hist, cur[..., :3])
        o0[..., 3] = np.where(fin, np.where(found, N, F(1)), F(0))
        o1[..., 0] = np.where(fin, np.where(found, m1_hist, Lc), F(0))
        o1[..., 1] = np.where(fin, np.where(found, m2_hist, Lc * Lc), F(0))
        o1[..., 2] = t
        o1[..., 3] = index_bits(s)
    taps &= fin[..., None]
    return o0, o1, {"taps": taps, "found": found, "finite": fin}


def step_f64(cur, rays, index, t, xyzr1, xyzr0, M, o_prev, h0, h1, params=None):
    """The same definition per pixel in float64 (no float32 rounding): (h0', h1' without the index bits, taps)."""
    p = dict(T_DEFAULTS, **(params or {}))
    s = np.asarray(index, np.int32)
    H, W = s.shape
    cur, rays, t = (np.asarray(a, np.float64) for a in (cur, rays, t))
    x1, x0_ = np.asarray(xyzr1, np.float64).reshape(-1, 4), np.asarray(xyzr0, np.float64).reshape(-1, 4)
    M, o_prev = np.asarray(M, np.float64), np.asarray(o_prev, np.float64)
    g0, g1 = np.asarray(h0, np.float64), np.asarray(h1, np.float64)
    gbits = np.asarray(h1, F)[..., 3].view(np.int32)
    L = lambda c: (0.2126 * c[0] + 0.7152 * c[1]) + 0.0722 * c[2]
    o0 = np.zeros((H, W, 4))
    o1 = np.zeros((H, W, 3))
    taps = np.zeros((H, W, 4), bool)
    for y in range(H):
        for x in range(W):
            c = cur[y, x, :3]
            o1[y, x, 2] = t[y, x]
            if not np.isfinite(c).all():
                o0[y, x, :3] = c
                continue
            o, d = rays[y, x, :3], rays[y, x, 3:]
            k = int(s[y, x])
            if k >= 0:
                Xp = x0_[k, :3] + (o + t[y, x] * d - x1[k, :3]) * (x0_[k, 3] / x1[k, 3])
            else:
                Xp = o_prev + d
            v = Xp - o_prev
            a, b, l = M @ v
            sw, sc, s1, s2, lmin = 0.0, np.zeros(3), 0.0, 0.0, math.inf
            if l > 0:
                fx = a / l * 0.5 * H + 0.5 * W - 1
                fy = b / l * 0.5 * H + 0.5 * H - 1
                te = math.sqrt(float(v @ v))
                fx0, fy0 = math.floor(fx), math.floor(fy)
                wx, wy = fx - fx0, fy - fy0
                for j in (0, 1):
                    for i in (0, 1):
                        xq, yq = fx0 + i, fy0 + j
                        bw = (wx if i else 1 - wx) * (wy if j else 1 - wy)
                        if not (0 <= xq < W and 0 <= yq < H) or not bw > 0:
                            continue
                        q0, q1 = g0[yq, xq], g1[yq, xq]
                        if not q0[3] >= 1 or not np.isfinite(q0[:3]).all() or gbits[yq, xq] != k:
                            continue
                        if k >= 0 and not abs(q1[2] - te) <= p["depth_tol"] * te:
                            continue
                        taps[y, x, 2 * j + i] = True
                        sw += bw
                        sc += bw * q0[:3]
                        s1 += bw * q1[0]
                        s2 += bw * q1[1]
                        lmin = min(lmin, q0[3])
            Lc = L(c)
            if sw > 0:
                N = min(lmin + 1, p["max_history"])
                cp, m1p, m2p = sc / sw, s1 / sw, s2 / sw
                o0[y, x, :3] = cp + (c - cp) / N
                o0[y, x, 3] = N
                o1[y, x, 0] = m1p + (Lc - m1p) / N
                o1[y, x, 1] = m2p + (Lc * Lc - m2p) / N
            else:
                o0[y, x, :3] = c
                o0[y, x, 3] = 1
                o1[y, x, 0], o1[y, x, 1] = Lc, Lc * Lc
    return o0, o1, taps


def variance_field(h0, h1, guides, dparams=None, spatial_len=4):
    """(r, g, b, var), the filter's input: the history's own moments where it is long enough, else the spatial estimate."""
    h0 = np.asarray(h0, F)
    h1 = np.asarray(h1, F)
    with np.errstate(all="ignore"):
        N = h0[..., 3]
        long_ = N >= F(max(2, spatial_len))
        var_m = np.fmax(F(0), h1[..., 1] - h1[..., 0] * h1[..., 0]) / (N - F(1))
        has = N >= F(1)
        sp = spatial_variance(h0, np.where(has, F(0), F(np.nan)).astype(F), guides, dparams)
        short = has & np.isfinite(h0[..., :3]).all(-1)
        cv = h0.copy()
        cv[..., 3] = np.where(long_, var_m, np.where(short, sp, F(0)))
    return cv


def filter_field(cv, alpha, guides, dparams=None):
    """The denoiser's prefiltering iterations over a given (r, g, b, var) field (denoise_var_ref.denoise_var's loop as its
    variance 2 runs it: luminance stop on, every iteration prefiltered); alpha: the framebuffer's."""
    p = dict(DEFAULTS, **(dparams or {}))
    cv = np.asarray(cv, F).copy()
    shape = cv.shape[:2]
    sl = F(p["sigma_l"])
    stops = _stops(guides, p)
    with np.errstate(all="ignore"):
        for it in range(p["iterations"]):
            h = 1 << it
            fin = np.isfinite(cv).all(-1)
            g = prefiltered_var(cv, fin)
            active = fin & ~(g == 0)
            lp = lum(cv)
            inv_l = (F(1) / (sl * np.sqrt(g) + EPS)).astype(F)
            sw = np.zeros(shape, F)
            sc = np.zeros(shape + (3,), F)
            sv = np.zeros(shape, F)
            for ty in range(5):
                for tx in range(5):
                    dy, dx = (ty - 2) * h, (tx - 2) * h
                    kxy = KERN[tx] * KERN[ty]
                    if dx == 0 and dy == 0:
                        w = np.full(shape, kxy, F)
                        cq = cv
                    else:
                        cq = _shift(cv, dy, dx, F(0))
                        valid = _shift(fin, dy, dx, False)
                        wl = tukey(np.abs(lp - lum(cq)) * inv_l)
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
    out[..., 3] = alpha
    return out


def image(h0, h1, alpha, guides, dparams=None, spatial_len=4):
    """mrt_read_temporal's image of a history."""
    return filter_field(variance_field(h0, h1, guides, dparams, spatial_len), alpha, guides, dparams)
