"""Host reference of the temporal response (include/myraytracer_amd.h, "temporal reprojection", steps 3 and 4 with the fast history
H2, 4b the clamp, 4c the anti-lag): one mrt_temporal_step with the response on, restated in float32 numpy in the library's
operation order (temporal.hip is built with -ffp-contract=off), and a plain float64 per-pixel form of the same definition that
the float32 one is checked against (tests/test_temporal_response_host.py).  The reprojection's geometry is restated here as
tests/temporal_ref.py states it (that file is imported, not edited): with a clamp that never acts, H0' and H1' must be
temporal_ref.step's bit for bit, which the host test asserts.

Arrays as in temporal_ref; h2 = (fr, fg, fb, valid), (H, W, 4)."""
import math

import numpy as np

from denoise_ref import F, _shift, lum
from temporal_ref import T_DEFAULTS, index_bits

R_DEFAULTS = {"fast_history": 4, "clamp_sigma": 2.0, "antilag": 1.0}
BROKEN = ("window_order", "sample_variance", "no_halo")     # references broken on purpose (tests/test_temporal_response_host.py)
TILE_W, TILE_H, HALO = 32, 8, 2                             # temporal_clamp_kernel's tiles and its window's reach
WINDOW = [(dy, dx) for dy in range(-HALO, HALO + 1) for dx in range(-HALO, HALO + 1)]


def reproject(cur, rays, index, t, xyzr1, xyzr0, M, o_prev, h0, h1, h2, params=None, rparams=None):
    """Steps 1 to 4 with the fast history: (h0', h1', h2', info) before the clamp.  info as temporal_ref.step's."""
    p = dict(T_DEFAULTS, **(params or {}))
    rp = dict(R_DEFAULTS, **(rparams or {}))
    cur, rays, t, h0, h1, h2 = (np.asarray(a, F) for a in (cur, rays, t, h0, h1, h2))
    s = np.ascontiguousarray(index, np.int32)
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
        sf = np.zeros((H, W, 3), F)
        s1 = np.zeros((H, W), F)
        s2 = np.zeros((H, W), F)
        lmin = np.full((H, W), np.inf, F)
        taps = np.zeros((H, W, 4), bool)
        for j, i in [(j, i) for j in (0, 1) for i in (0, 1)]:
            xq, yq = x0 + F(i), y0 + F(j)
            inside = (xq >= 0) & (xq < Wf) & (yq >= 0) & (yq < Hf)
            bw = (wx if i else F(1) - wx) * (wy if j else F(1) - wy)
            xi = np.where(inside, xq, F(0)).astype(np.int64)
            yi = np.where(inside, yq, F(0)).astype(np.int64)
            q0, q1, q2, qs = h0[yi, xi], h1[yi, xi], h2[yi, xi], sbits[yi, xi]
            depth = np.abs(q1[..., 2] - te) <= tol
            cnt = (front & inside & (bw > 0) & (q0[..., 3] >= 1) & np.isfinite(q0[..., :3]).all(-1) & (qs == s) & (~hit | depth))
            taps[..., 2 * j + i] = cnt
            sw = sw + np.where(cnt, bw, F(0))
            sc = sc + np.where(cnt[..., None], bw[..., None] * q0[..., :3], F(0))
            sf = sf + np.where(cnt[..., None], bw[..., None] * q2[..., :3], F(0))
            s1 = s1 + np.where(cnt, bw * q1[..., 0], F(0))
            s2 = s2 + np.where(cnt, bw * q1[..., 1], F(0))
            lmin = np.where(cnt, np.fmin(lmin, q0[..., 3]), lmin)
        Lc = lum(cur)
        found = sw > 0
        cp, fp, m1p, m2p = sc / sw[..., None], sf / sw[..., None], s1 / sw, s2 / sw
        N = np.fmin(lmin + F(1), F(p["max_history"]))
        alpha = F(1) / N
        c_hist = cp + alpha[..., None] * (cur[..., :3] - cp)
        m1_hist = m1p + alpha * (Lc - m1p)
        m2_hist = m2p + alpha * (Lc * Lc - m2p)
        af = F(1) / np.fmin(N, F(rp["fast_history"]))
        f_hist = fp + af[..., None] * (cur[..., :3] - fp)
        fin = np.isfinite(cur[..., :3]).all(-1)
        found = found & fin
        o0 = np.empty((H, W, 4), F)
        o1 = np.empty((H, W, 4), F)
        o2 = np.empty((H, W, 4), F)
        o0[..., :3] = np.where(found[..., None], c_hist, cur[..., :3])
        o0[..., 3] = np.where(fin, np.where(found, N, F(1)), F(0))
        o1[..., 0] = np.where(fin, np.where(found, m1_hist, Lc), F(0))
        o1[..., 1] = np.where(fin, np.where(found, m2_hist, Lc * Lc), F(0))
        o1[..., 2] = t
        o1[..., 3] = index_bits(s)
        o2[..., :3] = np.where(found[..., None], f_hist, cur[..., :3])
        o2[..., 3] = np.where(fin, F(1), F(0))
    taps &= fin[..., None]
    return o0, o1, o2, {"taps": taps, "found": found, "finite": fin}


def clamp(h0, h1, h2, rparams=None, broken=None):
    """Steps 4b and 4c over step 4's output: (h0'', info).  info: "window" (H, W, 25) bool, the window taps that counted (dy then
    dx); "applied" the pixels with a history and two counted taps or more; "side" (H, W, 3) int8, -1 / 0 / +1 where a channel
    was raised to the box's lower edge / left alone / lowered to its upper edge; "moved" = the clamp changed the colour; "kept" =
    a pixel with history (len >= 2) that was not moved; "halo" = moved, and a counted tap of its window lies in another 32 x 8
    tile."""
    assert broken is None or broken in BROKEN
    rp = dict(R_DEFAULTS, **(rparams or {}))
    h0, h1, h2 = (np.asarray(a, F) for a in (h0, h1, h2))
    H, W = h0.shape[:2]
    c, N = h0[..., :3], h0[..., 3]
    sb = np.ascontiguousarray(h1[..., 3]).view(np.int32)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        ok = (h2[..., 3] == 1) & np.isfinite(h2[..., :3]).all(-1)
        s1 = np.zeros((H, W, 3), F)
        s2 = np.zeros((H, W, 3), F)
        n = np.zeros((H, W), F)
        window = np.zeros((H, W, 25), bool)
        other_tile = np.zeros((H, W), bool)
        order = [(dy, dx) for dx in range(-2, 3) for dy in range(-2, 3)] if broken == "window_order" else WINDOW
        for dy, dx in order:
            fq = _shift(h2[..., :3], dy, dx, F(0))
            cnt = _shift(ok, dy, dx, False) & (_shift(sb, dy, dx, 0) == sb)     # (outside the image: ok is False)
            same_tile = ((xx + dx) // TILE_W == xx // TILE_W) & ((yy + dy) // TILE_H == yy // TILE_H)
            if broken == "no_halo":
                cnt &= same_tile
            window[..., WINDOW.index((dy, dx))] = cnt
            other_tile |= cnt & ~same_tile
            s1 = s1 + np.where(cnt[..., None], fq, F(0))
            s2 = s2 + np.where(cnt[..., None], fq * fq, F(0))
            n = n + np.where(cnt, F(1), F(0))
        window &= (N >= 2)[..., None]            # (a pixel without history has no window)
        applied = (N >= 2) & (n >= 2)
        mean = s1 / n[..., None]
        var = s2 / n[..., None] - mean * mean
        if broken == "sample_variance":
            var = var * (n / (n - F(1)))[..., None]
        e = F(rp["clamp_sigma"]) * np.sqrt(np.fmax(F(0), var))
        lo, hi = mean - e, mean + e
        c2 = np.fmin(np.fmax(c, lo), hi)
        dd = np.abs(c2 - c)
        d = np.fmax(np.fmax(dd[..., 0], dd[..., 1]), dd[..., 2])
        emax = np.fmax(np.fmax(e[..., 0], e[..., 1]), e[..., 2])
        r = np.fmin(F(1), d / (emax + F(1e-6)))
        N2 = N + (F(rp["antilag"]) * r) * (np.fmin(N, F(rp["fast_history"])) - N)
        out = h0.copy()
        out[..., :3] = np.where(applied[..., None], c2, c)
        out[..., 3] = np.where(applied, N2, N)
        side = np.where(applied[..., None], (c > hi).astype(np.int8) - (c < lo).astype(np.int8), 0).astype(np.int8)
    moved = applied & (c2.view(np.uint32) != c.view(np.uint32)).any(-1)
    return out, {"window": window, "applied": applied, "side": side, "moved": moved, "kept": (N >= 2) & ~moved,
                 "halo": moved & other_tile, "r": np.where(applied, r, F(0))}


def step(cur, rays, index, t, xyzr1, xyzr0, M, o_prev, h0, h1, h2, params=None, rparams=None, broken=None):
    """One mrt_temporal_step with the response on: (h0'', h1', h2', info), bit for bit what the device computes.  info:
    reproject's and clamp's together."""
    o0, o1, o2, info = reproject(cur, rays, index, t, xyzr1, xyzr0, M, o_prev, h0, h1, h2, params, rparams)
    out, cinfo = clamp(o0, o1, o2, rparams, broken)
    return out, o1, o2, dict(info, **cinfo, unclamped=o0)


def step_f64(cur, rays, index, t, xyzr1, xyzr0, M, o_prev, h0, h1, h2, params=None, rparams=None):
    """The same definition per pixel in float64 (no float32 rounding): (h0'', h1' without the index bits, h2', taps, window,
    side)."""
    p = dict(T_DEFAULTS, **(params or {}))
    rp = dict(R_DEFAULTS, **(rparams or {}))
    s = np.asarray(index, np.int32)
    H, W = s.shape
    cur, rays, t = (np.asarray(a, np.float64) for a in (cur, rays, t))
    x1, x0_ = np.asarray(xyzr1, np.float64).reshape(-1, 4), np.asarray(xyzr0, np.float64).reshape(-1, 4)
    M, o_prev = np.asarray(M, np.float64), np.asarray(o_prev, np.float64)
    g0, g1, g2 = np.asarray(h0, np.float64), np.asarray(h1, np.float64), np.asarray(h2, np.float64)
    gbits = np.asarray(h1, F)[..., 3].view(np.int32)
    L = lambda c: (0.2126 * c[0] + 0.7152 * c[1]) + 0.0722 * c[2]
    o0 = np.zeros((H, W, 4))
    o1 = np.zeros((H, W, 3))
    o2 = np.zeros((H, W, 4))
    taps = np.zeros((H, W, 4), bool)
    for y in range(H):
        for x in range(W):
            c = cur[y, x, :3]
            o1[y, x, 2] = t[y, x]
            if not np.isfinite(c).all():
                o0[y, x, :3] = c
                o2[y, x, :3] = c
                continue
            o, d = rays[y, x, :3], rays[y, x, 3:]
            k = int(s[y, x])
            if k >= 0:
                Xp = x0_[k, :3] + (o + t[y, x] * d - x1[k, :3]) * (x0_[k, 3] / x1[k, 3])
            else:
                Xp = o_prev + d
            v = Xp - o_prev
            a, b, l = M @ v
            sw, sc, sf, s1, s2, lmin = 0.0, np.zeros(3), np.zeros(3), 0.0, 0.0, math.inf
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
                        sf += bw * g2[yq, xq, :3]
                        s1 += bw * q1[0]
                        s2 += bw * q1[1]
                        lmin = min(lmin, q0[3])
            Lc = L(c)
            o2[y, x, 3] = 1
            if sw > 0:
                N = min(lmin + 1, p["max_history"])
                cp, fp, m1p, m2p = sc / sw, sf / sw, s1 / sw, s2 / sw
                o0[y, x, :3] = cp + (c - cp) / N
                o0[y, x, 3] = N
                o1[y, x, 0] = m1p + (Lc - m1p) / N
                o1[y, x, 1] = m2p + (Lc * Lc - m2p) / N
                o2[y, x, :3] = fp + (c - fp) / min(N, rp["fast_history"])
            else:
                o0[y, x, :3] = c
                o0[y, x, 3] = 1
                o1[y, x, 0], o1[y, x, 1] = Lc, Lc * Lc
                o2[y, x, :3] = c
    out = o0.copy()
    window = np.zeros((H, W, 25), bool)
    side = np.zeros((H, W, 3), np.int8)
    for y in range(H):
        for x in range(W):
            if not o0[y, x, 3] >= 2:
                continue
            fs = []
            for w, (dy, dx) in enumerate(WINDOW):
                yq, xq = y + dy, x + dx
                if 0 <= yq < H and 0 <= xq < W and o2[yq, xq, 3] == 1 and np.isfinite(o2[yq, xq, :3]).all() and s[yq, xq] == s[y, x]:
                    window[y, x, w] = True
                    fs.append(o2[yq, xq, :3])
            if len(fs) < 2:
                continue
            fs = np.array(fs)
            mean = fs.mean(0)
            e = rp["clamp_sigma"] * np.sqrt(np.maximum(0.0, (fs * fs).mean(0) - mean * mean))
            c = o0[y, x, :3]
            c2 = np.minimum(np.maximum(c, mean - e), mean + e)
            side[y, x] = (c > mean + e).astype(np.int8) - (c < mean - e).astype(np.int8)
            r = min(1.0, np.abs(c2 - c).max() / (e.max() + 1e-6))
            N = o0[y, x, 3]
            out[y, x, :3] = c2
            out[y, x, 3] = N + rp["antilag"] * r * (min(N, rp["fast_history"]) - N)
    return out, o1, o2, taps, window, side


def synthetic_history(rng, index, t):
    """(h0, h1, h2) over the guides (index, t): a history that holds everything the taps and the window refuse -- holes (len 0,
    valid 0), lengths between the integers, other spheres' texels, distances beyond depth_tol, NaN and Inf in H0 and in H2 -- and,
    in one texel of seven, a colour four times too bright, which every clamp_sigma up to 3 moves."""
    h, w = index.shape
    h0 = rng.random((h, w, 4), dtype=F)
    h0[..., :3] *= np.where(rng.random((h, w)) < 0.15, F(4), F(1))[..., None]
    h0[..., 3] = rng.integers(0, 9, (h, w)).astype(F) + np.where(rng.random((h, w)) < 0.2, F(0.375), F(0))
    h1 = rng.random((h, w, 4), dtype=F)
    h1[..., 2] = t * (F(1) + F(0.08) * (rng.random((h, w), dtype=F) - F(0.5)))
    idx = np.array(index, np.int32)
    idx[rng.random((h, w)) < 0.1] += 1
    h1[..., 3] = index_bits(idx)
    h2 = rng.random((h, w, 4), dtype=F)
    h2[..., 3] = np.where(rng.random((h, w)) < 0.05, F(0), F(1))
    h0[0, 1, 0] = np.nan
    h0[h - 1, w - 1, 2] = np.inf
    h2[h // 2, w // 2, 1] = -np.inf
    h2[1, 0, 2] = np.nan
    h2[h - 1, 0, 0] = np.inf
    return h0, h1, h2
