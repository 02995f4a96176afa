"""Host reference of the denoiser's filter (include/myraytracer_amd.h, "denoiser"), restated in float32 numpy in the library's
operation order (denoise.hip is built with -ffp-contract=off, so every step is one correctly rounded float32 operation), and a
plain float64 per-pixel form of the same definition that the float32 one is checked against (tests/test_denoise_host.py)."""
import math

import numpy as np

F = np.float32
KERN = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F)
EPS = F(1e-6)
DEFAULTS = {"iterations": 5, "sigma_l": 8.0, "normal_exp": 7, "sigma_z": 0.05, "sigma_a": 0.1}


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def tukey(x):
    u = F(1) - x * x
    return np.where(x < F(1), u * u, F(0)).astype(F)


def _shift(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx] where that is inside the image, else fill."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if ys.stop > ys.start and xs.stop > xs.start:
        out[yd, xd] = a[ys, xs]
    return out


def denoise(rgba, S, K, guides, params=None):
    """float32 [rows, W, 4] frame, [rows, W] S, the noise factor K (+inf allowed) and the guides (index, t, normal, albedo as
    State.debug_read_guides returns them) -> the denoised [rows, W, 4], bit for bit what mrt_debug_denoise computes."""
    p = dict(DEFAULTS, **(params or {}))
    rgba = np.asarray(rgba, F)
    S = np.asarray(S, F)
    lum_stop = not math.isinf(K)
    sl, sz, sa = F(p["sigma_l"]), F(p["sigma_z"]), F(p["sigma_a"])
    inv_a = F(1) / sa
    n = np.asarray(guides["normal"], F)
    t = np.asarray(guides["t"], F)
    alb = np.asarray(guides["albedo"], F)
    miss = np.asarray(guides["index"]) < 0
    with np.errstate(all="ignore"):
        cv = np.empty(rgba.shape, F)
        cv[..., :3] = rgba[..., :3]
        cv[..., 3] = S * F(K) if lum_stop else np.where(np.isfinite(S), F(0), S)
        inv_z = np.where(miss, F(0), F(1) / (sz * t)).astype(F)
        for it in range(p["iterations"]):
            h = 1 << it
            fin = np.isfinite(cv).all(-1)
            active = fin & ~(lum_stop & (cv[..., 3] == 0))
            lp = lum(cv)
            inv_l = (F(1) / (sl * np.sqrt(cv[..., 3]) + EPS)).astype(F) if lum_stop else None
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
                        nq = _shift(n, dy, dx, F(0))
                        wn = np.fmax(F(0), (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
                        for _ in range(p["normal_exp"]):
                            wn = wn * wn
                        mq = _shift(miss, dy, dx, False)
                        tq = _shift(t, dy, dx, F(0))
                        wz = np.where(miss != mq, F(0), np.where(miss, F(1), tukey(np.abs(t - tq) * inv_z)))
                        aq = _shift(alb, dy, dx, F(0))
                        da = np.fmax(np.fmax(np.abs(alb[..., 0] - aq[..., 0]), np.abs(alb[..., 1] - aq[..., 1])),
                                     np.abs(alb[..., 2] - aq[..., 2]))
                        wa = tukey(da * inv_a)
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


def denoise_f64(rgba, S, K, guides, params=None):
    """The same definition per pixel in float64 (no float32 rounding): what denoise() approximates."""
    p = dict(DEFAULTS, **(params or {}))
    rows, width = S.shape
    lum_stop = not math.isinf(K)
    k = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    tk = lambda x: (1 - x * x) ** 2 if x < 1 else 0.0
    L = lambda c: (0.2126 * c[0] + 0.7152 * c[1]) + 0.0722 * c[2]
    n = np.asarray(guides["normal"], np.float64)
    t = np.asarray(guides["t"], np.float64)
    alb = np.asarray(guides["albedo"], np.float64)
    miss = np.asarray(guides["index"]) < 0
    cv = np.empty((rows, width, 4))
    cv[..., :3] = rgba[..., :3]
    with np.errstate(all="ignore"):
        cv[..., 3] = np.asarray(S, np.float64) * float(F(K)) if lum_stop else np.where(np.isfinite(S), 0.0, S)
    for it in range(p["iterations"]):
        h = 1 << it
        nxt = cv.copy()
        fin = np.isfinite(cv).all(-1)
        for y in range(rows):
            for x in range(width):
                c = cv[y, x]
                if not fin[y, x] or (lum_stop and c[3] == 0):
                    continue
                sw = sv = 0.0
                sc = np.zeros(3)
                for ty in range(5):
                    for tx in range(5):
                        yq, xq = y + (ty - 2) * h, x + (tx - 2) * h
                        if not (0 <= yq < rows and 0 <= xq < width) or not fin[yq, xq]:
                            continue
                        q = cv[yq, xq]
                        w = k[tx] * k[ty]
                        if (yq, xq) != (y, x):
                            wl = tk(abs(L(c) - L(q)) / (p["sigma_l"] * math.sqrt(c[3]) + 1e-6)) if lum_stop else 1.0
                            wn = max(0.0, float(n[y, x] @ n[yq, xq])) ** (2 ** p["normal_exp"])
                            if miss[y, x] != miss[yq, xq]:
                                wz = 0.0
                            elif miss[y, x]:
                                wz = 1.0
                            else:
                                wz = tk(abs(t[y, x] - t[yq, xq]) / (p["sigma_z"] * t[y, x]))
                            wa = tk(float(np.max(np.abs(alb[y, x] - alb[yq, xq]))) / p["sigma_a"])
                            w *= wl * wn * wz * wa
                        sw += w
                        sc += w * q[:3]
                        sv += w * w * q[3]
                nxt[y, x, :3] = sc / sw
                nxt[y, x, 3] = sv / (sw * sw)
        cv = nxt
    out = cv.copy()
    out[..., 3] = rgba[..., 3]
    return out


def random_case(rng, rows, width, n_spheres=5, nonfinite=True, zero_var=True):
    """A small synthetic frame, S and guides with a few spheres, misses, NaN / Inf texels and zero-variance texels."""
    rgba = rng.uniform(0.0, 1.0, (rows, width, 4)).astype(F)
    S = rng.uniform(0.0, 0.05, (rows, width)).astype(F)
    # patches of one sphere each (so that the edge stops see both sides), a band of sky on top
    idx = (np.arange(width)[None, :] * n_spheres // width + np.arange(rows)[:, None] // 4) % n_spheres
    idx = idx.astype(np.int32)
    idx[-2:, :] = -1
    base_n = rng.normal(size=(n_spheres, 3))
    base_n /= np.linalg.norm(base_n, axis=1, keepdims=True)
    normal = base_n[idx] + rng.normal(scale=0.05, size=(rows, width, 3))
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    t = (rng.uniform(1.0, 5.0, n_spheres)[idx] * rng.uniform(0.97, 1.03, (rows, width)))
    albedo = rng.uniform(0.1, 0.9, (n_spheres, 3))[idx]
    sky = idx < 0
    t[sky] = np.inf
    normal[sky] = (0.0, 0.0, 1.0)
    albedo[sky] = 1.0
    if nonfinite:
        rgba[1, 2, 0] = np.nan
        rgba[rows // 2, width - 1, 1] = np.inf
        S[0, width // 2] = np.nan
        S[rows - 1, 0] = np.inf
    if zero_var:
        S[rows // 2, width // 3] = 0.0
        S[2, 1] = 0.0
    guides = {"index": idx, "t": t.astype(F), "normal": normal.astype(F), "albedo": albedo.astype(F)}
    return rgba, S, guides


def fma32(a, b, c):
    """fmaf per element, correctly rounded: the exact product in float64, an exact sum (TwoSum), and the one case where rounding
    the float64 sum to float32 differs from rounding the exact value -- a float32 halfway point with a non-zero remainder."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(F)
    r64 = r.astype(np.float64)
    other = np.nextafter(r, np.where(s > r64, F(np.inf), F(-np.inf)).astype(F)).astype(np.float64)
    tie = (s != r64) & (s == (r64 + other) / 2) & (err != 0)
    toward_other = np.sign(other - r64) == np.sign(err)
    return np.where(tie & toward_other, other, r64).astype(F)


def centre_rays(width, height, cam_raw=None):
    """render_kernel's camera ray at u = v = 0.5 for every pixel (row 0 = bottom), the look-at camera through its lens centre,
    normalised as the render normalises: (rows, W, 6) = origin, direction."""
    ps = F(2) / F(height)
    x = np.arange(width, dtype=F)[None, :] * np.ones((height, 1), F)
    y = np.arange(height, dtype=F)[:, None] * np.ones((1, width), F)
    vx = ((x + F(0.5)) - F(0.5) * F(width)) * ps + F(0.5) * ps
    vy = ((y + F(0.5)) - F(0.5) * F(height)) * ps + F(0.5) * ps
    rays = np.zeros((height, width, 6), F)
    if cam_raw is None or cam_raw.mode == 0:
        d = [vx, vy, np.full_like(vx, F(-1))]
    else:
        d = [(vx * F(cam_raw.su[k]) + vy * F(cam_raw.sv[k])) - F(cam_raw.fw[k]) for k in range(3)]
        for k in range(3):
            rays[..., k] = F(cam_raw.origin[k])
    length = np.sqrt(fma32(d[2], d[2], fma32(d[1], d[1], d[0] * d[0])))
    for k in range(3):
        rays[..., 3 + k] = d[k] / length
    return rays


def expected_guides(O, spheres, rays):
    """orc_world_hit_batch's winners and t, orc_world_hit's normal and material per hit, the albedo from the packed materials."""
    import ctypes as C

    from common import to_oracle_spheres
    packed = O.pack_world(to_oracle_spheres(O, spheres))
    flat = rays.reshape(-1, 6)
    hit, t, _, _ = O.world_hit_batch(packed, flat)
    normal = np.zeros((len(flat), 3), np.float32)
    albedo = np.ones((len(flat), 3), np.float32)
    w = packed.world
    L = O.lib()
    for i in np.nonzero(hit >= 0)[0]:
        h, which = O.Hit(), C.c_int32()
        o = (C.c_float * 3)(*flat[i, :3]); d = (C.c_float * 3)(*flat[i, 3:])
        assert L.orc_world_hit(C.byref(w), packed.vec4.ctypes.data, packed.f32.ctypes.data, packed.i32.ctypes.data, o, d,
                               0.001, 1.0e4, C.byref(h), C.byref(which)) == 1 and which.value == hit[i]
        normal[i] = np.array(h.normal[:], np.float32)
        v4 = packed.vec4.reshape(-1, 4)
        if h.ty == 1:
            albedo[i] = v4[w.lambertians.albedo_base_idx + h.idx, :3]
        elif h.ty == 2:
            albedo[i] = v4[w.metals.albedo_base_idx + h.idx, :3]
        elif h.ty != 3:
            albedo[i] = 0.0
    miss = hit < 0
    normal[miss] = -flat[miss, 3:]
    t = np.where(miss, np.float32(np.inf), t).astype(np.float32)
    return hit, t, normal, albedo
