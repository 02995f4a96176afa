"""Ground truth for converged renders: the value of the rendering integral per pixel, in float64, and the statistics that
compare a rendered mean with it.  numpy only; imports neither the oracle nor the product, and is written from the definitions in
include/myraytracer_amd.h and the physical meaning of each material, not from oracle/rt_oracle.c.

What it returns, per pixel: the expected RGB, the expected luminance (the header's lum: 0.2126 r + 0.7152 g + 0.0722 b) and the
per-sample variance of the luminance (second moment minus squared first).

The shader's definitions, quirks included (they are the definition, not bugs; the truth follows them):
  * footprint: viewport_base = ((x + 0.5) - 0.5 W) * 2 / H, sample offset [0, 1) * pixel_side, so the footprint is shifted half a
    pixel up and right of the pixel's centre; row 0 is the bottom row; directions are normalised;
  * sample offsets are float32(u32) / 2^32 and can reach 1.0 (a set of measure 2^-25: not modelled);
  * the hit range is [0.001, 1e4), the lowest sphere index wins ties, the normal is (at - centre) / radius (a negative radius
    turns it round) and faces the ray: front_face = dot(normal, dir) <= 0;
  * Lambertian: normalize(n + unit-sphere point), i.e. cosine-distributed about n; Metal: reflect + fuzz * unit-ball point,
    absorbed when dot(dir, n) <= 0 (with <=); Dielectric: Schlick reflectance, total internal reflection reflects;
  * a path that has made `depth` calls of world_hit without leaving is black;
  * stream RNG mode: frame k starts pixel p from seed_p ^ shuffle_k (XOR shuffle): see xor_shuffle_allowance.

Quadrature.  closed_form() integrates over the footprint by a G x G midpoint grid.  The mean's error is O(1 / G^2) of the
curvature.  The VARIANCE needs more: a midpoint grid leaves out the variance inside each cell, about 1 / G^2 of a smooth pixel's
variance.  This module ADDS the within-cell term: the squared gradient of the conditional mean across the cell / 12 per axis.
"""
import math

import numpy as np

SPHERE_DTYPE = np.dtype([("center", "<f4", 3), ("radius", "<f4"), ("material_ty", "<i4"), ("albedo", "<f4", 3), ("param", "<f4")])
LAMBERTIAN, METAL, DIELECTRIC = 1, 2, 3
LUM = np.array([0.2126, 0.7152, 0.0722])
SKY_A = np.array([0.75, 0.85, 1.0])        # sky(y) = mix(white, (0.5, 0.7, 1), 0.5 y + 0.5) = A + B y per channel
SKY_B = np.array([-0.25, -0.15, 0.0])
T_MIN, T_SUP = 0.001, 1.0e4
EPS32 = 2.0 ** -24


def lum(c):
    c = np.asarray(c, np.float64)
    return c[..., 0] * LUM[0] + c[..., 1] * LUM[1] + c[..., 2] * LUM[2]


def spheres(*rows):
    """rows: (centre, radius, type, albedo, param)."""
    out = np.zeros(len(rows), SPHERE_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def scene_default():
    """The shipped scene (the header's mrt_scene_default): ground, a Lambertian ball, two fuzzy metal balls."""
    return spheres(((0, -100.5, -1), 100, LAMBERTIAN, (0.8, 0.8, 0.0), 0.0), ((0, 0, -1), 0.5, LAMBERTIAN, (0.7, 0.3, 0.3), 0.0),
                   ((-1, 0, -1), 0.5, METAL, (0.8, 0.8, 0.8), 0.3), ((1, 0, -1), 0.5, METAL, (0.8, 0.6, 0.2), 1.0))


PINHOLE = None


def lookat(lookfrom, at, vup=(0, 1, 0), vfov=90.0, defocus=0.0, focus=1.0):
    return {"lookfrom": tuple(map(float, lookfrom)), "lookat": tuple(map(float, at)), "vup": tuple(map(float, vup)),
            "vfov": float(vfov), "defocus": float(defocus), "focus": float(focus)}


# The fixed scenes.  Closed-form scenes hold ONE sphere; the others go through the Monte-Carlo integrator.
_BALL = ((0.1, 0.05, -1.2), 0.5)
_LOOK = lookat((1.5, 0.8, 0.6), (0.1, 0.0, -1.2), vfov=50.0)
SCENES = {
    "sky": dict(spheres=spheres(), cam=PINHOLE, depth=8),
    "lambert": dict(spheres=spheres((*_BALL, LAMBERTIAN, (0.7, 0.4, 0.3), 0.0)), cam=PINHOLE, depth=8),
    "lambert-depth1": dict(spheres=spheres((*_BALL, LAMBERTIAN, (0.7, 0.4, 0.3), 0.0)), cam=PINHOLE, depth=1),
    "lambert-lookat": dict(spheres=spheres((*_BALL, LAMBERTIAN, (0.7, 0.4, 0.3), 0.0)), cam=_LOOK, depth=8),
    "metal": dict(spheres=spheres((*_BALL, METAL, (0.8, 0.6, 0.3), 0.0)), cam=PINHOLE, depth=8),
    "glass": dict(spheres=spheres((*_BALL, DIELECTRIC, (1, 1, 1), 1.5)), cam=PINHOLE, depth=8),
    "glass-low": dict(spheres=spheres(((0.1, 0.05, -1.2), 0.6, DIELECTRIC, (1, 1, 1), 0.85)), cam=PINHOLE, depth=8),
    # no closed form: tests/golden/radiometry_<name>.npz
    "fuzzy": dict(spheres=spheres((*_BALL, METAL, (0.8, 0.6, 0.3), 0.4)), cam=PINHOLE, depth=8),
    "default": dict(spheres=scene_default(), cam=PINHOLE, depth=8),
    "hollow": dict(spheres=spheres(((0, -100.5, -1), 100, LAMBERTIAN, (0.5, 0.6, 0.4), 0.0), (*_BALL, DIELECTRIC, (1, 1, 1), 1.5),
                                   (_BALL[0], -0.4, DIELECTRIC, (1, 1, 1), 1.5)), cam=PINHOLE, depth=12),
    "lens": dict(spheres=scene_default(), cam=lookat((1.6, 0.7, 0.8), (0, 0, -1), vfov=45.0, defocus=4.0, focus=2.5), depth=8),
}
CLOSED_FORM = ("sky", "lambert", "lambert-depth1", "lambert-lookat", "metal", "glass", "glass-low")
FIXTURES = ("glass", "fuzzy", "default", "hollow", "lens")        # whole images; the other closed-form scenes: edge pixels only
WIDTH, HEIGHT = 48, 32


# ------------------------------------------------------------------ footprints

def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def camera_basis(cam):
    lf, la, up = (np.array(cam[k], np.float64) for k in ("lookfrom", "lookat", "vup"))
    w = _unit(lf - la)
    u = _unit(np.cross(up, w))
    v = np.cross(w, u)
    half = math.tan(math.radians(cam["vfov"]) / 2) * cam["focus"]          # the viewport's half height on the focus plane
    lens = math.tan(math.radians(cam["defocus"]) / 2) * cam["focus"] if cam["defocus"] > 0 else 0.0
    return lf, u, v, w, half, lens


def camera_rays(cam, width, height, px, py, su, sv, lens_xy=None):
    """Rays of pixels (px, py) at sample offsets (su, sv) in [0, 1) (arrays broadcast together); lens_xy: points of the unit disc.
    -> (origin, unit direction), float64."""
    side = 2.0 / height
    vx = ((px + 0.5) - 0.5 * width) * side + su * side
    vy = ((py + 0.5) - 0.5 * height) * side + sv * side
    vx, vy = np.broadcast_arrays(np.asarray(vx, np.float64), np.asarray(vy, np.float64))
    if cam is None:
        d = np.stack([vx, vy, -np.ones_like(vx)], -1)
        return np.zeros_like(d), _unit(d)
    lf, u, v, w, half, lens = camera_basis(cam)
    p = vx[..., None] * (half * u) + vy[..., None] * (half * v) - cam["focus"] * w       # the point on the focus plane
    if lens > 0.0:
        off = lens * (lens_xy[..., 0:1] * u + lens_xy[..., 1:2] * v)
        return lf + off, _unit(p - off)
    return np.broadcast_to(lf, p.shape).copy(), _unit(p)


# ------------------------------------------------------------------ one sphere

def hit_sphere(o, d, centre, radius):
    """t of the sphere's hit in [T_MIN, T_SUP), +inf on a miss: near root first, else the far root."""
    oc = o - centre
    a = (d * d).sum(-1)
    b = (oc * d).sum(-1)
    c = (oc * oc).sum(-1) - radius * radius
    disc = b * b - a * c
    ok = disc >= 0
    sq = np.sqrt(np.where(ok, disc, 0.0))
    t = (-b - sq) / a
    far = (t < T_MIN) | (t >= T_SUP)
    t = np.where(far, (-b + sq) / a, t)
    ok &= ~((t < T_MIN) | (t >= T_SUP))
    return np.where(ok, t, np.inf)


def _surface(o, d, t, centre, radius):
    at = o + t[..., None] * d
    n = (at - centre) / radius
    front = (n * d).sum(-1) <= 0
    n = np.where(front[..., None], n, -n)
    return at, n, front


def dielectric_split(d, n, front, ior):
    """-> (reflectance used: 1 under total internal reflection, reflected dir, refracted dir, total-reflection mask)."""
    ri = np.where(front, 1.0 / ior, ior)
    cos_t = np.minimum(-(d * n).sum(-1), 1.0)
    sin_t = np.sqrt(np.maximum(1.0 - cos_t * cos_t, 0.0))
    tir = ri * sin_t > 1.0
    r0 = ((1.0 - ri) / (1.0 + ri)) ** 2
    refl_p = np.where(tir, 1.0, r0 + (1.0 - r0) * (1.0 - cos_t) ** 5)
    refl = d - 2.0 * (d * n).sum(-1, keepdims=True) * n
    perp = ri[..., None] * (d + cos_t[..., None] * n)
    para = -np.sqrt(np.abs(1.0 - (perp * perp).sum(-1)))[..., None] * n
    return refl_p, refl, _unit(perp + para), tir


class _Moments:
    """Per ray: E[rgb], E[L], E[L^2] and a path-class code, accumulated over the leaves of the scatter tree."""

    def __init__(self, n):
        self.rgb = np.zeros((n, 3))
        self.l1 = np.zeros(n)
        self.l2 = np.zeros(n)
        self.prob = np.zeros(n)                 # probability that has reached a leaf (out-of-depth leaves included)
        self.cls = np.zeros(n, np.int64)
        self.node = 0

    def mark(self, idx, code):
        """Path class: one base-3 digit per tree node visited (0 miss, 1 hit, 2 hit under total reflection)."""
        assert self.node < 39
        self.cls[idx] += np.asarray(code, np.int64) * 3 ** self.node
        self.node += 1

    def leaf(self, idx, p, att, ey, ey2):
        """A leaf that leaves the scene with E[y] = ey, E[y^2] = ey2 of its direction: value att * sky(y)."""
        P, Q = float(LUM @ (att * SKY_A)), float(LUM @ (att * SKY_B))
        self.rgb[idx] += p[:, None] * (att * SKY_A + (att * SKY_B) * ey[:, None])
        self.l1[idx] += p * (P + Q * ey)
        self.l2[idx] += p * (P * P + 2 * P * Q * ey + Q * Q * ey2)
        self.prob[idx] += p

    def dark(self, idx, p):
        self.prob[idx] += p


def _glass_tree(m, idx, p, o, d, centre, radius, ior, depth):
    """The tree of reflect / refract choices down to `depth` calls of world_hit; branches nobody takes are pruned."""
    if idx.size == 0:
        return
    if depth == 0:
        m.dark(idx, p)
        return
    t = hit_sphere(o, d, centre, radius)
    hit = np.isfinite(t)
    at, n, front = _surface(o[hit], d[hit], t[hit], centre, radius)
    refl_p, refl, refr, tir = dielectric_split(d[hit], n, front, ior)
    code = np.zeros(idx.size, np.int64)
    code[hit] = 1 + tir
    m.mark(idx, code)
    m.leaf(idx[~hit], p[~hit], np.ones(3), d[~hit, 1], d[~hit, 1] ** 2)
    keep = refl_p > 0
    _glass_tree(m, idx[hit][keep], (p[hit] * refl_p)[keep], at[keep], refl[keep], centre, radius, ior, depth - 1)
    keep = ~tir
    _glass_tree(m, idx[hit][keep], (p[hit] * (1.0 - refl_p))[keep], at[keep], refr[keep], centre, radius, ior, depth - 1)


def ray_moments(scene, o, d):
    """Closed-form transport of rays (n, 3) through a scene of at most one sphere -> _Moments."""
    sp, depth = scene["spheres"], scene["depth"]
    n = len(o)
    m = _Moments(n)
    idx, one = np.arange(n), np.ones(n)
    if depth == 0:
        m.dark(idx, one)
        return m
    if len(sp) == 0:
        m.leaf(idx, one, np.ones(3), d[:, 1], d[:, 1] ** 2)
        return m
    assert len(sp) == 1 and sp[0]["radius"] > 0, "closed forms hold for one convex sphere"
    centre, radius = sp[0]["center"].astype(np.float64), float(sp[0]["radius"])
    ty, albedo, param = int(sp[0]["material_ty"]), sp[0]["albedo"].astype(np.float64), float(sp[0]["param"])
    if ty == DIELECTRIC:
        _glass_tree(m, idx, one, o, d, centre, radius, param, depth)
        return m
    t = hit_sphere(o, d, centre, radius)
    hit = np.isfinite(t)
    m.mark(idx, hit)
    m.leaf(idx[~hit], one[~hit], np.ones(3), d[~hit, 1], d[~hit, 1] ** 2)
    h = idx[hit]
    if depth == 1:                                  # the scattered ray would need a second world_hit: black
        m.dark(h, one[hit])
        return m
    _, nrm, _ = _surface(o[hit], d[hit], t[hit], centre, radius)
    if ty == LAMBERTIAN:                            # cosine-distributed about n, and a convex sphere is not hit again
        m.leaf(h, one[hit], albedo, (2.0 / 3.0) * nrm[:, 1], 0.25 + 0.25 * nrm[:, 1] ** 2)
    elif ty == METAL:
        assert param == 0.0, "closed form for fuzz 0 only"
        r = d[hit] - 2.0 * (d[hit] * nrm).sum(-1, keepdims=True) * nrm
        m.leaf(h, one[hit], albedo, r[:, 1], r[:, 1] ** 2)
    else:
        m.dark(h, one[hit])                          # an unknown material absorbs
    return m


def closed_form(name_or_scene, width=WIDTH, height=HEIGHT, G=16, rows=None):
    """The truth of a closed-form scene by a G x G midpoint grid -> dict(rgb (H, W, 3), mu (H, W), var (H, W), cls (H, W, G*G),
    prob).  var includes the within-cell term (module docstring).  rows = (y0, y1) restricts the rows computed."""
    scene = SCENES[name_or_scene] if isinstance(name_or_scene, str) else name_or_scene
    cam = scene["cam"]
    assert cam is None or cam["defocus"] == 0.0, "closed forms are pinhole / look-at; the thin lens goes through monte_carlo"
    y0, y1 = rows or (0, height)
    g = (np.arange(G) + 0.5) / G
    py, px, sv, su = np.meshgrid(np.arange(y0, y1), np.arange(width), g, g, indexing="ij")
    o, d = camera_rays(cam, width, height, px, py, su, sv)
    m = ray_moments(scene, o.reshape(-1, 3), d.reshape(-1, 3))
    shape = (y1 - y0, width, G, G)
    l1 = m.l1.reshape(shape)
    gy, gx = np.gradient(l1, axis=2), np.gradient(l1, axis=3)             # per cell step
    within = ((gx * gx + gy * gy) / 12.0).mean((2, 3))
    mu = l1.mean((2, 3))
    var = m.l2.reshape(shape).mean((2, 3)) + within - mu * mu
    return dict(rgb=m.rgb.reshape(shape + (3,)).mean((2, 3)), mu=mu, var=np.maximum(var, 0.0),
                cls=m.cls.reshape(shape[0], width, G * G), prob=m.prob.reshape(shape))


def smooth_mask(cls):
    """A pixel is smooth only if every grid point of the pixel AND of its eight neighbours takes the same path class (a pixel the
    sphere covers by less than a grid cell is caught by its neighbour's grid; at the image border the pixels that exist count)."""
    lo, hi = cls.min(-1), cls.max(-1)
    h, w = lo.shape
    plo = np.pad(lo, 1, mode="edge")
    phi = np.pad(hi, 1, mode="edge")
    ok = lo == hi
    for dy in range(3):
        for dx in range(3):
            ok &= (plo[dy:dy + h, dx:dx + w] == lo) & (phi[dy:dy + h, dx:dx + w] == lo)
    return ok


# ------------------------------------------------------------------ the Monte-Carlo integrator

def world_hit(sp, o, d):
    """Brute force over [T_MIN, T_SUP): the lowest index wins ties -> (t, index or -1)."""
    best = np.full(len(o), np.inf)
    which = np.full(len(o), -1)
    for i in range(len(sp)):
        t = hit_sphere(o, d, sp[i]["center"].astype(np.float64), float(sp[i]["radius"]))
        better = t < best
        best[better] = t[better]
        which[better] = i
    return best, which


def _unit_sphere(rng, n):
    return _unit(rng.standard_normal((n, 3)))


def trace(scene, o, d, rng):
    """Radiance of n paths, float64 (n, 3)."""
    sp = scene["spheres"]
    n = len(o)
    out = np.zeros((n, 3))
    att = np.ones((n, 3))
    alive = np.arange(n)
    for _ in range(scene["depth"]):
        if alive.size == 0:
            break
        t, which = world_hit(sp, o, d)
        miss = which < 0
        out[alive[miss]] = att[alive[miss]] * (SKY_A + SKY_B * d[miss, 1:2])
        alive, o, d, t, which = alive[~miss], o[~miss], d[~miss], t[~miss], which[~miss]
        new_d = np.zeros_like(d)
        new_o = np.zeros_like(o)
        keep = np.zeros(alive.size, bool)
        for i in np.unique(which):
            s = which == i
            k = int(s.sum())
            centre, radius = sp[i]["center"].astype(np.float64), float(sp[i]["radius"])
            ty, albedo, param = int(sp[i]["material_ty"]), sp[i]["albedo"].astype(np.float64), float(sp[i]["param"])
            at, nrm, front = _surface(o[s], d[s], t[s], centre, radius)
            new_o[s] = at
            if ty == LAMBERTIAN:
                nd = nrm + _unit_sphere(rng, k)
                zero = (nd * nd).sum(-1) == 0
                nd[zero] = nrm[zero]
                new_d[s], keep[s] = _unit(nd), True
                att[alive[s]] *= albedo
            elif ty == METAL:
                ball = _unit_sphere(rng, k) * rng.random((k, 1)) ** (1.0 / 3.0)
                nd = d[s] - 2.0 * (d[s] * nrm).sum(-1, keepdims=True) * nrm + param * ball
                ok = (nd * nrm).sum(-1) > 0                                # absorbed when dot(dir, n) <= 0
                nd[~ok] = nrm[~ok]
                new_d[s], keep[s] = _unit(nd), ok
                att[alive[s]] *= albedo
            elif ty == DIELECTRIC:
                refl_p, refl, refr, _ = dielectric_split(d[s], nrm, front, param)
                new_d[s], keep[s] = np.where((refl_p > rng.random(k))[:, None], refl, refr), True
        alive, o, d = alive[keep], new_o[keep], new_d[keep]                # absorbed paths stay black
    return out


def monte_carlo(name_or_scene, n_ref, seed, width=WIDTH, height=HEIGHT, pixels=None, batch=128):
    """n_ref paths per pixel by numpy's PCG64 -> dict(rgb, mu, var (unbiased), n) over the whole image, or over `pixels` (a
    boolean (H, W) mask; the other pixels hold NaN).  The sample count comes back so that the reference's own error enters
    every comparison."""
    scene = SCENES[name_or_scene] if isinstance(name_or_scene, str) else name_or_scene
    cam = scene["cam"]
    mask = np.ones((height, width), bool) if pixels is None else pixels
    ys, xs = np.nonzero(mask)
    rng = np.random.Generator(np.random.PCG64(seed))
    s_rgb = np.zeros((len(ys), 3))
    s1 = np.zeros(len(ys))
    s2 = np.zeros(len(ys))
    done = 0
    defocus = cam is not None and cam["defocus"] > 0
    while done < n_ref and len(ys):
        b = min(batch, n_ref - done)
        shape = (len(ys), b)
        lens = None
        if defocus:
            r, th = np.sqrt(rng.random(shape)), rng.random(shape) * (2 * math.pi)
            lens = np.stack([r * np.cos(th), r * np.sin(th)], -1)
        o, d = camera_rays(cam, width, height, xs[:, None], ys[:, None], rng.random(shape), rng.random(shape), lens)
        c = trace(scene, o.reshape(-1, 3), d.reshape(-1, 3), rng).reshape(shape + (3,))
        L = lum(c)
        s_rgb += c.sum(1)
        s1 += L.sum(1)
        s2 += (L * L).sum(1)
        done += b
    out = dict(rgb=np.full((height, width, 3), np.nan), mu=np.full((height, width), np.nan), var=np.full((height, width), np.nan),
               n=n_ref)
    out["rgb"][ys, xs] = s_rgb / n_ref
    out["mu"][ys, xs] = s1 / n_ref
    out["var"][ys, xs] = np.maximum(s2 - s1 * s1 / n_ref, 0.0) / (n_ref - 1)
    return out


def truth(name, fixture=None, G=16):
    """The truth the tests compare with: the closed form on the smooth pixels, the Monte-Carlo result `fixture` (a dict as
    monte_carlo returns, e.g. a committed tests/golden/radiometry_<name>.npz) on the others, which have no bounded quadrature
    error -> dict(mu, var, rgb, ref_var = the variance of the truth's own mean, smooth, on = pixels whose first grid path hits).
    Scenes without a closed form are the fixture everywhere (smooth = all False).  Without a fixture the pixels that are not
    smooth hold NaN."""
    if name not in CLOSED_FORM:
        f = fixture
        return dict(mu=np.asarray(f["mu"]), var=np.asarray(f["var"]), rgb=np.asarray(f["rgb"]),
                    ref_var=np.asarray(f["var"]) / float(f["n"]), smooth=np.zeros(f["mu"].shape, bool),
                    on=np.zeros(f["mu"].shape, bool))
    cf = closed_form(name, G=G)
    smooth = smooth_mask(cf["cls"])
    out = dict(mu=cf["mu"].copy(), var=cf["var"].copy(), rgb=cf["rgb"].copy(), ref_var=np.zeros_like(cf["mu"]), smooth=smooth,
               on=(cf["cls"][..., 0] % 3) != 0)
    edge = ~smooth
    if fixture is not None:
        for k in ("mu", "var", "rgb"):
            out[k][edge] = np.asarray(fixture[k])[edge]
        out["ref_var"][edge] = np.asarray(fixture["var"])[edge] / float(fixture["n"])
    else:
        out["mu"][edge] = np.nan
    return out


# ------------------------------------------------------------------ statistics

def z_max(m, level=1e-6):
    """The two-sided Gaussian quantile at a family-wise level over m tests: P(|z| > z_max) = level / m (about 6.3 for 1,500)."""
    p = level / m
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if math.erfc(mid / math.sqrt(2.0)) > p:
            lo = mid
        else:
            hi = mid
    return hi


def rounding_var(mu, frames, spp):
    """Variance that float32 itself adds to an accumulated mean mu (from the number format, nothing measured): every rounding
    is uniform within half a unit in the last place of its result.  A frame sums spp samples one by one (sample i is added to a
    sum of about i mu: ulp(mu)^2 spp^3 / 36 in the sum) and divides; the running mean takes three roundings per blend (two
    products, one sum), and frame k's error is carried on with weight k / frames.  Holds while the addends' spread is many units in
    the last place of the running sum; beyond that the roundings of a sequential sum stop being random (it drifts), which
    bounds the samples per frame a stream-mode test may use (tests/test_gpu_radiometry.py, test_one_frame_of_many_samples)."""
    ulp = np.spacing(np.abs(mu).astype(np.float32)).astype(np.float64)
    in_frame = ulp * ulp * (spp / 36.0 + 1.0 / 12.0) / frames
    blend = ulp * ulp * (3.0 / 12.0) * (frames / 3.0 if frames > 1 else 0.0)
    return in_frame + blend


def statistics(got_rgb, tr, c2_over_spp, pixels=None, extra_var=0.0):
    """got_rgb (H, W, >=3) rendered mean; tr = truth(); c2_over_spp = sum of squared normalised frame weights / spp, a number or
    per pixel; pixels = boolean selection (default: every pixel with a truth).  Pixels whose true variance is 0 are compared
    for equality (`exact_bad` counts the failures) and take no part in z.
    -> dict(M, z (H, W) with NaN outside, max_z, z_bound, mean_z2, z2_bound, Z, r_h, r_v, r_bound, exact_bad, n_exact)."""
    got = lum(np.asarray(got_rgb, np.float64)[..., :3])
    sel = np.isfinite(tr["mu"]) if pixels is None else (pixels & np.isfinite(tr["mu"]))
    zero = sel & (tr["var"] == 0.0)
    exact_bad = int((np.abs(got[zero] - tr["mu"][zero]) > 4 * EPS32 * np.abs(tr["mu"][zero])).sum())
    sel = sel & ~zero
    se2 = tr["var"] * c2_over_spp + tr["ref_var"] + extra_var
    z = np.full(got.shape, np.nan)
    z[sel] = (got[sel] - tr["mu"][sel]) / np.sqrt(se2[sel])
    M = int(sel.sum())
    zs = z[sel]

    def lag(a, b):
        ok = np.isfinite(a) & np.isfinite(b)
        return float((a[ok] * b[ok]).mean()) if ok.any() else 0.0

    return dict(M=M, z=z, max_z=float(np.abs(zs).max()), z_bound=z_max(M), mean_z2=float((zs * zs).mean()),
                z2_bound=6.0 * math.sqrt(2.0 / M), Z=float((got[sel] - tr["mu"][sel]).sum() / math.sqrt(se2[sel].sum())),
                r_h=lag(z[:, :-1], z[:, 1:]), r_v=lag(z[:-1], z[1:]), r_bound=6.0 / math.sqrt(M), exact_bad=exact_bad,
                n_exact=int(zero.sum()))


def summary(s):
    return (f"M={s['M']} max|z|={s['max_z']:.2f}(<={s['z_bound']:.2f}) mean(z^2)={s['mean_z2']:.3f}(1+-{s['z2_bound']:.3f}) "
            f"Z={s['Z']:+.2f} r_h={s['r_h']:+.4f} r_v={s['r_v']:+.4f}(<={s['r_bound']:.4f}) exact_bad={s['exact_bad']}/{s['n_exact']}")


def check(s, variance=True, allowance=0.0, label=""):
    """The assertions of one comparison.  variance=False leaves the variance-type statistics (mean(z^2), neighbour correlation)
    measured and printed only: stream RNG mode below 64 samples per frame.  allowance widens those two for the XOR shuffle
    (xor_shuffle_allowance); the mean-type bounds never move."""
    text = f"{label}: {summary(s)}" + (f" allowance={allowance:.3f}" if allowance else "") + ("" if variance else " [variance: measured only]")
    print(text)
    assert s["exact_bad"] == 0, text
    assert s["max_z"] <= s["z_bound"], text
    assert abs(s["Z"]) <= 5.0, text
    if variance:
        assert abs(s["mean_z2"] - 1.0) <= s["z2_bound"] + allowance, text
        grow = math.sqrt(1.0 + (allowance / (6.0 * math.sqrt(2.0))) ** 2)
        assert abs(s["r_h"]) <= s["r_bound"] * grow and abs(s["r_v"]) <= s["r_bound"] * grow, text
    return text


def frame_pair_correlations(zs, max_lag=3):
    """zs: (F, H, W) z of single frames (NaN outside the selection) -> ({lag: r_k over the F - lag pairs}, M)."""
    zs = np.asarray(zs)
    flat = zs.reshape(len(zs), -1)
    flat = flat[:, np.isfinite(flat).all(0)]
    return {lag: (flat[:-lag] * flat[lag:]).mean(1) for lag in range(1, max_lag + 1)}, flat.shape[1]


def frame_independence(zs, counter, label=""):
    """Counter mode claims independent samples: |mean_k r_k| <= 6 / sqrt(M pairs).  Stream mode: zero on average only,
    self-normalised: |mean_k r_k| <= 6 sd_k(r_k) / sqrt(pairs).  -> {lag: (mean, sd, spread = sd x sqrt(M))}, lines printed."""
    r, M = frame_pair_correlations(zs)
    out, lines = {}, []
    for lag, rk in r.items():
        mean, sd = float(rk.mean()), float(rk.std(ddof=1))
        out[lag] = (mean, sd, sd * math.sqrt(M))
        bound = 6.0 / math.sqrt(M * len(rk)) if counter else 6.0 * sd / math.sqrt(len(rk))
        text = (f"{label} lag {lag}: mean r_k={mean:+.5f} (<={bound:.5f}) spread={sd * math.sqrt(M):.2f} x independent, "
                f"max|r_k|={float(np.abs(rk).max()):.3f}, M={M}, pairs={len(rk)}")
        print(text)
        lines.append(text)
        assert abs(mean) <= bound, text
    return out, lines


def calibration(S, K, tr, c2_over_spp, frames_eff, pixels):
    """R = sum S K / sum (var c2 / spp) over `pixels`, and sd(R) = sqrt(2 / (F - 1)) sqrt(sum v^2) / sum v."""
    v = (tr["var"] * c2_over_spp)[pixels]
    R = float((np.asarray(S, np.float64)[pixels] * K).sum() / v.sum())
    return R, math.sqrt(2.0 / (frames_eff - 1.0)) * math.sqrt(float((v * v).sum())) / float(v.sum())


# ------------------------------------------------------------------ the stream mode's XOR shuffle

def xoshiro128plus(s):
    """One step on a (4, n) uint32 state, in place -> the outputs (n,) uint32 (pinned by the published vector for (1, 2, 3, 4))."""
    out = s[0] + s[3]
    t = s[1] << np.uint32(9)
    s[2] ^= s[0]
    s[3] ^= s[1]
    s[1] ^= s[2]
    s[0] ^= s[3]
    s[2] ^= t
    s[3] = (s[3] << np.uint32(11)) | (s[3] >> np.uint32(21))
    return out


def xor_shuffle_spread(draws, n_c=128, n_a=4096, seed=7):
    """sd over random constants c of the correlation (over random states a) between the k-th outputs from a and a ^ c,
    k = 0 .. draws - 1 -> (draws,) float64.  The generator is GF(2)-linear, so the two streams differ by T^k c at every step and
    the outputs' top bits agree or disagree for a whole image at once."""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.integers(0, 2 ** 32, (4, 1, n_a), dtype=np.uint32)
    c = rng.integers(0, 2 ** 32, (4, n_c, 1), dtype=np.uint32)
    s0 = np.broadcast_to(a, (4, n_c, n_a)).reshape(4, -1).copy()
    s1 = (a ^ c).reshape(4, -1).copy()
    out = np.empty(draws)
    for k in range(draws):
        u0 = xoshiro128plus(s0).reshape(n_c, n_a) * 2.0 ** -32
        u1 = xoshiro128plus(s1).reshape(n_c, n_a) * 2.0 ** -32
        u0 = u0 - u0.mean(1, keepdims=True)
        u1 = u1 - u1.mean(1, keepdims=True)
        rho = (u0 * u1).mean(1) / np.sqrt((u0 * u0).mean(1) * (u1 * u1).mean(1))
        out[k] = math.sqrt(max(float((rho * rho).mean()) - 1.0 / n_a, 0.0))
    return out


_ALLOWANCE = {}


def xor_shuffle_allowance(spp, frames):
    """What the XOR shuffle may add to |mean(z^2) - 1| of a stream-mode accumulation of `frames` > 1 frames of spp samples.
    Two frames' states differ by one constant c at every pixel, so their samples' correlation rho has one sign over the image;
    over c it has mean 0 and, for one draw, the sd xor_shuffle_spread models.  A frame's mean averages spp samples whose
    correlations are independent in sign: sd(rho_frame) = s / sqrt(spp), s = the root mean square of the per-draw sd over the
    first 2 spp draws (a sample takes at least its two footprint draws).  The variance of the mean of F frames is
    sigma^2 / F x (1 + 2 / F x sum over pairs of rho), and the sum over F (F - 1) / 2 pairs has sd s sqrt(F (F - 1) / 2 / spp):
    a relative deviation of sd sqrt(2 (F - 1) / F) s / sqrt(spp), of which six are allowed, as everywhere in this module."""
    if frames <= 1:
        return 0.0
    if spp not in _ALLOWANCE:
        sd = xor_shuffle_spread(min(2 * spp, 128))
        _ALLOWANCE[spp] = math.sqrt(float((sd * sd).mean()))
    return 6.0 * math.sqrt(2.0 * (frames - 1) / frames) * _ALLOWANCE[spp] / math.sqrt(spp)
