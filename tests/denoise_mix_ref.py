"""Host reference of the denoiser's blend with the accumulation (include/myraytracer_amd.h, "Blend with the accumulation"),
restated in float32 numpy in the library's operation order on top of tests/denoise_ref.py, tests/denoise_var_ref.py and
tests/denoise_tiles_ref.py, and a plain float64 per-pixel form of the same definition that the float32 one is checked against
(tests/test_denoise_mix_host.py).

Those references return the filtered image with alpha in the place of the last iteration's variance u, which the blend needs.  So
the iterations are restated once here (filtered: every source, the luminance stop as a per-pixel array) and the host test holds
the restatement's colour to each of the three references bit for bit."""
import math

import numpy as np

from denoise_ref import DEFAULTS, EPS, F, KERN, _shift, lum, tukey
from denoise_tiles_ref import initial_variance, library_k, pixel_state
from denoise_var_ref import _stops, prefiltered_var, spatial_variance

R = 2           # the window: (2 R + 1)^2 pixels


def _iterate(cv, guides, p, stop, prefilter):
    """The a-trous iterations on (r, g, b, var); stop: the centre's luminance stop per pixel.  Returns (f, u) as one array."""
    sl = F(p["sigma_l"])
    stops = _stops(guides, p)
    shape = cv.shape[:2]
    with np.errstate(all="ignore"):
        for it in range(p["iterations"]):
            h = 1 << it
            fin = np.isfinite(cv).all(-1)
            g = np.where(stop, prefiltered_var(cv, fin), cv[..., 3]).astype(F) if prefilter else cv[..., 3]
            active = fin & ~(stop & (g == 0))
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
                        wl = np.where(stop, tukey(np.abs(lp - lum(cq)) * inv_l), F(1)).astype(F)
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
    return cv


def filtered(rgba, S, K, guides, params=None, variance=0):
    """(f, u) of a uniform accumulation: the last iteration's output of denoise_var_ref.denoise_var, before alpha."""
    p = dict(DEFAULTS, **(params or {}))
    rgba = np.asarray(rgba, F)
    S = np.asarray(S, F)
    spatial = variance == 2
    lum_stop = spatial or not math.isinf(K)
    with np.errstate(all="ignore"):
        cv = np.empty(rgba.shape, F)
        cv[..., :3] = rgba[..., :3]
        if spatial:
            cv[..., 3] = spatial_variance(rgba, S, guides, p)
        else:
            cv[..., 3] = S * F(K) if lum_stop else np.where(np.isfinite(S), F(0), S)
    return _iterate(cv, guides, p, np.full(S.shape, lum_stop), variance != 0 and lum_stop)


def filtered_tiles(rgba, S, tile_frames, guides, params=None, mode=0, spatial_frames=3, k_of=None):
    """((f, u), K_p) of an adaptive accumulation: the last iteration's output of denoise_tiles_ref.denoise_tiles."""
    p = dict(DEFAULTS, **(params or {}))
    rgba = np.asarray(rgba, F)
    S = np.asarray(S, F)
    rows, width = S.shape
    K, spatial, stop = pixel_state(tile_frames, rows, width, mode, spatial_frames, k_of or library_k())
    cv = np.empty(rgba.shape, F)
    cv[..., :3] = rgba[..., :3]
    cv[..., 3] = initial_variance(rgba, S, guides, p, K, spatial)
    return _iterate(cv, guides, p, stop, mode != 0), K


def blend(rgba, S, fu, K, index, gain, broken=None):
    """The blend itself, float32: rgba the frame, fu = (f, u), K a float or an array per pixel (+inf: not valid), index the
    guides' sphere index.  broken: a wrong definition on purpose, "v_plus_u" (n = v + u) or "dx_then_dy" (the window's order)."""
    rgba = np.asarray(rgba, F)
    S = np.asarray(S, F)
    fu = np.asarray(fu, F)
    index = np.asarray(index, np.int32)
    K = np.broadcast_to(np.asarray(K, F), S.shape)
    gain = F(gain)
    c, f, u = rgba[..., :3], fu[..., :3], fu[..., 3]
    with np.errstate(all="ignore"):
        valid = np.isfinite(c).all(-1) & np.isfinite(S) & np.isfinite(fu).all(-1) & np.isfinite(K)
        d = lum(f) - lum(c)
        d2 = d * d
        v = S * K
        n = np.fmax(v + u if broken == "v_plus_u" else v - u, F(0))
        e = np.zeros(S.shape, F)
        m = np.zeros(S.shape, F)
        offsets = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
        if broken == "dx_then_dy":
            offsets = [(dy, dx) for dx in range(-R, R + 1) for dy in range(-R, R + 1)]
        for dy, dx in offsets:
            ok = _shift(valid, dy, dx, False) & (_shift(index, dy, dx, 0) == index)
            e = e + np.where(ok, _shift(d2, dy, dx, F(0)), F(0)).astype(F)
            m = m + np.where(ok, _shift(n, dy, dx, F(0)), F(0)).astype(F)
        a = np.where(e > F(0), np.fmin(m / (gain * e), F(1)), F(0)).astype(F)
        out = np.empty_like(rgba)
        out[..., :3] = np.where(valid[..., None], c + a[..., None] * (f - c), f)
        out[..., 3] = rgba[..., 3]
    return out


def blend_f64(rgba, S, fu, K, index, gain):
    """The same definition per pixel in float64 (no float32 rounding): what blend() approximates."""
    rgba64, S64, fu64 = (np.asarray(a, np.float64) for a in (rgba, S, fu))
    index = np.asarray(index)
    rows, width = S64.shape
    K = np.broadcast_to(np.asarray(K, F), S64.shape).astype(np.float64)
    L = lambda c: (0.2126 * c[0] + 0.7152 * c[1]) + 0.0722 * c[2]
    valid = np.isfinite(rgba64[..., :3]).all(-1) & np.isfinite(S64) & np.isfinite(fu64).all(-1) & np.isfinite(K)
    out = np.empty_like(rgba64)
    out[..., :3] = fu64[..., :3]
    out[..., 3] = rgba64[..., 3]
    for y in range(rows):
        for x in range(width):
            if not valid[y, x]:
                continue
            e = m = 0.0
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    yq, xq = y + dy, x + dx
                    if not (0 <= yq < rows and 0 <= xq < width) or not valid[yq, xq] or index[yq, xq] != index[y, x]:
                        continue
                    dq = L(fu64[yq, xq]) - L(rgba64[yq, xq])
                    e += dq * dq
                    m += max(S64[yq, xq] * K[yq, xq] - fu64[yq, xq, 3], 0.0)
            a = min(m / (float(F(gain)) * e), 1.0) if e > 0 else 0.0
            out[y, x, :3] = rgba64[y, x, :3] + a * (fu64[y, x, :3] - rgba64[y, x, :3])
    return out


def denoise_mix(rgba, S, K, guides, params=None, variance=0, gain=1.0, broken=None):
    """Bit for bit what mrt_debug_denoise_mix computes with the blend on (and a uniform accumulation's denoise with
    mrt_set_denoise_mix on).  K = +inf: the filter's image."""
    fu = filtered(rgba, S, K, guides, params, variance)
    if math.isinf(K):
        out = fu.copy()
        out[..., 3] = np.asarray(rgba, F)[..., 3]
        return out
    return blend(rgba, S, fu, K, guides["index"], gain, broken)


def denoise_mix_tiles(rgba, S, tile_frames, guides, params=None, mode=0, spatial_frames=3, k_of=None, gain=1.0):
    """Bit for bit what mrt_read_denoised computes for a diverged accumulation with mrt_set_denoise_adaptive and the blend on."""
    fu, K = filtered_tiles(rgba, S, tile_frames, guides, params, mode, spatial_frames, k_of)
    return blend(rgba, S, fu, K, guides["index"], gain)


# ---- the quality curve from the oracle's frames (scripts/denoise_mix_quality.py; the tests' quality assertion) ----------------
def host_guides(O, spheres, cam_raw, w, h):
    """The first-hit guides of a scene on the host (tests/test_gpu_denoise.py holds the device's to these bit for bit)."""
    from denoise_ref import centre_rays, expected_guides
    rays = centre_rays(w, h, cam_raw)
    hit, t, normal, albedo = expected_guides(O, spheres, rays)
    return {"index": hit.reshape(h, w).astype(np.int32), "t": t.reshape(h, w), "normal": normal.reshape(h, w, 3),
            "albedo": albedo.reshape(h, w, 3)}


def oracle_accumulations(O, spheres, cam, w, h, seed, counts, depth=50, max_w=1.0, noise=True):
    """{n: (fb, S, K)} after n 1-spp frames of `seed` for every n of counts: the oracle's frames (bit for bit the device's) through
    tests/noise_ref.py's tracked blend.  noise False: the framebuffer alone (S, K None), by the oracle's own blend."""
    import noise_ref
    from common import to_oracle_camera, to_oracle_spheres
    packed = O.pack_world(to_oracle_spheres(O, spheres))
    ocam = to_oracle_camera(O, cam)
    seeds = O.fill_seeds(seed, w, h)
    fb = np.zeros((h, w, 4), np.float32)
    S = np.zeros((h, w), np.float32)
    c2 = 1.0
    out = {}
    for k in range(max(counts)):
        wgt = O.frame_weight(k, max_w)
        if noise:
            mean = O.render_frame(w, h, 1, depth, packed, ocam, seeds, O.frame_shuffle(seed, k), 0.0)
            S = noise_ref.s_update(S, mean, fb, wgt)
            fb = noise_ref.blend(mean, fb, wgt)
            c2 = noise_ref.c2_next(c2, wgt)
        else:
            fb = O.render_frame(w, h, 1, depth, packed, ocam, seeds, O.frame_shuffle(seed, k), wgt, fb)
        if k + 1 in counts:
            out[k + 1] = (fb.copy(), S.copy(), noise_ref.factor(c2)) if noise else (fb.copy(), None, None)
    return out


def rmse(a, b):
    d = np.asarray(a)[..., :3].astype(np.float64) - np.asarray(b)[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


# The quality assertion's setup (tests/test_denoise_mix_host.py and its repetition on the GPU): the cover scene without glass at
# 160 x 96 x 1 spp, seed 7 after 32 and 64 frames against 512 frames of seed 101, default parameters, accumulated mode.
QUALITY = {"w": 160, "h": 96, "seed": 7, "ref_seed": 101, "ref_frames": 512, "counts": (32, 64), "depth": 50}
_quality = {}


def quality_figures_host(O, M):
    """{frames: (rmse_noisy, rmse_denoised, rmse_blend at the default gain)} on the host, computed once."""
    if not _quality:
        q = QUALITY
        sp, cam = M.scene_cover(1, False)
        guides = host_guides(O, sp, M.camera_derive(cam), q["w"], q["h"])
        ref = oracle_accumulations(O, sp, cam, q["w"], q["h"], q["ref_seed"], [q["ref_frames"]], q["depth"], noise=False)[q["ref_frames"]][0]
        gain = M.denoise_mix_default()["gain"]
        for n, (fb, S, K) in oracle_accumulations(O, sp, cam, q["w"], q["h"], q["seed"], q["counts"], q["depth"]).items():
            fu = filtered(fb, S, K, guides)
            _quality[n] = (rmse(fb, ref), rmse(fu, ref), rmse(blend(fb, S, fu, K, guides["index"], gain), ref))
    return _quality
