#!/usr/bin/env python3
"""Dev helper: what the temporal response buys where the picture changes BEHIND an unchanged first hit -- the table of
   profiles/temporal_response_quality.txt.
   The scene (made here): a ground, one large mirror (Metal, fuzz 0), one large glass sphere and six small saturated Lambertian
   spheres that are seen reflected and refracted in the two.  96x64, 1 spp, depth 12, max_framebuffer_weight 0, a fixed camera.
   Steps 1 .. 16 are static and fill the history; before step 17 the small spheres JUMP to other places; steps 17 .. 24 are
   static again.  Ground truth: a 512-spp render of each of the two geometries (seed 101).
   The GHOST REGION is the set of pixels whose first-hit sphere index and distance are the same before and after the jump: the
   history's index and depth tests accept every tap there, whatever the mirror and the glass now show.  Reported: the RMSE of the
   temporal image in the ghost region at steps 18, 20 and 24, and over the whole image the mean RMSE of the static steps 9 .. 16,
   with the response on (fast_history x clamp_sigma, antilag 1) against the same run with it off.  Seeds 7 and 8.
   python scripts/temporal_response_quality.py [--host] [--out FILE]
   Default: on the GPU through the library (the default setting only).  --host: the whole grid on the CPU -- the oracle's frames
   (bit-identical to the GPU's, tests/test_gpu_parity.py), guides made from the oracle's closest hits, tests/temporal_ref.py and
   tests/temporal_response_ref.py, which the GPU tests hold the kernels to bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

W, H, DEPTH = 96, 64, 12
FILL, JUMP_AT, LAST = 16, 17, 24
GHOST_STEPS = (18, 20, 24)
STATIC_STEPS = tuple(range(9, 17))
SEEDS = (7, 8)
REF_SEED, REF_SPP = 101, 512
GRID = [(fh, cs) for fh in (2, 4, 8) for cs in (1.0, 2.0, 3.0)]
F = np.float32

# (centre, radius, material type 1 Lambertian / 2 Metal / 3 Dielectric, albedo, fuzz or index of refraction)
BIG = [((0.0, -1000.0, 0.0), 1000.0, 1, (0.5, 0.5, 0.5), 0.0),
       ((-1.05, 1.0, 0.0), 1.0, 2, (0.9, 0.9, 0.9), 0.0),
       ((1.05, 1.0, 0.0), 1.0, 3, (1.0, 1.0, 1.0), 1.5)]
SMALL_R = 0.3
SMALL = [((1.0, 0.05, 0.05), (-0.45, 0.3, 1.9), (0.55, 0.3, 2.1)),      # albedo, centre before the jump, centre after it
         ((0.05, 0.9, 0.1), (0.5, 0.3, 1.7), (-0.6, 0.3, 1.6)),
         ((0.1, 0.15, 1.0), (1.3, 0.3, -2.2), (0.6, 0.3, -2.4)),
         ((1.0, 0.85, 0.05), (-2.5, 0.3, 1.2), (-2.3, 0.3, -0.6)),
         ((0.95, 0.05, 0.9), (2.6, 0.3, 1.0), (2.2, 0.3, 2.2)),
         ((0.05, 0.9, 0.9), (0.0, 0.3, 3.2), (-1.4, 0.3, 3.0))]
CAMERA = dict(mode=1, lookfrom=(0.0, 1.3, 5.2), lookat=(0.0, 0.85, 0.0), vup=(0.0, 1.0, 0.0), vfov_deg=36.0, defocus_angle_deg=0.0,
              focus_dist=1.0)


def scene(M):
    """(the spheres before the jump, (n, 4) centre + radius after it, the camera)"""
    s = np.zeros(len(BIG) + len(SMALL), M.SPHERE_DTYPE)
    for k, (c, r, ty, a, p) in enumerate(BIG):
        s[k] = (c, r, ty, a, p)
    for k, (a, c0, _) in enumerate(SMALL, len(BIG)):
        s[k] = (c0, SMALL_R, 1, a, 0.0)
    after = np.concatenate([s["center"].reshape(-1, 3), s["radius"].reshape(-1, 1)], 1).astype(F)
    for k, (_, _, c1) in enumerate(SMALL, len(BIG)):
        after[k, :3] = c1
    return s, after, M.Camera(**CAMERA)


def xyzr_of(s):
    return np.concatenate([s["center"].reshape(-1, 3), s["radius"].reshape(-1, 1)], 1).astype(F)


def rmse(a, b, mask=None):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    d = (d * d).sum(-1) / 3
    return float(np.sqrt(d[mask].mean() if mask is not None else d.mean()))


def ghost_region(g0, g1):
    """the pixels whose first hit is the same sphere at the same distance before and after the jump; the reference's own check
    that the comparison is over something: at least 5 % of the image"""
    mask = (g0["index"] == g1["index"]) & (np.asarray(g0["t"]).view(np.uint32) == np.asarray(g1["t"]).view(np.uint32))
    assert mask.mean() >= 0.05, f"the ghost region holds {mask.mean():.3f} of the image"
    return mask


def summarise(images, truths, mask):
    """images: {step: temporal image}; -> ({step: ghost region RMSE}, mean whole-image RMSE over the static steps)"""
    truth = lambda k: truths[0] if k < JUMP_AT else truths[1]
    return ({k: rmse(images[k], truth(k), mask) for k in GHOST_STEPS}, float(np.mean([rmse(images[k], truth(k)) for k in STATIC_STEPS])))


def gpu_run(M, seed, rp=None):
    """the run with the response on (rp over the defaults) and off, on the GPU: {"ghost_share", "ghost": {step: (on, off)},
    "static": (on, off), "static_ratio"}"""
    spheres, after, cam = scene(M)

    def state(spp, s, max_w):
        st = M.State(M.Args(W, H, spp, DEPTH, max_w), seed=s)
        st.set_world(spheres)
        st.set_camera(cam)
        return st
    with state(REF_SPP, REF_SEED, 1.0) as ref:
        ref.redraw()
        truths = [ref.read_framebuffer()]
        ref.reset()
        ref.update_spheres(0, after)
        ref.redraw()
        truths.append(ref.read_framebuffer())
    with state(1, seed, 0.0) as on, state(1, seed, 0.0) as off:
        on.set_temporal(True)
        off.set_temporal(True)
        on.set_temporal_response(True, **(rp or {}))
        g0 = on.debug_read_guides()
        imgs = {"on": {}, "off": {}}
        for k in range(1, LAST + 1):
            for name, st in (("on", on), ("off", off)):
                if k == JUMP_AT:
                    st.update_spheres(0, after)
                st.redraw()
                st.temporal_step()
                if k in GHOST_STEPS or k in STATIC_STEPS:
                    imgs[name][k] = st.read_temporal()
        mask = ghost_region(g0, on.debug_read_guides())
    (g_on, s_on), (g_off, s_off) = summarise(imgs["on"], truths, mask), summarise(imgs["off"], truths, mask)
    return {"ghost_share": float(mask.mean()), "ghost": {k: (g_on[k], g_off[k]) for k in GHOST_STEPS}, "static": (s_on, s_off),
            "static_ratio": s_on / s_off}


def host_runs(seeds=SEEDS, grid=GRID):
    """{seed: {None | (fast_history, clamp_sigma): ({step: ghost RMSE}, static RMSE)}}, ghost share: the whole grid on the CPU"""
    import myraytracer_amd as M
    from oracle import pyoracle as O
    from common import to_oracle_camera, to_oracle_spheres
    from denoise_ref import centre_rays
    from temporal_quality import host_guides
    from temporal_ref import camera_matrix, image
    from temporal_ref import step as plain_step
    from temporal_response_ref import step
    spheres, after, cam = scene(M)
    ocam = to_oracle_camera(O, cam)
    raw = M.camera_derive(cam)
    rays = centre_rays(W, H, raw)
    Mx, o_prev = camera_matrix(raw)
    geo = []
    for xyzr in (xyzr_of(spheres), after):
        sc = spheres.copy()
        sc["center"], sc["radius"] = xyzr[:, :3], xyzr[:, 3]
        packed = O.pack_world(to_oracle_spheres(O, sc))
        geo.append((xyzr, packed, host_guides(O, spheres, xyzr, rays), O.render(W, H, REF_SPP, DEPTH, packed, ocam, REF_SEED)))
    mask = ghost_region(geo[0][2], geo[1][2])
    truths = [geo[0][3], geo[1][3]]
    out = {}
    for seed in seeds:
        seedtex = O.fill_seeds(seed, W, H)
        settings = [None] + list(grid)
        hist = {s: tuple(np.zeros((H, W, 4), F) for _ in range(3)) for s in settings}
        imgs = {s: {} for s in settings}
        prev = geo[0][0]
        for k in range(1, LAST + 1):
            xyzr, packed, g, _ = geo[0] if k < JUMP_AT else geo[1]
            fb = O.render_frame(W, H, 1, DEPTH, packed, ocam, seedtex, O.frame_shuffle(seed, k - 1), 0.0)
            for s in settings:
                if s is None:
                    h0, h1, _ = plain_step(fb, rays, g["index"], g["t"], xyzr, prev, Mx, o_prev, *hist[s][:2])
                    h2 = hist[s][2]
                else:
                    h0, h1, h2, _ = step(fb, rays, g["index"], g["t"], xyzr, prev, Mx, o_prev, *hist[s], None,
                                         {"fast_history": s[0], "clamp_sigma": s[1], "antilag": 1.0})
                hist[s] = (h0, h1, h2)
                if k in GHOST_STEPS or k in STATIC_STEPS:
                    imgs[s][k] = image(h0, h1, fb[..., 3], g)
            prev = xyzr
            print(f"seed {seed} step {k}", file=sys.stderr, flush=True)
        out[seed] = {s: summarise(imgs[s], truths, mask) for s in settings}
    return out, float(mask.mean())


def table(runs, share):
    lines = [f"{W}x{H} x 1 spp, depth {DEPTH}; ghost region {share:.3f} of the image; antilag 1; RMSE against {REF_SPP} spp"]
    for seed, res in runs.items():
        g_off, s_off = res[None]
        lines.append(f"seed {seed}")
        lines.append("  fast_history clamp_sigma   ghost region RMSE at step " + " ".join(f"{k:8d}" for k in GHOST_STEPS) +
                     "   on / off at those steps    static 9..16 RMSE   on / off")
        lines.append("           off         off                             " + " ".join(f"{g_off[k]:8.5f}" for k in GHOST_STEPS) +
                     f"                              {s_off:17.5f}")
        for s, (g, st) in res.items():
            if s is None:
                continue
            lines.append(f"  {s[0]:12d} {s[1]:11.1f}                             " + " ".join(f"{g[k]:8.5f}" for k in GHOST_STEPS) + "   " +
                         " ".join(f"{g[k] / g_off[k]:7.3f}" for k in GHOST_STEPS) + f"   {st:17.5f}   {st / s_off:8.4f}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    argv = sys.argv[1:]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    if "--host" in argv:
        runs, share = host_runs()
        text = table(runs, share)
    else:
        import myraytracer_amd as M
        lines = []
        for seed in SEEDS:
            r = gpu_run(M, seed)
            lines.append(f"seed {seed} (GPU, the default setting): ghost region {r['ghost_share']:.3f} of the image; ghost RMSE on / off " +
                         ", ".join(f"step {k}: {a:.5f} / {b:.5f}" for k, (a, b) in r["ghost"].items()) +
                         f"; static 9..16 on / off {r['static'][0]:.5f} / {r['static'][1]:.5f} = {r['static_ratio']:.4f}")
        text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
