#!/usr/bin/env python3
"""Dev helper: what temporal reprojection buys on a moving scene -- the table of profiles/temporal_quality.txt.
   The cover scene with glass (scene_cover(1, True)) at 320x192, 1 spp, depth 50, max_framebuffer_weight 0.  Every step each small
   sphere (|radius| < 0.5) takes the random-walk step of scripts/animation_rates.py (0.0005 x the scene's size, one generator
   seeded 1), then one frame and one mrt_temporal_step.  At steps 1, 2, 4, 8, 16 and 32 the RMSE against a 256-spp render OF THAT
   STEP'S GEOMETRY (seed 101) of three images: the raw frame; the spatial denoiser alone on one frame after a reset (the
   spatial-early variance mode: today's best for one frame); the temporal image.  Seeds 7 and 8.
   python scripts/temporal_quality.py [--host] [--out FILE] [w h]
   Default: on the GPU through the library.  --host: the same computation on the CPU -- the oracle's frames (bit-identical to the
   GPU's, tests/test_gpu_parity.py), guides made from the oracle's closest hits, tests/temporal_ref.py and
   tests/denoise_var_ref.py, which the GPU tests hold the kernels to bit for bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = (1, 2, 4, 8, 16, 32)
SEEDS = (7, 8)
REF_SEED, REF_SPP, DEPTH, WALK = 101, 256, 50, 0.0005
F = np.float32


def rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def geometry(spheres, steps):
    """[(n, 4) centre + radius after step 1, 2, ...]: the small spheres on animation_rates.py's random walk"""
    xyzr = np.concatenate([spheres["center"].reshape(-1, 3), spheres["radius"].reshape(-1, 1)], axis=1).astype(F)
    small = np.abs(xyzr[:, 3]) < 0.5
    size = float(np.ptp(xyzr[small, :3], axis=0).max())
    rng = np.random.default_rng(1)
    out = []
    for _ in range(steps):
        xyzr = xyzr.copy()
        xyzr[small, :3] += (rng.normal(size=(int(small.sum()), 3)) * WALK * size).astype(F)
        out.append(xyzr)
    return out


def gpu_curve(M, seed, w=320, h=192, steps=STEPS):
    """[(step, rmse raw, rmse spatial-only, rmse temporal)] on the GPU"""
    spheres, cam = M.scene_cover(1, True)
    path = geometry(spheres, max(steps))

    def state(spp, s, max_w):
        st = M.State(M.Args(w, h, spp, DEPTH, max_w), seed=s)
        st.set_world(spheres)
        st.set_camera(cam)
        return st
    rows = []
    with state(1, seed, 0.0) as st, state(1, seed, 1.0) as sp, state(REF_SPP, REF_SEED, 1.0) as ref:
        st.set_temporal(True)
        sp.set_noise_tracking(True)
        sp.set_denoise_variance("spatial-early")
        for k, xyzr in enumerate(path, 1):
            st.update_spheres(0, xyzr)
            st.redraw()
            st.temporal_step()
            if k not in steps:
                continue
            ref.reset()
            ref.update_spheres(0, xyzr)
            ref.redraw()
            truth = ref.read_framebuffer()
            sp.reset()
            sp.update_spheres(0, xyzr)
            sp.redraw()
            rows.append((k, rmse(st.read_framebuffer(), truth), rmse(sp.read_denoised(), truth), rmse(st.read_temporal(), truth)))
    return rows


def host_guides(O, spheres, xyzr, rays):
    """the first-hit guides of denoise.hip's guide pass from the oracle's closest hits"""
    from common import to_oracle_spheres
    from denoise_ref import fma32
    sc = spheres.copy()
    sc["center"], sc["radius"] = xyzr[:, :3], xyzr[:, 3]
    hit, t, _, _ = O.world_hit_batch(O.pack_world(to_oracle_spheres(O, sc)), rays.reshape(-1, 6))
    hit, t = hit.reshape(rays.shape[:2]), t.reshape(rays.shape[:2]).astype(F)
    miss = hit < 0
    si = np.where(miss, 0, hit)
    o, d = rays[..., :3], rays[..., 3:]
    with np.errstate(all="ignore"):
        n = ((o + t[..., None] * d) - xyzr[si, :3]) / xyzr[si, 3:4]
        flip = ~(fma32(n[..., 2], d[..., 2], fma32(n[..., 1], d[..., 1], n[..., 0] * d[..., 0])) <= 0)
    n = np.where(flip[..., None], -n, n)
    ty = sc["material_ty"][si]
    albedo = np.where((ty == 1)[..., None] | (ty == 2)[..., None], sc["albedo"][si], np.where((ty == 3)[..., None], F(1), F(0))).astype(F)
    return {"rays": rays, "index": np.where(miss, -1, hit).astype(np.int32), "t": np.where(miss, F(np.inf), t).astype(F),
            "normal": np.where(miss[..., None], -d, n).astype(F), "albedo": np.where(miss[..., None], F(1), albedo).astype(F)}


def host_curves(w=320, h=192, steps=STEPS, seeds=SEEDS):
    """{seed: [(step, rmse raw, rmse spatial-only, rmse temporal)]} on the CPU"""
    import myraytracer_amd as M
    from oracle import pyoracle as O
    from common import to_oracle_camera, to_oracle_spheres
    from denoise_ref import centre_rays
    from denoise_var_ref import denoise_var
    from temporal_ref import camera_matrix, image, step
    spheres, cam = M.scene_cover(1, True)
    path = geometry(spheres, max(steps))
    ocam = to_oracle_camera(O, cam)
    raw = M.camera_derive(cam)
    rays = centre_rays(w, h, raw)
    Mx, o_prev = camera_matrix(raw)
    hist = {s: (np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)) for s in seeds}
    seedtex = {s: O.fill_seeds(s, w, h) for s in seeds}
    rows = {s: [] for s in seeds}
    prev = path[0]
    for k, xyzr in enumerate(path, 1):
        sc = spheres.copy()
        sc["center"], sc["radius"] = xyzr[:, :3], xyzr[:, 3]
        packed = O.pack_world(to_oracle_spheres(O, sc))
        g = host_guides(O, spheres, xyzr, rays)
        truth = O.render(w, h, REF_SPP, DEPTH, packed, ocam, REF_SEED) if k in steps else None
        for s in seeds:
            fb = O.render_frame(w, h, 1, DEPTH, packed, ocam, seedtex[s], O.frame_shuffle(s, k - 1), 0.0)
            h0, h1, _ = step(fb, rays, g["index"], g["t"], xyzr, prev, Mx, o_prev, *hist[s])
            hist[s] = (h0, h1)
            if truth is None:
                continue
            first = O.render_frame(w, h, 1, DEPTH, packed, ocam, seedtex[s], O.frame_shuffle(s, 0), 0.0)
            spatial = denoise_var(first, np.zeros((h, w), F), np.inf, g, None, 2)
            rows[s].append((k, rmse(fb, truth), rmse(spatial, truth), rmse(image(h0, h1, fb[..., 3], g), truth)))
            print(f"seed {s} step {k}: {rows[s][-1][1:]}", file=sys.stderr, flush=True)
        prev = xyzr
    return rows


def table(curves, w, h):
    lines = []
    for seed, rows in curves.items():
        lines.append(f"cover-glass {w}x{h} x 1 spp, seed {seed}, default temporal and denoise parameters")
        lines.append("  step    rmse_raw  spatial-only     temporal   ratio to raw: spatial temporal   temporal / spatial-only")
        for k, a, b, c in rows:
            lines.append(f"{k:6d}  {a:10.5f}  {b:12.5f}  {c:11.5f}                  {b / a:7.3f}  {c / a:7.3f}   {c / b:23.3f}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    argv = sys.argv[1:]
    host = "--host" in argv
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    pos = [x for i, x in enumerate(argv) if not x.startswith("--") and (i == 0 or argv[i - 1] != "--out")]
    w, h = (int(pos[0]), int(pos[1])) if pos else (320, 192)
    if host:
        curves = host_curves(w, h)
    else:
        import myraytracer_amd as M
        curves = {s: gpu_curve(M, s, w, h) for s in SEEDS}
    text = table(curves, w, h)
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
