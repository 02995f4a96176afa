#!/usr/bin/env python3
"""CPU model of the small-scene sweep's output on the cover scene with glass (bench.py's C3): how many top-level bounds the
rays of whole paths make candidates, under the kernel's rule (stretched line test, bounds entirely behind the origin dropped),
and what that means per wave of 64 rays: cluster items, node rounds (ceil(items / 64)), the busiest lane.

Rows: the world-space records (D = I, what the SGPR-fed sweep tests), then the records the library builds for the matrix-core
sweep in the scaled space x' = D (x - origin) (hierarchy.cpp, build_sweep_operand) for a list of forced D and for the D the
library chooses for the scene.  Rays: 4,096 camera rays and their diffuse bounces against the oracle's world_hit_batch, to depth 12.

    python experiments/cand_hist.py            (library and oracle built: make; CPU only, about a minute)

The committed phase profile (profiles/r05_c3_phase_profile.txt) has 217-223 items and 3.9-4.0 node rounds per wave; the D = I row
reproduces it.  The last line is the figure DESIGN_HISTORY.md quotes: items per wave under the chosen D against D = I."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import myraytracer_amd as M                     # noqa: E402
from myraytracer_amd import _lib                # noqa: E402
from oracle import pyoracle as O                # noqa: E402
from common import to_oracle_spheres            # noqa: E402

STRETCH2 = 1.0001 ** 2


def sweep_records(sc, axis=None):
    """(records in the sweep's space [n_top, 4], origin, D) as mrt_set_world derives them; axis: a forced D"""
    L = _lib.load()
    sc = np.ascontiguousarray(sc, M.SPHERE_DTYPE)
    force = (C.c_float * 3)(*axis) if axis is not None else None
    ax, org = (C.c_float * 3)(), (C.c_float * 3)()
    info = (C.c_uint32 * 10)()
    assert L.mrt_debug_build_hierarchy(sc.ctypes.data, len(sc), 4, 0, None, 0, None, 0, None, 0, None, 0, None, info) == 0
    rec = np.zeros((info[1], 4), np.float32)
    assert L.mrt_debug_build_sweep(sc.ctypes.data, len(sc), force, ax, rec.ctypes.data, len(rec), None, 0, org, None) == 0
    return rec.astype(np.float64), np.array(list(org), np.float64), np.array(list(ax), np.float64)


def candidates(rays, rec, org, D):
    """per ray: bounds the kernel's test passes -- the unit direction of the scaled line, stretched; bounds behind dropped"""
    o = (rays[:, None, :3].astype(np.float64) - org) * D
    d = rays[:, None, 3:].astype(np.float64) * D
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    oc = o - rec[None, :, :3]
    b = (oc * d).sum(-1)
    c = (oc * oc).sum(-1) + rec[None, :, 3]
    real = np.isfinite(rec[None, :, 3])
    c = np.where(real, c, 1.0)
    ok = (STRETCH2 * b * b - c >= 0) & ~((b >= 0) & (c >= 0)) & real
    return ok.sum(1)


def main():
    rng = np.random.default_rng(5)
    n_rays = 4096
    sc, cam = M.scene_cover(1, True)
    packed = O.pack_world(to_oracle_spheres(O, sc))
    lf, la = np.array(cam.lookfrom, float), np.array(cam.lookat, float)
    fw = (la - lf) / np.linalg.norm(la - lf)
    right = np.cross(fw, np.array(cam.vup, float))
    right /= np.linalg.norm(right)
    up = np.cross(right, fw)
    th = np.tan(np.radians(cam.vfov_deg) / 2)
    u = rng.uniform(-1, 1, n_rays) * th * 16 / 9
    v = rng.uniform(-1, 1, n_rays) * th
    d = fw[None] + u[:, None] * right[None] + v[:, None] * up[None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.repeat(lf[None], n_rays, 0), d], 1).astype(np.float32)
    centers = np.asarray(sc["center"], float).reshape(-1, 3)
    radii = np.asarray(sc["radius"], float)

    chosen = sweep_records(sc)
    rows = [("D = I", sweep_records(sc, (1, 1, 1)))]
    for ax in [(1, 2, 1), (1, 4, 1), (2, 1, 1), (1, 1, 2)]:
        rows.append(("D = diag(%g, %g, %g)" % ax, sweep_records(sc, ax)))
    rows.append(("chosen: diag(%g, %g, %g)" % tuple(chosen[2]), chosen))
    per_depth = [[] for _ in rows]
    for depth in range(12):
        if len(rays) == 0:
            break
        for k, (_, (rec, org, D)) in enumerate(rows):
            per_depth[k].append(candidates(rays, rec, org, D))
        hit, t, _, _ = O.world_hit_batch(packed, rays)
        ok = hit >= 0
        r = rays[ok].astype(float)
        p = r[:, :3] + t[ok, None] * r[:, 3:]
        n = (p - centers[hit[ok]]) / radii[hit[ok], None]
        s = rng.normal(size=n.shape)
        s /= np.linalg.norm(s, axis=1, keepdims=True)
        nd = n + s
        nd /= np.linalg.norm(nd, axis=1, keepdims=True)
        rays = np.concatenate([p, nd], 1).astype(np.float32)
    print("| records | candidates per ray (camera / bounce) | items per wave | node rounds | busiest lane |")
    print("|---|---|---|---|---|")
    items = {}
    for (name, _), a in zip(rows, per_depth):
        kk = np.concatenate(a)
        w = kk[np.random.default_rng(11).permutation(len(kk))][: len(kk) // 64 * 64].reshape(-1, 64)
        items[name] = w.sum(1).mean()
        print(f"| {name} | {kk.mean():.2f} ({a[0].mean():.2f} / {np.concatenate(a[1:]).mean():.2f}) | {w.sum(1).mean():.0f} | "
              f"{np.ceil(w.sum(1) / 64).mean():.2f} | {w.max(1).mean():.1f} |")
    base, got = items["D = I"], items[rows[-1][0]]
    print(f"items per wave, chosen D against D = I: {got:.1f} / {base:.1f} = {got / base:.3f} ({100 * (1 - got / base):.1f} % fewer)")
    return 0 if got <= 0.85 * base else 1


if __name__ == "__main__":
    sys.exit(main())
