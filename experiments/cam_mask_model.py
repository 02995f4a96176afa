#!/usr/bin/env python3
"""CPU model of the camera-ray cluster masks (myraytracer_amd/csrc/cam_mask.hip) on the cover scene with glass (bench.py's C3):
what ANDing a texel's entry onto the sweep's candidate words of its camera rays leaves, from the library's own records.

Rays: camera rays of random texels of the image, drawn with the kernel's float32 camera arithmetic (tests/camera_mask_ref.py),
and their diffuse bounces against the oracle's world_hit_batch, as experiments/cand_hist.py follows them.  Candidates: the sweep's
rule on the records the library builds for the matrix-core sweep in the space it chooses (cand_hist.sweep_records / candidates).
Masks: tests/camera_mask_ref.py, the float64 restatement of the build kernel's bound.

    python experiments/cam_mask_model.py [width height]          (library and oracle built: make; CPU only)

Prints the candidates per camera ray without and with the masks, the set bits per entry, and the cluster items and node rounds
per wave of 64 rays (camera and bounce rays mixed as a frame mixes them) without and with them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "experiments"))
import myraytracer_amd as M                     # noqa: E402
from oracle import pyoracle as O                # noqa: E402
from common import to_oracle_spheres            # noqa: E402
import camera_mask_ref as R                     # noqa: E402
from cand_hist import STRETCH2, sweep_records   # noqa: E402


def candidate_matrix(rays, rec, org, D):
    """[rays, records] bool: the sweep's candidates (cand_hist.candidates, before the count)"""
    o = (rays[:, None, :3].astype(np.float64) - org) * D
    d = rays[:, None, 3:].astype(np.float64) * D
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    oc = o - rec[None, :, :3]
    b = (oc * d).sum(-1)
    c = (oc * oc).sum(-1) + rec[None, :, 3]
    real = np.isfinite(rec[None, :, 3])
    c = np.where(real, c, 1.0)
    return (STRETCH2 * b * b - c >= 0) & ~((b >= 0) & (c >= 0)) & real


def camera_ray_model(sc, cam, W, H, n_texels, seed=5, per_texel=2):
    """the sampled texels' camera rays: (rays, their texels, sweep candidates [rays, records], mask bits of their entries [rays, 128])"""
    rng = np.random.default_rng(seed)
    raw = M.camera_derive(cam) if cam is not None else None
    members, index, n_top, direct_first = R.host_hierarchy(M, sc)
    n_tex = R.local_texels(W, H)
    px_all, py_all = R.texel_pixels(n_tex, W)
    ok = np.nonzero(py_all < H)[0]
    tex = rng.choice(ok, min(n_texels, len(ok)), replace=False)
    rays, ray_tex = R.camera_rays(raw, W, H, tex, px_all[tex], py_all[tex], rng, per_texel)
    rec, org, D = sweep_records(sc)
    cand = candidate_matrix(rays, rec, org, D)
    ent, inv = np.unique(ray_tex >> 3, return_inverse=True)
    bits = R.mask_bits(R.camera_masks_ref(members, n_top, direct_first, raw, W, H, only=ent))[inv]
    return rays, ray_tex, cand, bits[:, :cand.shape[1]]


def main():
    W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) == 3 else (1920, 1080)
    sc, cam = M.scene_cover(1, True)
    rays, _, cand, bits = camera_ray_model(sc, cam, W, H, 2048)
    packed = O.pack_world(to_oracle_spheres(O, sc))
    rec, org, D = sweep_records(sc)
    centers = np.asarray(sc["center"], float).reshape(-1, 3)
    radii = np.asarray(sc["radius"], float)
    rng = np.random.default_rng(7)
    plain, culled = [cand.sum(1)], [(cand & bits).sum(1)]
    print(f"{W} x {H}: sweep candidates per camera ray {plain[0].mean():.2f}, with the masks {culled[0].mean():.2f}; "
          f"set bits per entry {bits.sum(1).mean():.2f}")
    for _ in range(11):
        hit, t, _, _ = O.world_hit_batch(packed, rays)
        ok = hit >= 0
        if not ok.any():
            break
        r = rays[ok].astype(float)
        p = r[:, :3] + t[ok, None] * r[:, 3:]
        n = (p - centers[hit[ok]]) / radii[hit[ok], None]
        s = rng.normal(size=n.shape)
        s /= np.linalg.norm(s, axis=1, keepdims=True)
        nd = n + s
        nd /= np.linalg.norm(nd, axis=1, keepdims=True)
        rays = np.concatenate([p, nd], 1).astype(np.float32)
        k = candidate_matrix(rays, rec, org, D).sum(1)
        plain.append(k)
        culled.append(k)
    for name, a in (("without masks", plain), ("with masks", culled)):
        kk = np.concatenate(a)
        w = kk[np.random.default_rng(11).permutation(len(kk))][: len(kk) // 64 * 64].reshape(-1, 64)
        print(f"{name}: candidates per ray {kk.mean():.2f} (camera {a[0].mean():.2f} / bounce {np.concatenate(a[1:]).mean():.2f}), "
              f"items per wave {w.sum(1).mean():.0f}, node rounds {np.ceil(w.sum(1) / 64).mean():.2f}; "
              f"camera rays are {len(a[0]) / len(kk):.2f} of the rays and supply {a[0].sum() / kk.sum():.2f} of the items")
    return 0


if __name__ == "__main__":
    sys.exit(main())
