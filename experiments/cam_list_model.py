#!/usr/bin/env python3
"""CPU model of the camera-ray sphere lists (myraytracer_amd/csrc/cam_mask.hip, the second table; the primary hit in the lane:
kernels.hip) on the cover scene with glass (bench.py's C3): how long the lists are, how many camera rays hit, and what taking the
camera ray out of the world_hit iteration does to the lane slots a sample costs.

Lists: tests/camera_list_ref.py, the float64 restatement of the build kernel's bound, for random entries and for the 8 entries of
random 8x8 tiles.  Rays: camera rays of the sampled entries' texels in the kernel's float32 camera arithmetic
(tests/camera_mask_ref.py) against the oracle's world_hit_batch.  world_hit calls per sample: the oracle's counters on a small frame.

    python experiments/cam_list_model.py [width height [entries]]          (library and oracle built: make; CPU only)

Lane slots per sample: today every world_hit call of a sample is a slot of its lane's wave iteration, and a sample whose path has
ended idles none (it starts the next one in the same tail): calls / utilisation.  With the lists the camera ray is resolved in the
tail: a sample whose camera ray hits costs its bounces, one that misses one idle slot: (calls - 1) + (1 - hit fraction)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import myraytracer_amd as M                     # noqa: E402
from oracle import pyoracle as O                # noqa: E402
from common import oracle_render, to_oracle_spheres   # noqa: E402
import camera_list_ref as L                     # noqa: E402
import camera_mask_ref as R                     # noqa: E402

LANE_UTILISATION = 0.97                         # C3, profiles/cam_mask_rates.txt's session (bench.py: roofline.lane_utilisation)


def pct(a, qs=(50, 90, 99, 99.9)):
    return ", ".join(f"p{q:g} {np.percentile(a, q):.0f}" for q in qs)


def main():
    W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) >= 3 else (1920, 1080)
    n_entries = int(sys.argv[3]) if len(sys.argv) >= 4 else 20000
    sc, cam = M.scene_cover(1, True)
    raw = M.camera_derive(cam)
    members, index, n_top, direct_first = R.host_hierarchy(M, sc)
    rng = np.random.default_rng(5)
    n_tex = R.local_texels(W, H)
    px_all, py_all = R.texel_pixels(n_tex, W)
    on_image = np.nonzero((py_all < H).reshape(-1, 8).any(1))[0] if n_tex % 8 == 0 else np.arange((n_tex + 7) // 8)
    ent = rng.choice(on_image, min(n_entries, len(on_image)), replace=False)
    lists = L.camera_lists_ref(members, n_top, direct_first, raw, W, H, only=ent)
    n = lists.sum(1)
    print(f"{W} x {H}, {len(ent)} random entries: slots per entry mean {n.mean():.2f}, {pct(n)}, max {n.max()}; "
          f"{(n > L.CAP).sum()} above the cap of {L.CAP}; {(n == 0).mean():.2f} empty")
    if W % 8 == 0:
        tiles_x, tiles_y = W // 8, (H + 7) // 8
        t = rng.choice(tiles_x * tiles_y, min(n_entries // 8, tiles_x * tiles_y), replace=False)
        rows = 8 * (t // tiles_x)[:, None] + np.arange(8)[None]
        te = ((rows * W + 8 * (t % tiles_x)[:, None]) >> 3).reshape(-1)
        tn = L.camera_lists_ref(members, n_top, direct_first, raw, W, H, only=te).sum(1).reshape(-1, 8).max(1)
        print(f"{len(t)} random 8x8 tiles: the longest list among a tile's 8 entries mean {tn.mean():.2f}, {pct(tn)}, max {tn.max()}")
    # camera rays of one texel of every sampled entry
    tex = 8 * ent + rng.integers(0, 8, len(ent))
    tex = tex[(tex < n_tex) & (py_all[np.minimum(tex, n_tex - 1)] < H)]
    rays, _ = R.camera_rays(raw, W, H, tex, px_all[tex], py_all[tex], rng, per_texel=2)
    hit, _, _, _ = O.world_hit_batch(O.pack_world(to_oracle_spheres(O, sc)), rays)
    p_hit = (hit >= 0).mean()
    ground = int(np.argmax(np.asarray(sc["radius"])))
    print(f"{len(rays)} camera rays: {p_hit:.2f} hit something, {(hit == ground).sum() / max(1, (hit >= 0).sum()):.2f} of those the ground sphere")
    cnt = O.Counters()
    oracle_render(O, sc, cam, 240, 135, 8, 50, 1, counters=cnt)
    calls = cnt.world_hit_calls / cnt.samples
    now = calls / LANE_UTILISATION
    then = (calls - 1.0) + (1.0 - p_hit)
    print(f"world_hit calls per sample {calls:.2f} (240 x 135, 8 spp, depth 50); lane slots per sample: {now:.2f} today at "
          f"{LANE_UTILISATION} utilisation, {then:.2f} with the camera ray resolved in the lane ({then / now:.2f} x the wave iterations)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
