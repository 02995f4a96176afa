#!/usr/bin/env python3
"""CPU model behind adaptive sampling by budget ("By budget"): what the allocation should buy, from the oracle's
frames at a small size, before anything runs on a GPU.

The cover-glass scene at W x H x 1 spp.  Frame k is the oracle's frame with shuffle mrt_frame_shuffle(seed, k); the accumulation
is tests/adaptive_ref.py's (every tile blended at its own frame count, S by the library's recursion), the tile map and the
allocation are tests/budget_ref.py's.  Three rules spend the samples of FRAMES uniform frames:
  uniform     FRAMES whole frames
  threshold   START whole frames, then chunks of EVERY subset frames over the tiles whose largest rel is above THR (render_adaptive's
              rule), until the samples are spent
  greedy      START whole frames, then chunks of render_budget(CHUNK x tiles tile-frames, MAX_FRAMES) from the summed-S map of the
              state before the chunk (no lag: the model asks what the rule buys, not what the pipeline costs)
and each reports the RGB RMSE against REF uniform frames of other shuffles, the luminance error summed per tile next to the
model's own figure sum of s_t K(n_t), and the spread of n_t.

    python experiments/budget_model.py [W H] [--frames 40] [--ref 1600]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adaptive_ref  # noqa: E402
import budget_ref  # noqa: E402
import myraytracer_amd as M  # noqa: E402  (the scenes only: host functions)
import noise_ref  # noqa: E402
from common import to_oracle_camera, to_oracle_spheres  # noqa: E402
from oracle import pyoracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="*", type=int, default=[96, 64])
ap.add_argument("--frames", type=int, default=40)
ap.add_argument("--ref", type=int, default=1600)
ap.add_argument("--start", type=int, default=8)
ap.add_argument("--every", type=int, default=4)
ap.add_argument("--thr", type=float, default=0.1)
ap.add_argument("--floor", type=float, default=0.05)
ap.add_argument("--chunk", type=int, default=2)
ap.add_argument("--max-frames", type=int, default=8)
ap.add_argument("--depth", type=int, default=16)
a = ap.parse_args()
W, H = a.size
SEED, MAX_W = 1, 1.0
O.lib()
spheres, cam = M.scene_cover(1, True)
ARGS = (W, H, 1, a.depth, O.pack_world(to_oracle_spheres(O, spheres)), to_oracle_camera(O, cam))
SEEDS = O.fill_seeds(SEED, W, H)
_cache = {}


def mean(k):
    if k not in _cache:
        _cache[k] = O.render_frame(*ARGS, SEEDS, O.frame_shuffle(SEED, k), 0.0)
    return _cache[k]


ref = np.zeros((H, W, 4), np.float64)
for k in range(a.ref):                                   # frames of their own: shuffles 10000 .., never used by a run
    ref += O.render_frame(*ARGS, SEEDS, O.frame_shuffle(SEED, 10000 + k), 0.0)
ref /= a.ref
n_tiles = adaptive_ref.Accum(H, W, MAX_W).n_tiles
total = (a.frames - a.start) * n_tiles                   # tile-frames after the start: the samples of `frames` uniform frames


def start():
    acc = adaptive_ref.Accum(H, W, MAX_W)
    for _ in range(a.start):
        acc.frame(mean(acc.frames_done))
    return acc


def uniform():
    acc = start()
    for _ in range(a.frames - a.start):
        acc.frame(mean(acc.frames_done))
    return acc


def threshold():
    acc, left = start(), total
    while left > 0:
        sel = adaptive_ref.select(acc.tiles(a.thr, a.floor), a.thr)
        if len(sel) == 0:
            break
        for _ in range(a.every):
            if left < len(sel):
                sel = sel[:left]
            if len(sel) == 0:
                break
            acc.frame(mean(acc.frames_done), sel)
            left -= len(sel)
    return acc


def greedy():
    acc, left = start(), total
    while left > 0:
        k, res = budget_ref.allocate(budget_ref.tile_sums(acc.S, acc.fb), acc.n, MAX_W, min(a.chunk * n_tiles, left), a.max_frames)
        if res["tile_frames"] == 0:
            break
        for tiles, run in budget_ref.levels(k):
            for _ in range(run):
                acc.frame(mean(acc.frames_done), tiles)
        left -= res["tile_frames"]
    return acc


print(f"cover-glass {W}x{H} x 1 spp, depth {a.depth}, {n_tiles} tiles; the samples of {a.frames} uniform frames; reference: {a.ref} frames")
base = None
for name, run in (("uniform", uniform), ("threshold", threshold), ("greedy", greedy)):
    acc = run()
    d = acc.fb[..., :3].astype(np.float64) - ref[..., :3]
    rmse = float(np.sqrt(np.mean(d * d)))
    dl = noise_ref.lum(acc.fb).astype(np.float64) - noise_ref.lum(ref.astype(np.float32)).astype(np.float64)
    K = budget_ref.k_values(int(acc.n.max()), MAX_W)
    model = float((budget_ref.tile_sums(acc.S, acc.fb).ravel().astype(np.float64) * K[acc.n]).sum())
    base = base or rmse
    print(f"  {name:10s} tile-frames {int(acc.n.sum()):7d}  rmse {rmse:.5f} ({rmse / base:.3f} x uniform)  luminance error^2 summed "
          f"{float((dl * dl).sum()):.4f}, the model's sum of s_t K(n_t) {model:.4f}  n_t {int(acc.n.min())}..{int(acc.n.max())}")
