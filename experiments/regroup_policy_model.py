#!/usr/bin/env python3
"""CPU model behind mrt_set_auto_regroup: how strongly the policy's figure -- Q, the sum over the levels of the
sum of R^2 over a level's nodes (tests/regroup_ref.py, sum_r2) -- responds as a scene moves under a kept grouping, and when the
rule "regroup when Q > ratio x Q right after the previous regroup" fires.  No GPU.

Scenes: mrt_scene_stress(1, 100) and mrt_scene_stress(1, 40); motion: DESIGN.md 7e's random walk, `walk` x the scene's size a
step; the figure is looked at every `check` steps.  (1) Q kept / Q regrouped after a number of steps; (2) for each ratio, the
steps at which the rule fires over `steps` steps, every regroup by tests/regroup_ref.py's ordering.
    python experiments/regroup_policy_model.py [--steps 400] [--check 8] [--walk 0.0005] [--ratios 1.5 2 3 4]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import myraytracer_amd as M  # noqa: E402
import regroup_ref as G  # noqa: E402
from myraytracer_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=400)
ap.add_argument("--check", type=int, default=8)
ap.add_argument("--walk", type=float, default=0.0005)
ap.add_argument("--ratios", type=float, nargs="*", default=[1.5, 2.0, 3.0, 4.0])
ap.add_argument("--at", type=int, nargs="*", default=[8, 24, 48, 96, 200, 400])
a = ap.parse_args()
L = _lib.load()


def build(sc):
    """the host builder's level-0 layout of the scene: member_index, the real slots, the hierarchy's slots, levels, n_pool"""
    info = (C.c_uint32 * 10)()
    assert L.mrt_debug_build_hierarchy(sc.ctypes.data, len(sc), 4, 0, None, 0, None, 0, None, 0, None, 0, None, info) == 0
    nodes, midx = np.zeros((info[2], 4), np.float32), np.zeros(info[3], np.uint32)
    assert L.mrt_debug_build_hierarchy(sc.ctypes.data, len(sc), 4, 0, None, 0, nodes.ctypes.data, len(nodes), midx.ctypes.data, len(midx),
                                       None, 0, None, info) == 0
    n_pool = C.c_uint32()
    assert L.mrt_debug_pool_clusters(sc.ctypes.data, len(sc), 4, 0, C.byref(n_pool)) == 0
    real = ~np.isinf(nodes[:info[3], 3])
    return dict(midx=midx, real=real, n_hier=int(info[5] if info[4] else info[3]), levels=int(info[0]), n_pool=n_pool.value)


def figure(h, midx, xyzr):
    return float(sum(G.sum_r2(midx, h["real"], h["n_hier"], h["levels"], xyzr)))


def walk(sc, steps):
    xyzr = np.concatenate([sc["center"].reshape(-1, 3), sc["radius"].reshape(-1, 1)], axis=1).astype(np.float32)
    size = float(np.ptp(xyzr[:-1, :3], axis=0).max())
    rng = np.random.default_rng(1)
    out = []
    for _ in range(steps):
        xyzr = xyzr.copy()
        xyzr[:-1, :3] += (rng.normal(size=(len(xyzr) - 1, 3)) * a.walk * size).astype(np.float32)
        out.append(xyzr)
    return out


for side in (100, 40):
    sc = M.scene_stress(1, side)[0]
    h = build(sc)
    path = walk(sc, a.steps)
    start = np.concatenate([sc["center"].reshape(-1, 3), sc["radius"].reshape(-1, 1)], axis=1).astype(np.float32)
    print(f"mrt_scene_stress(1, {side}): {len(sc)} spheres, {h['n_pool']} pool clusters, {h['levels']} levels; the walk of {a.walk} x the scene's size a step", flush=True)
    print("(1) Q with the grouping kept / Q regrouped, after")
    for n in a.at:
        if n <= a.steps:
            xyzr = path[n - 1]
            kept = figure(h, h["midx"], xyzr)
            new = figure(h, G.regroup(h["midx"], h["real"], h["n_pool"], xyzr[:, :3]), xyzr)
            print(f"  {n:4d} steps: {kept / new:.2f}", flush=True)
    print(f"(2) the rule, looked at every {a.check} steps over {a.steps} steps")
    for ratio in a.ratios:
        midx, fired = h["midx"], []
        q_ref = figure(h, midx, start)                               # the build's figure is the first reference
        for n in range(a.check, a.steps + 1, a.check):
            xyzr = path[n - 1]
            if figure(h, midx, xyzr) > ratio * q_ref:
                midx = G.regroup(midx, h["real"], h["n_pool"], xyzr[:, :3])
                q_ref = figure(h, midx, xyzr)
                fired.append(n)
        print(f"  ratio {ratio:g}: {len(fired)} regroups, at steps {', '.join(map(str, fired))}", flush=True)
