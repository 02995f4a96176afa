#!/usr/bin/env python3
"""CPU model behind mrt_regroup_spheres: what the regroup's ordering (tests/regroup_ref.py) does to the hierarchy
of a moving scene, against keeping the grouping (mrt_update_spheres alone) and against the host builder's rebuild.  No GPU.

Scene: a jittered n x n grid of spheres of radius 0.15 .. 0.25 resting on a radius-1000 ground (a stand-in for
mrt_scene_stress); motion: DESIGN.md 7e's random walk, `walk` x the scene's size a step.  Per grouping: sum R^2 of the enclosing
spheres per level, and 3,000 rays -- half from a camera above the grid, half bouncing off the ground -- walked top-down through
the bounding spheres: node tests (the levels below the top) and member tests per ray.
    python experiments/regroup_model.py [--side 100] [--steps 200 800] [--walk 0.0005]"""
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
ap.add_argument("--side", type=int, default=100)
ap.add_argument("--steps", type=int, nargs="*", default=[200, 800])
ap.add_argument("--walk", type=float, default=0.0005)
ap.add_argument("--rays", type=int, default=3000)
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


def bounds(h, midx, xyzr):
    """per level 1 .. levels: (centres (n, 3), radii (n,), real members per node) of build_hierarchy's enclosing spheres"""
    c, r = xyzr[:, :3].astype(np.float64), np.abs(xyzr[:, 3].astype(np.float64))
    out = []
    for k in range(1, h["levels"] + 1):
        span, ctr, rad, cnt = 4 ** k, [], [], []
        for lo in range(0, h["n_hier"], span):
            hi = min(h["n_hier"], lo + span)
            ids = midx[lo:hi][h["real"][lo:hi]]
            if len(ids) == 0:
                ctr.append(np.zeros(3, np.float32)); rad.append(-1.0); cnt.append(0)
                continue
            cc, R = G._node_bound(c[ids], r[ids])
            ctr.append(cc); rad.append(R); cnt.append(len(ids))
        out.append((np.array(ctr, np.float64), np.array(rad), np.array(cnt)))
    return out


def walk_rays(levels, rays):
    """(node tests, member tests) per ray: every node of the top level is swept; a node that the ray's line meets in front of the
    origin has its four children tested, a cluster its members"""
    o, d = rays[:, :3], rays[:, 3:]

    def meets(ctr, rad):
        oc = ctr[None, :, :] - o[:, None, :]
        b = (oc * d[:, None, :]).sum(2)
        d2 = (oc * oc).sum(2) - b * b
        return (rad[None, :] >= 0) & (d2 <= rad[None, :] ** 2) & (b + np.maximum(rad[None, :], 0) >= 0)
    hit = meets(*levels[-1][:2])
    node_tests = 0
    for k in range(len(levels) - 2, -1, -1):
        ctr, rad, cnt = levels[k]
        parent = np.repeat(hit, 4, axis=1)[:, :len(rad)]
        if parent.shape[1] < len(rad):
            parent = np.pad(parent, ((0, 0), (0, len(rad) - parent.shape[1])))
        node_tests += (parent & (rad[None, :] >= 0)).sum()
        hit = parent & meets(ctr, rad)
    return node_tests / len(rays), (hit * levels[0][2][None, :]).sum() / len(rays)


rng = np.random.default_rng(1)
n = a.side
sc = np.zeros(n * n + 1, M.SPHERE_DTYPE)
gx, gz = np.meshgrid(np.arange(n) - 0.5 * (n - 1), np.arange(n) - 0.5 * (n - 1))
rad = rng.uniform(0.15, 0.25, n * n)
sc["center"][:-1] = np.stack([gx.ravel() + rng.uniform(-0.3, 0.3, n * n), rad, gz.ravel() + rng.uniform(-0.3, 0.3, n * n)], axis=1)
sc["radius"][:-1] = rad
sc["center"][-1], sc["radius"][-1] = (0.0, -1000.0, 0.0), 1000.0
sc["material_ty"] = 1
xyzr = np.concatenate([sc["center"].reshape(-1, 3), sc["radius"].reshape(-1, 1)], axis=1).astype(np.float32)
size = float(np.ptp(xyzr[:-1, :3], axis=0).max())

half = a.rays // 2
cam = np.array([0.0, 0.15 * n, 0.75 * n])
target = np.stack([rng.uniform(-0.5 * n, 0.5 * n, half), np.zeros(half), rng.uniform(-0.5 * n, 0.5 * n, half)], axis=1)
d_cam = target - cam
start = np.stack([rng.uniform(-0.5 * n, 0.5 * n, a.rays - half), np.full(a.rays - half, 1e-3), rng.uniform(-0.5 * n, 0.5 * n, a.rays - half)], axis=1)
d_b = rng.normal(size=(a.rays - half, 3))
d_b[:, 1] = np.abs(d_b[:, 1])
dirs = np.concatenate([d_cam, d_b])
rays = np.concatenate([np.concatenate([np.tile(cam, (half, 1)), start]), dirs / np.linalg.norm(dirs, axis=1, keepdims=True)], axis=1)

h0 = build(sc)
print(f"{n} x {n} jittered grid + ground: {len(sc)} spheres, {h0['n_pool']} pool clusters, {h0['levels']} levels; walk {a.walk} x {size:.1f} a step; {a.rays} rays")
print(f"{'grouping':38s} {'sum R^2, levels 1 .. ' + str(h0['levels']):40s} node tests / ray   member tests / ray")


def report(label, h, midx, pos):
    lv = bounds(h, midx, pos)
    nt, mt = walk_rays(lv, rays)
    print(f"{label:38s} {' / '.join(f'{(l[1][l[1] >= 0] ** 2).sum():.0f}' for l in lv):40s} {nt:10.1f} {mt:19.1f}", flush=True)


report("as built", h0, h0["midx"], xyzr)
pos, done = xyzr, 0
for steps in sorted(a.steps):
    for _ in range(steps - done):
        pos = pos.copy()
        pos[:-1, :3] += (rng.normal(size=(len(pos) - 1, 3)) * a.walk * size).astype(np.float32)
    done = steps
    report(f"{steps} steps, grouping kept", h0, h0["midx"], pos)
    report(f"{steps} steps, regrouped", h0, G.regroup(h0["midx"], h0["real"], h0["n_pool"], pos[:, :3]), pos)
    moved = sc.copy()
    moved["center"] = pos[:, :3]
    hb = build(moved)
    report(f"{steps} steps, mrt_set_world rebuild", hb, hb["midx"], pos)
