#!/usr/bin/env python3
"""Dev helper (GPU box): an animated scene through mrt_set_world against mrt_update_spheres, for profiles/animation_rates.txt.
   Scenes C3 (cover-glass) and C5 (stress 100 x 100) at w x h x 1 spp.  `steps` steps of "move every sphere a little (a random
   walk, `walk` x the scene's size a step), then one frame", two ways in one process: the whole scene through mrt_set_world (the
   rebuild: the baseline) and the moved spheres through mrt_update_spheres (the refit, grouping kept).  Per way: steps per second
   (host clock around the loop and the final mrt_sync); the host time of the call; for the refit the time between HIP events
   recorded on the context's stream before and after the call (the scatter + refit kernels); how often the call returned while
   the previous frame was still unfinished (an event recorded behind that frame, queried when the call returns); and the member
   tests per world_hit call over the first and the last quarter of the run (what the kept grouping costs as the spheres drift).
   python scripts/animation_rates.py [w h] [--steps 200] [--walk 0.0005] [--depth 50]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import myraytracer_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="*", type=int, default=[1920, 1080])
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--walk", type=float, default=0.0005)
ap.add_argument("--depth", type=int, default=50)
a = ap.parse_args()
W, H = a.size


def walk(spheres, steps, rng):
    """the scene's (n, 4) centre + radius per step: every sphere but the last (the ground) on a random walk"""
    xyzr = np.concatenate([spheres["center"].reshape(-1, 3), spheres["radius"].reshape(-1, 1)], axis=1).astype(np.float32)
    size = float(np.ptp(xyzr[:-1, :3], axis=0).max())
    out = []
    for _ in range(steps):
        xyzr = xyzr.copy()
        xyzr[:-1, :3] += (rng.normal(size=(len(xyzr) - 1, 3)) * a.walk * size).astype(np.float32)
        out.append(xyzr)
    return out


def run(name, spheres, cam, way, path):
    stream = torch.cuda.Stream()
    quarter = max(1, len(path) // 4)
    with M.State(M.Args(W, H, 1, a.depth, 1.0), seed=1, stream=stream.cuda_stream) as st:
        st.set_world(spheres)
        st.set_camera(cam)
        st.render(8)
        st.sync()
        sc = spheres.copy()
        host, pairs, early, marks = [], [], 0, []
        behind_frame = None
        st.sync()
        t0 = time.perf_counter()
        for i, xyzr in enumerate(path):
            if i in (quarter, len(path) - quarter):
                st.sync()
                marks.append(st.read_counters())
            if i == 0:
                marks.append(st.read_counters())
            if way == "update":
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                c0 = time.perf_counter()
                st.update_spheres(0, xyzr)
                host.append(time.perf_counter() - c0)
                e1.record(stream)
                pairs.append((e0, e1))
            else:
                sc["center"] = xyzr[:, :3]
                c0 = time.perf_counter()
                st.set_world(sc)
                host.append(time.perf_counter() - c0)
            if behind_frame is not None and not behind_frame.query():
                early += 1
            st.redraw()
            behind_frame = torch.cuda.Event()
            behind_frame.record(stream)
        st.sync()
        sec = time.perf_counter() - t0
        marks.append(st.read_counters())
        sch = st.get_schedule()

    def tests_per_hit(c0, c1):
        return (c1["member_tests"] - c0["member_tests"]) / max(1, c1["world_hit_calls"] - c0["world_hit_calls"])
    host = np.array(host) * 1e3
    line = (f"  {name} {way:9s} {len(path) / sec:8.1f} steps/s  call on the host: median {np.median(host):8.3f} ms, mean {host.mean():8.3f}, "
            f"max {host.max():8.3f}")
    if pairs:
        dev = np.array([p[0].elapsed_time(p[1]) for p in pairs])
        line += f"  refit on the device (events): median {np.median(dev):.4f} ms, max {dev.max():.4f}"
    line += (f"  returned before the previous frame had ended: {early} of {len(path) - 1} calls"
             f"  member tests / world_hit: first quarter {tests_per_hit(marks[0], marks[1]):.2f}, last quarter {tests_per_hit(marks[2], marks[3]):.2f}"
             f"  schedule at the end: div {sch['div']} x {sch['mult']}, settled {sch['settled']}")
    print(line, flush=True)
    return len(path) / sec


print(f"{W}x{H} x 1 spp, depth {a.depth}; {a.steps} steps of a random walk ({a.walk} x the scene's size a step), one frame a step", flush=True)
for name, (spheres, cam) in (("C3 cover-glass", M.scene_cover(1, True)), ("C5 stress 100x100", M.scene_stress(1, 100))):
    path = walk(spheres, a.steps, np.random.default_rng(1))
    print(f"{name}: {len(spheres)} spheres", flush=True)
    base = run(name, spheres, cam, "set_world", path)
    upd = run(name, spheres, cam, "update", path)
    print(f"  {name}: mrt_update_spheres / mrt_set_world = {upd / base:.2f} x the steps per second", flush=True)
