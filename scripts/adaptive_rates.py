#!/usr/bin/env python3
"""Dev helper (GPU box): uniform against adaptive rendering to the same stop, for profiles/adaptive_rates.txt.
   Per samples-per-frame setting: the cover-glass scene at w x h; every run checks the noise report every `every` frames with
   the report lagged one check (render_until's loop) and stops at the first report with above == 0 at rel threshold `thr`
   (floor `fl`), or at `cap` frames.  Runs: uniform; adaptive (render_until(adaptive=True): the subset frames of a chunk in one
   in-lane launch); adaptive without frame batching (mrt_debug_set_frame_batching(0): a launch per frame, the uniform chunks'
   included); and uniform at the adaptive run's counted samples.  Each records frames, counted
   samples (mrt_read_counters), wall time (host clock around the loop and the final mrt_sync) and the RMSE of the final image
   against a long uniform accumulation of `ref` frames.
   python scripts/adaptive_rates.py [w h] [--spp 1,8] [--thr 0.1] [--floor 0.05] [--every 8] [--cap 1024,256] [--ref 2048,512]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import myraytracer_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="*", type=int, default=[1920, 1080])
ap.add_argument("--spp", default="1,8")
ap.add_argument("--thr", type=float, default=0.1)
ap.add_argument("--floor", type=float, default=0.05)
ap.add_argument("--every", type=int, default=8)
ap.add_argument("--cap", default="1024,256")
ap.add_argument("--ref", default="2048,512")
ap.add_argument("--depth", type=int, default=50)
a = ap.parse_args()
W, H = a.size
SPHERES, CAM = M.scene_cover(1, True)


def state(spp):
    st = M.State(M.Args(W, H, spp, a.depth, 1.0), seed=1)
    st.set_world(SPHERES)
    st.set_camera(CAM)
    return st


def warm(st):
    st.render(4)
    st.sync()
    st.reset()


def uniform_until(st, cap):
    st.set_noise_tracking(True)
    st.render(min(a.every, cap))
    st.noise_query(a.thr, a.floor)
    while True:
        n = min(a.every, cap - st.frames_done)
        if n > 0:
            st.render(n)
        rep = st.noise_result(wait=True)
        if rep["above"] == 0 or rep["frames_done"] >= cap:
            return rep
        st.noise_query(a.thr, a.floor)


def rmse(x, ref):
    d = x[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


for spp, cap, nref in zip([int(s) for s in a.spp.split(",")], [int(s) for s in a.cap.split(",")], [int(s) for s in a.ref.split(",")]):
    with state(spp) as st:
        warm(st)
        st.render(nref)
        st.sync()
        ref = st.read_framebuffer()
    print(f"cover-glass {W}x{H} x {spp} spp, depth {a.depth}: stop at above == 0 (rel threshold {a.thr}, floor {a.floor}), "
          f"checked every {a.every} frames, capped at {cap} frames; reference: {nref} uniform frames", flush=True)
    results = {}
    for name in ("uniform", "adaptive", "adaptive, no batching", "uniform, adaptive's samples"):
        with state(spp) as st:
            warm(st)
            if name == "adaptive, no batching":
                st.debug_set_frame_batching(0)
            st.sync()
            t0 = time.perf_counter()
            if name == "uniform":
                rep = uniform_until(st, cap)
            elif name.startswith("adaptive"):
                _, rep = st.render_until(0.0, cap, check_every=a.every, threshold=a.thr, floor=a.floor, adaptive=True)
            else:
                frames = max(1, round(results["adaptive"]["samples"] / (W * H * spp)))
                st.render(frames)
                rep = None
            st.sync()
            sec = time.perf_counter() - t0
            samples = st.read_counters()["samples"]
            tf = st.tile_frames()
            r = {"frames": st.frames_done, "samples": samples, "sec": sec, "rmse": rmse(st.read_framebuffer(), ref),
                 "above": rep["above"] if rep else None, "tile_frames": (int(tf.min()), int(tf.max()))}
            results[name] = r
            print(f"  {name:28s} frames {r['frames']:5d}  samples {samples / 1e6:10.1f} M  wall {sec * 1e3:9.1f} ms  "
                  f"{samples / sec * 1e-6:8.0f} Msamples/s  rmse {r['rmse']:.5f}  above at stop {r['above']}  "
                  f"tile frames {r['tile_frames'][0]}..{r['tile_frames'][1]}", flush=True)
    u, ad = results["uniform"], results["adaptive"]
    print(f"  adaptive / uniform: samples {ad['samples'] / u['samples']:.3f}, wall {ad['sec'] / u['sec']:.3f}", flush=True)
