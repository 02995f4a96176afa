#!/usr/bin/env python3
"""Dev helper (GPU box): image RMSE at equal samples -- uniform rendering, render_adaptive and render_budget -- for
   profiles/adaptive_budget_quality.txt and profiles/adaptive_budget_rates.txt.
   The cover-glass scene at w x h, 1 spp; the reference is a long uniform accumulation of `ref` frames (as
   scripts/adaptive_rates.py takes it).  Runs, each from a fresh context and timed on the host clock around the loop and the final
   sync:
     uniform           `frames` whole frames
     adaptive          render_until(adaptive=True) to above == 0 at rel threshold `thr`, floor `fl`, checked every `every` frames
                       (profiles/adaptive_rates.txt's run: its samples are what `frames` uniform frames count)
     budget M          2 x `every` uniform frames, then chunks of render_budget(chunk, M, the report one check before the newest)
                       with noise_query(tile_map="sum_s") after every chunk, until (frames - 2 x every) x tiles tile-frames are
                       spent: the samples of `frames` uniform frames.  chunk = `chunk_frames` x tiles.
     uniform, wall     whole frames for as long as the slowest budget run took (frames scaled by the measured rate)
   and the cost of the call: the host time of mrt_render_budget per chunk (allocation, read-back of the map and the queueing),
   of mrt_budget_allocate alone on the last map, and the chunk's wall time.
   --trace: a short run for rocprofv3 --kernel-trace --stats: queries of both kinds on a uniform and on a diverged accumulation.
   --plan device (profiles/budget_plan_rates.txt): beside every "budget M" run, the same loop with the allocation on the device
     budget M, device          noise_query(budget=chunk, max_frames=M) after every chunk and render_planned(the report one check
                               before the newest): the same one-check lag, under the target rule -- frames queued since a plan's
                               query count towards it, so a chunk may queue less than its plan and the run takes more chunks
     budget M, host / device, lag 0   the chunk renders the plan of the query just queued (it waits for that query: nothing
                               overlaps, nothing is discounted)
   and the host time per chunk of the query plus mrt_render_planned against mrt_render_budget's.
   --trace --plan device: for rocprofv3 --kernel-trace --stats, per max_frames of its own: 20 noise_query(budget=chunk) on a
     diverged accumulation (the budget_* kernels are the allocation), and mrt_budget_allocate's host time on the same map and n_t.
   python scripts/adaptive_budget_quality.py [w h] [--frames 66] [--ref 2048] [--every 8] [--max-frames 4,8,16] [--chunk-frames 2]
                                             [--plan host|device]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import myraytracer_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="*", type=int, default=[1920, 1080])
ap.add_argument("--frames", type=int, default=66)
ap.add_argument("--ref", type=int, default=2048)
ap.add_argument("--every", type=int, default=8)
ap.add_argument("--thr", type=float, default=0.1)
ap.add_argument("--floor", type=float, default=0.05)
ap.add_argument("--cap", type=int, default=1024)
ap.add_argument("--max-frames", default="4,8,16")
ap.add_argument("--chunk-frames", type=int, default=2)
ap.add_argument("--depth", type=int, default=50)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--plan", choices=("host", "device"), default="host")
a = ap.parse_args()
W, H = a.size
SPHERES, CAM = M.scene_cover(1, True)


def state():
    st = M.State(M.Args(W, H, 1, a.depth, 1.0), seed=1)
    st.set_world(SPHERES)
    st.set_camera(CAM)
    st.render(4)                                           # warm: buffers, tile costs, the schedule
    st.sync()
    st.reset()
    return st


def rmse(x, ref):
    d = x[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def budget_run(st, max_frames, total, chunk, log):
    """the lagged loop of render_until(budget=...), stopped by the tile-frames spent instead of by a report"""
    st.set_noise_tracking(True)
    st.render(a.every)
    st.noise_query(a.thr, a.floor, tile_map="sum_s")
    st.render(a.every)
    earlier = st.noise_result(wait=True)
    st.noise_query(a.thr, a.floor, tile_map="sum_s")
    spent = 0
    while spent < total:
        t0 = time.perf_counter()
        res = st.render_budget(min(chunk, total - spent), max_frames, earlier["seq"])
        t1 = time.perf_counter()
        earlier = st.noise_result(wait=True)               # the newest queued: the check before this chunk
        st.noise_query(a.thr, a.floor, tile_map="sum_s")
        log.append((t1 - t0, time.perf_counter() - t0, res))
        if res["tile_frames"] == 0:
            break
        spent += res["tile_frames"]
    return spent


def planned_run(st, max_frames, total, chunk, log, device, lag):
    """budget_run with the allocation on the device (device) or without the lag (lag 0: the chunk renders from the query just
    queued); log: (host time of the query and the render call, the chunk's wall time, the result)"""
    budgets = {}                                           # a device plan's budget is fixed at its query: what was left then

    def query():
        left = max(1, min(chunk, total - spent))
        if device:
            st.noise_query(a.thr, a.floor, budget=left, max_frames=max_frames)
        else:
            st.noise_query(a.thr, a.floor, tile_map="sum_s")
            budgets[len(budgets) + 1] = left

    def render(seq):
        return st.render_planned(seq) if device else st.render_budget(budgets[seq], max_frames, seq)
    spent = idle = 0
    st.set_noise_tracking(True)
    st.render(a.every)
    query()
    st.render(a.every)
    earlier = st.noise_result(wait=True)
    t0 = time.perf_counter()
    query()
    while spent < total and idle < 2:
        if lag == 0:
            res = render(st.noise_result(wait=True)["seq"])
            t1 = time.perf_counter()
        else:
            res = render(earlier["seq"])
            t1 = time.perf_counter()
            earlier = st.noise_result(wait=True)
        log.append((t1 - t0, time.perf_counter() - t0, res))
        t0 = time.perf_counter()
        query()
        idle = idle + 1 if res["tile_frames"] == 0 else 0   # (a plan met by the chunk before it queues nothing: not the end)
        spent += res["tile_frames"]
    return spent


if a.trace and a.plan == "device":
    mf = int(a.max_frames.split(",")[0])
    with state() as st:
        st.set_noise_tracking(True)
        st.render(16)
        n_tiles = st.tile_frames().size
        st.noise_query(a.thr, a.floor, budget=a.chunk_frames * n_tiles, max_frames=mf)
        st.render_planned(st.noise_result(wait=True)["seq"])          # diverged, as a run's accumulation is
        st.sync()
        for _ in range(20):
            st.noise_query(a.thr, a.floor, budget=a.chunk_frames * n_tiles, max_frames=mf)
        seq = st.noise_result(wait=True)["seq"]
        plan = st.budget_plan(seq)
        s_map, n_t = st.read_noise_tiles(), st.tile_frames()
        ts = []
        for _ in range(9):
            t0 = time.perf_counter()
            k, res = M.State.budget_allocate(s_map, n_t, 1.0, a.chunk_frames * n_tiles, mf)
            ts.append(time.perf_counter() - t0)
        assert np.array_equal(k, plan["k"]) and res["tile_frames"] == plan["tile_frames"]
        print(f"trace run done: {n_tiles} tiles, max_frames {mf}, budget {a.chunk_frames * n_tiles}: the plan gives {plan['tile_frames']} "
              f"tile-frames to {plan['tiles']} tiles, equal to mrt_budget_allocate's, which took a median {np.median(ts) * 1e3:.2f} ms "
              f"(min {min(ts) * 1e3:.2f}) on the same map and n_t", flush=True)
    sys.exit(0)

if a.trace:
    with state() as st:
        st.set_noise_tracking(True)
        st.render(16)
        for _ in range(20):
            st.noise_query(a.thr, a.floor)
            st.noise_query(a.thr, a.floor, tile_map="sum_s")
        st.sync()
        st.render_tiles(np.arange(0, st.tile_frames().size, 3, dtype=np.uint32), 2)
        for _ in range(20):
            st.noise_query(a.thr, a.floor)
            st.noise_query(a.thr, a.floor, tile_map="sum_s")
        st.sync()
    print("trace run done", flush=True)
    sys.exit(0)

with state() as st:
    st.render(a.ref)
    st.sync()
    ref = st.read_framebuffer()
    n_tiles = st.tile_frames().size
print(f"cover-glass {W}x{H} x 1 spp, depth {a.depth}, {n_tiles} tiles; reference: {a.ref} uniform frames; equal samples: those of "
      f"{a.frames} uniform frames", flush=True)


def line(name, st, sec, extra=""):
    samples = st.read_counters()["samples"]
    tf = st.tile_frames()
    r = rmse(st.read_framebuffer(), ref)
    print(f"  {name:26s} frames {st.frames_done:5d}  samples {samples / 1e6:8.1f} M  wall {sec * 1e3:8.1f} ms  rmse {r:.5f}  "
          f"tile frames {int(tf.min())}..{int(tf.max())}{extra}", flush=True)
    return r, sec, samples


results = {}
with state() as st:
    st.set_noise_tracking(True)                            # (as every other run: the blends keep S)
    st.sync()
    t0 = time.perf_counter()
    st.render(a.frames)
    st.sync()
    results["uniform"] = line("uniform", st, time.perf_counter() - t0)
with state() as st:
    st.sync()
    t0 = time.perf_counter()
    st.render_until(0.0, a.cap, check_every=a.every, threshold=a.thr, floor=a.floor, adaptive=True)
    st.sync()
    results["adaptive"] = line("adaptive", st, time.perf_counter() - t0)
total = (a.frames - 2 * a.every) * n_tiles
chunk = a.chunk_frames * n_tiles
logs = {}
for mf in [int(s) for s in a.max_frames.split(",")]:
    with state() as st:
        st.sync()
        log = logs[mf] = []
        t0 = time.perf_counter()
        budget_run(st, mf, total, chunk, log)
        st.sync()
        sec = time.perf_counter() - t0
        results[f"budget {mf}"] = line(f"budget, max_frames {mf}", st, sec, f"  chunks {len(log)}")
        last_map, last_n = st.read_noise_tiles(), st.tile_frames()
    for name, device, lag in (("device", True, 1), ("host, lag 0", False, 0), ("device, lag 0", True, 0)) if a.plan == "device" else ():
        with state() as st:
            st.sync()
            log = logs[(mf, name)] = []
            t0 = time.perf_counter()
            planned_run(st, mf, total, chunk, log, device, lag)
            st.sync()
            sec = time.perf_counter() - t0
            results[f"budget {mf}, {name}"] = line(f"budget {mf}, {name}", st, sec, f"  chunks {len(log)}")
slowest = max(v[1] for k, v in results.items() if k.startswith("budget"))
frames_wall = max(1, round(a.frames * slowest / results["uniform"][1]))
with state() as st:
    st.set_noise_tracking(True)
    st.sync()
    t0 = time.perf_counter()
    st.render(frames_wall)
    st.sync()
    results["uniform, wall"] = line("uniform, budget's wall", st, time.perf_counter() - t0)
u = results["uniform"][0]
print("  rmse against uniform's at equal samples: " + ", ".join(f"{k} {v[0] / u:.3f}" for k, v in results.items() if k != "uniform"), flush=True)
uw = results["uniform, wall"][0]
print("  rmse against uniform's at equal wall time (the slowest budget run's): " +
      ", ".join(f"{k} {v[0] / uw:.3f}" for k, v in results.items() if k.startswith("budget")), flush=True)

print(f"cost of the call, {n_tiles} tiles, chunk = {a.chunk_frames} x tiles tile-frames:")
for mf, log in logs.items():
    call = np.array([c for c, _, r in log if r["tile_frames"]]) * 1e3
    whole = np.array([w for _, w, r in log if r["tile_frames"]]) * 1e3
    lv = [r["frames"] for _, _, r in log if r["tile_frames"]]
    if isinstance(mf, tuple):
        what = "query + mrt_render_planned" if mf[1].startswith("device") else "query + mrt_render_budget"
        print(f"  max_frames {mf[0]:2d}, {mf[1]}: {what} host time per chunk median {np.median(call):.2f} ms (min {call.min():.2f}, max "
              f"{call.max():.2f}); chunk to its report median {np.median(whole):.2f} ms; frames per chunk {min(lv)}..{max(lv)}; "
              f"chunks that queued nothing {sum(1 for _, _, r in log if not r['tile_frames'])}", flush=True)
        continue
    print(f"  max_frames {mf:2d}: mrt_render_budget host time per chunk median {np.median(call):.2f} ms (min {call.min():.2f}, max {call.max():.2f}); "
          f"chunk to its report median {np.median(whole):.2f} ms; frames per chunk {min(lv)}..{max(lv)}", flush=True)
for mf in [int(s) for s in a.max_frames.split(",")]:
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        M.State.budget_allocate(last_map, last_n, 1.0, chunk, mf)
        ts.append(time.perf_counter() - t0)
    print(f"  mrt_budget_allocate alone (the last run's map and n_t, budget {chunk}), max_frames {mf:2d}: median {np.median(ts) * 1e3:.2f} ms", flush=True)
