#!/usr/bin/env python3
"""Dev helper (GPU box): an animated scene through mrt_set_world against mrt_update_spheres, for profiles/animation_rates.txt.
   Scenes C3 (cover-glass) and C5 (stress 100 x 100) at w x h x 1 spp.  `steps` steps of "move every sphere a little (a random
   walk, `walk` x the scene's size a step), then one frame", two ways in one process: the whole scene through mrt_set_world (the
   rebuild: the baseline) and the moved spheres through mrt_update_spheres (the refit, grouping kept).  Per way: steps per second
   (host clock around the loop and the final mrt_sync); the host time of the call; for the refit the time between HIP events
   recorded on the context's stream before and after the call (the scatter + refit kernels); how often the call returned while
   the previous frame was still unfinished (an event recorded behind that frame, queried when the call returns); and the member
   tests per world_hit call over the first and the last quarter of the run (what the kept grouping costs as the spheres drift).
   python scripts/animation_rates.py [w h] [--steps 200] [--walk 0.0005] [--depth 50]
   --regroup-every N prints the section "regroup" instead (mrt_regroup_spheres): (1) the cost of one regroup at C3
   and C5 -- host time of the call, device time between HIP events on the context's stream around it -- next to the same
   process's mrt_set_world call; (2) the animated C5 three ways in one process -- the refit alone, a regroup every N steps, a
   rebuild (mrt_set_world) every N steps -- with the member tests per world_hit by quarter; (3) the static C5 and C3 as built and
   after one regroup with no motion: the render kernel's time (mrt_kernel_ms_history) and member tests per world_hit.
   --temporal prints the section "temporal" instead (mrt_temporal_step): the animated C3 and C5 through
   mrt_update_spheres at max_framebuffer_weight 0, one frame a step, two ways in one process -- the frame and a present of the
   framebuffer; the frame, mrt_temporal_step and a present of the temporal image -- with the steps per second and the time between
   HIP events on the context's stream around the step (guide rebuild + reprojection + snapshot) and around the temporal present
   (variance + a-trous iterations + encode).
   --response (with or without --temporal) prints that section with a third way, the temporal response on (mrt_set_temporal_response,
   DESIGN.md 7h: the reprojection with the fast history, then the clamp), and the ways alternate over `--rounds` rounds in the one
   process: the response's cost is its step's device time against the response-off step's of the same round, and the difference
   between the rounds is the spread to read it against.
   --auto-regroup prints the section "auto-regroup" instead (mrt_set_auto_regroup): the animated C5 with the library
   deciding when to regroup.  With --ratio and / or --check-every: a regroup every N steps (--regroup-every, default 50) against
   the policy with those numbers, one run each, with the policy's statistics at the end.  With neither, the measurement the
   defaults come from, in one process: (1) the cost of a check that does not fire -- the policy at ratio 1e6, check_every 1
   against the policy off, as step time and as the device time of the update call between HIP events -- and from it the
   smallest power-of-two check_every that keeps the cost under 1 % of the every-N step; (2) ratios 1.5, 2, 3, 4 at that
   check_every, of which the largest within --spread steps/s of the fastest is taken; (3) the slow walk (0.2 x --walk) every N against the policy; (4) the C3 walk with the policy off and on.
   --materials prints the section "materials" instead (mrt_update_materials): (1) the call for 1 sphere and for all
   10,001 of C5 -- host time, device time between HIP events on the context's stream around it -- next to the same context's
   mrt_set_world; (2) on C3 and C5, `steps` steps of "recolour every sphere, then one frame" four ways, twice in turn in one
   process: no edit at all (the ceiling), the edit through mrt_update_materials, the same with the schedule pinned to full-width
   frames (mrt_set_schedule_hint(1, 1)), the edit through mrt_set_world."""
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
ap.add_argument("--regroup-every", type=int, default=0)
ap.add_argument("--temporal", action="store_true")
ap.add_argument("--response", action="store_true")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--auto-regroup", action="store_true")
ap.add_argument("--materials", action="store_true")
ap.add_argument("--ratio", type=float, default=None)
ap.add_argument("--check-every", type=int, default=None)
ap.add_argument("--spread", type=float, default=0.0, help="steps/s within which two ratios tie (the larger is taken)")
a = ap.parse_args()
W, H = a.size


def walk(spheres, steps, rng, amount=None):
    """the scene's (n, 4) centre + radius per step: every sphere but the last (the ground) on a random walk"""
    xyzr = np.concatenate([spheres["center"].reshape(-1, 3), spheres["radius"].reshape(-1, 1)], axis=1).astype(np.float32)
    size = float(np.ptp(xyzr[:-1, :3], axis=0).max())
    amount = a.walk if amount is None else amount
    out = []
    for _ in range(steps):
        xyzr = xyzr.copy()
        xyzr[:-1, :3] += (rng.normal(size=(len(xyzr) - 1, 3)) * amount * size).astype(np.float32)
        out.append(xyzr)
    return out


def run(name, spheres, cam, way, path, every=0, auto=None):
    """way: set_world | update | regroup (update, and mrt_regroup_spheres every `every` steps) | rebuild (update, but mrt_set_world
    every `every` steps) | auto (update with mrt_set_auto_regroup(**auto) on); with `every` the member tests are reported for each
    quarter of the run.  run.last: the update call's median device time and the policy's statistics of the run"""
    stream = torch.cuda.Stream()
    quarter = max(1, len(path) // 4)
    bounds = (quarter, 2 * quarter, 3 * quarter) if every else (quarter, len(path) - quarter)
    with M.State(M.Args(W, H, 1, a.depth, 1.0), seed=1, stream=stream.cuda_stream) as st:
        st.set_world(spheres)
        st.set_camera(cam)
        st.render(8)
        st.sync()
        if way == "auto":
            st.set_auto_regroup(True, **auto)
        sc = spheres.copy()
        host, pairs, early, marks = [], [], 0, []
        behind_frame = None
        st.sync()
        t0 = time.perf_counter()
        for i, xyzr in enumerate(path):
            if i in bounds:
                st.sync()
                marks.append(st.read_counters())
            if i == 0:
                marks.append(st.read_counters())
            if way != "set_world" and not (way == "rebuild" and i and i % every == 0):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                c0 = time.perf_counter()
                st.update_spheres(0, xyzr)
                host.append(time.perf_counter() - c0)
                e1.record(stream)
                pairs.append((e0, e1))
                if way == "regroup" and i and i % every == 0:
                    st.regroup_spheres()
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
        stats = st.read_regroup_stats() if way == "auto" else None

    def tests_per_hit(c0, c1):
        return (c1["member_tests"] - c0["member_tests"]) / max(1, c1["world_hit_calls"] - c0["world_hit_calls"])
    host = np.array(host) * 1e3
    label = way if way != "auto" else f"auto r{auto['ratio']:g}/{auto['check_every']}"
    run.last = dict(dev=None, stats=stats)
    line = (f"  {name} {label:9s} {len(path) / sec:8.1f} steps/s  call on the host: median {np.median(host):8.3f} ms, mean {host.mean():8.3f}, "
            f"max {host.max():8.3f}")
    if pairs:
        dev = np.array([p[0].elapsed_time(p[1]) for p in pairs])
        run.last["dev"] = float(np.median(dev))
        line += f"  refit on the device (events): median {np.median(dev):.4f} ms, max {dev.max():.4f}"
    line += f"  returned before the previous frame had ended: {early} of {len(path) - 1} calls"
    if every:
        line += "  member tests / world_hit by quarter: " + ", ".join(f"{tests_per_hit(marks[q], marks[q + 1]):.2f}" for q in range(4))
    else:
        line += f"  member tests / world_hit: first quarter {tests_per_hit(marks[0], marks[1]):.2f}, last quarter {tests_per_hit(marks[2], marks[3]):.2f}"
    line += (f"  schedule at the end: div {sch['div']} x {sch['mult']}, settled {sch['settled']}")
    if stats:
        line += (f"  policy: {stats['checks']} checks, {stats['regroups']} regroups, Q_ref {stats['q_ref']:.6g}, Q last {stats['q_last']:.6g}"
                 f" (by level {', '.join(f'{v:.6g}' for v in stats['q_level'])})")
    print(line, flush=True)
    return len(path) / sec


def regroup_cost(name, spheres, cam, path):
    """(1): one regroup of the scene moved to the end of the walk, against the same context's mrt_set_world of it"""
    stream = torch.cuda.Stream()
    with M.State(M.Args(W, H, 1, a.depth, 1.0), seed=1, stream=stream.cuda_stream) as st:
        st.set_world(spheres)
        st.set_camera(cam)
        st.render(4)
        st.update_spheres(0, path[-1])
        st.sync()
        host, dev = [], []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            c0 = time.perf_counter()
            st.regroup_spheres()
            host.append((time.perf_counter() - c0) * 1e3)
            e1.record(stream)
            st.sync()
            dev.append(e0.elapsed_time(e1))
        info = st.debug_regroup_info()
        sc = spheres.copy()
        sc["center"] = path[-1][:, :3]
        built = []
        for _ in range(5):
            c0 = time.perf_counter()
            st.set_world(sc)
            built.append((time.perf_counter() - c0) * 1e3)
    print(f"  {name}: mrt_regroup_spheres ({info['n_pool']} pool clusters, {info['global_depths']} depths over global memory, {info['lds_depths']} in LDS): "
          f"host median {np.median(host):.3f} ms, max {max(host):.3f}; device (events) median {np.median(dev):.4f} ms, max {max(dev):.4f};  "
          f"mrt_set_world of the same spheres: host median {np.median(built):.3f} ms;  regroup host + device = "
          f"{(np.median(host) + np.median(dev)) / np.median(built):.4f} x the rebuild's host time", flush=True)


def static_cost(name, spheres, cam):
    """(3): the scene as built and after one regroup with no motion, 64 frames each, twice in turn in one context (as built,
    regrouped, built again, regrouped again), so that a drift of the machine shows as a difference between the rounds"""
    out = []
    with M.State(M.Args(W, H, 1, a.depth, 1.0), seed=1) as st:
        st.set_camera(cam)
        for rnd in range(2):
            for regroup in (False, True):
                if regroup:
                    st.regroup_spheres()
                else:
                    st.set_world(spheres)
                st.reset()
                for _ in range(16):
                    st.redraw()
                st.sync()
                c0 = st.read_counters()
                for _ in range(64):
                    st.redraw()
                st.sync()
                c1 = st.read_counters()
                ms = np.array(st.kernel_ms_history(64))
                out.append((np.median(ms), ms.min(), (c1["member_tests"] - c0["member_tests"]) / max(1, c1["world_hit_calls"] - c0["world_hit_calls"])))
                print(f"  {name} static, round {rnd + 1}, {'regrouped' if regroup else 'as built '}: render kernel median {out[-1][0]:.4f} ms, min {out[-1][1]:.4f} "
                      f"(64 frames); member tests / world_hit {out[-1][2]:.2f}; sweep variant {st.debug_sweep_variant()}, "
                      f"sweep axes {st.debug_read_hierarchy()['axes']}", flush=True)
    for rnd in range(2):
        b, r = out[2 * rnd], out[2 * rnd + 1]
        print(f"  {name} static, round {rnd + 1}: regrouped / as built = {r[0] / b[0]:.4f} x the kernel's median time ({r[1] / b[1]:.4f} x its minimum), "
              f"{r[2] / b[2]:.4f} x the member tests", flush=True)


def temporal_cost(name, spheres, cam, path, response=False, rounds=1):
    ways = (False, True, "response") if response else (False, True)
    label = {False: "frame + present               ", True: "frame + step + temporal present", "response": "the same with the response on  "}
    step_med = {w: [] for w in ways}
    for rnd in range(rounds):
        rates = {}
        for way in ways:
            temporal = way is not False
            stream = torch.cuda.Stream()
            with M.State(M.Args(W, H, 1, a.depth, 0.0), seed=1, stream=stream.cuda_stream) as st:
                st.set_world(spheres)
                st.set_camera(cam)
                st.set_temporal(temporal)
                if way == "response":
                    st.set_temporal_response(True)
                st.set_present_ring(4)
                for _ in range(8):                      # (the schedule's trials, the first step's allocations and the ring)
                    st.redraw()
                    if temporal:
                        st.temporal_step()
                    st.present("rgba8", temporal=temporal)
                st.sync()
                steps, presents = [], []
                t0 = time.perf_counter()
                for xyzr in path:
                    st.update_spheres(0, xyzr)
                    st.redraw()
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                    ev[0].record(stream)
                    if temporal:
                        st.temporal_step()
                    ev[1].record(stream)
                    ev[2].record(stream)
                    st.present("rgba8", temporal=temporal)
                    ev[3].record(stream)
                    steps.append(ev[:2])
                    presents.append(ev[2:])
                st.sync()
                sec = time.perf_counter() - t0
            rates[way] = len(path) / sec
            step_ms = np.array([e0.elapsed_time(e1) for e0, e1 in steps])
            pres_ms = np.array([e0.elapsed_time(e1) for e0, e1 in presents])
            step_med[way].append(float(np.median(step_ms)))
            q1, q3 = np.percentile(step_ms, [25, 75])
            print(f"  {name} {label[way]} {rates[way]:8.1f} steps/s"
                  + (f"  mrt_temporal_step on the device (events): median {np.median(step_ms):.4f} ms, quartiles {q1:.4f} .. {q3:.4f}, max {step_ms.max():.4f};" if temporal else "")
                  + f"  present (kernels + copy, events): median {np.median(pres_ms):.4f} ms, max {pres_ms.max():.4f}"
                  + (f"  (round {rnd + 1})" if rounds > 1 else ""), flush=True)
        print(f"  {name}: with the temporal step and present / without = {rates[True] / rates[False]:.3f} x the steps per second"
              + (f"; with the response on {rates['response'] / rates[False]:.3f} x" if response else ""), flush=True)
    if response:
        on, off = np.array(step_med["response"]), np.array(step_med[True])
        print(f"  {name}: the response's cost, step on - step off by round: " + ", ".join(f"{d:+.4f} ms" for d in on - off)
              + f" ({', '.join(f'{r:.3f}' for r in on / off)} x the step); the step's median between the rounds: off "
              + " / ".join(f"{v:.4f}" for v in off) + ", on " + " / ".join(f"{v:.4f}" for v in on), flush=True)


def recolours(spheres, steps, rng):
    """per step, every sphere's material with a new albedo (and a new fuzz for the metals): a MATERIAL_DTYPE array of the scene"""
    out = []
    for _ in range(steps):
        m = M.materials_of(spheres)
        m["albedo"] = rng.uniform(0.05, 0.95, (len(m), 3)).astype(np.float32)
        m["param"] = np.where(m["material_ty"] == 2, rng.uniform(0.0, 0.5, len(m)), m["param"]).astype(np.float32)
        out.append(m)
    return out


def materials_cost(name, spheres, cam):
    """(1): the call for 1 sphere and for all of them -- host time, device time between HIP events on the context's stream around
    it, the context idle -- next to the same context's mrt_set_world of the same list"""
    stream = torch.cuda.Stream()
    edits = recolours(spheres, 50, np.random.default_rng(2))
    with M.State(M.Args(W, H, 1, a.depth, 1.0), seed=1, stream=stream.cuda_stream) as st:
        st.set_world(spheres)
        st.set_camera(cam)
        st.render(4)
        st.sync()
        for count in (1, len(spheres)):
            host, dev = [], []
            for m in edits:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                c0 = time.perf_counter()
                st.update_materials(0, m[:count])
                host.append((time.perf_counter() - c0) * 1e3)
                e1.record(stream)
                st.sync()
                dev.append(e0.elapsed_time(e1))
            print(f"  {name}: mrt_update_materials of {count} sphere{'s' if count > 1 else ''} ({-(-count // 192)} launch{'es' if count > 192 else ''}): "
                  f"host median {np.median(host):.4f} ms, max {max(host):.4f}; device (events) median {np.median(dev):.4f} ms, max {max(dev):.4f}", flush=True)
        built = []
        for _ in range(5):
            c0 = time.perf_counter()
            st.set_world(spheres)
            built.append((time.perf_counter() - c0) * 1e3)
        print(f"  {name}: mrt_set_world of the same {len(spheres)} spheres: host median {np.median(built):.3f} ms", flush=True)


def materials_loop(name, spheres, cam, way, edits):
    """(2): `way` = none | materials | mat-wide (materials with mrt_set_schedule_hint(1, 1)) | set_world: per step the edit (or
    nothing), then one frame; steps per second over the loop and the final mrt_sync"""
    stream = torch.cuda.Stream()
    with M.State(M.Args(W, H, 1, a.depth, 1.0), seed=1, stream=stream.cuda_stream) as st:
        st.set_world(spheres)
        st.set_camera(cam)
        if way == "mat-wide":                   # every frame on all the waves: an edit between two frames keeps them from overlapping anyway
            st.set_schedule_hint(1, 1)
        st.render(8)
        st.sync()
        sc = spheres.copy()
        host = []
        t0 = time.perf_counter()
        for m in edits:
            c0 = time.perf_counter()
            if way in ("materials", "mat-wide"):
                st.update_materials(0, m)
            elif way == "set_world":
                for k in M.MATERIAL_DTYPE.names:
                    sc[k] = m[k]
                st.set_world(sc)
            host.append((time.perf_counter() - c0) * 1e3)
            st.redraw()
        st.sync()
        sec = time.perf_counter() - t0
        sch = st.get_schedule()
    print(f"  {name} {way:9s} {len(edits) / sec:8.1f} steps/s ({1e3 * sec / len(edits):.3f} ms a step)  call on the host: median {np.median(host):8.4f} ms, "
          f"max {max(host):8.4f}  schedule at the end: div {sch['div']} x {sch['mult']}, settled {sch['settled']}, {sch['frames_in_flight']} frames in flight", flush=True)
    return len(edits) / sec


if a.materials:
    print(f"materials: {W}x{H} x 1 spp, depth {a.depth}; {a.steps} steps of \"recolour every sphere, then one frame\"; build {M._lib.load().mrt_build_id().decode()}",
          flush=True)
    scenes = (("C3 cover-glass", M.scene_cover(1, True)), ("C5 stress 100x100", M.scene_stress(1, 100)))
    print("(1) the call alone, 50 calls each, the context idle", flush=True)
    materials_cost(*scenes[1][:1], *scenes[1][1])
    print("(2) the loop four ways, twice in turn in one process", flush=True)
    for name, (spheres, cam) in scenes:
        edits = recolours(spheres, a.steps, np.random.default_rng(1))
        print(f"{name}: {len(spheres)} spheres", flush=True)
        for rnd in range(2):
            r = {way: materials_loop(name, spheres, cam, way, edits) for way in ("none", "materials", "mat-wide", "set_world")}
            print(f"  {name}, round {rnd + 1}: mrt_update_materials {r['materials'] / r['none']:.3f} x the no-edit loop ({1e3 / r['materials'] - 1e3 / r['none']:+.4f} ms a step), "
                  f"with the schedule pinned to full-width frames {r['mat-wide'] / r['none']:.3f} x ({1e3 / r['mat-wide'] - 1e3 / r['none']:+.4f} ms a step), "
                  f"mrt_set_world {r['set_world'] / r['none']:.3f} x ({1e3 / r['set_world'] - 1e3 / r['none']:+.4f} ms a step)", flush=True)
    sys.exit(0)

if a.temporal or a.response:
    print(f"temporal{' + response' if a.response else ''}: {W}x{H} x 1 spp, depth {a.depth}, max_framebuffer_weight 0; {a.steps} steps of a random walk ({a.walk} x the scene's size a "
          f"step), one frame a step; build {M._lib.load().mrt_build_id().decode()}", flush=True)
    for name, (spheres, cam) in (("C3 cover-glass", M.scene_cover(1, True)), ("C5 stress 100x100", M.scene_stress(1, 100))):
        temporal_cost(name, spheres, cam, walk(spheres, a.steps, np.random.default_rng(1)), a.response, a.rounds if a.response else 1)
    sys.exit(0)

if a.auto_regroup:
    N = a.regroup_every or 50
    scenes = (("C3 cover-glass", M.scene_cover(1, True)), ("C5 stress 100x100", M.scene_stress(1, 100)))
    name, (spheres, cam) = scenes[1]
    path = walk(spheres, a.steps, np.random.default_rng(1))
    d = M._lib.MrtAutoRegroup()
    M._lib.load().mrt_auto_regroup_default(d)
    print(f"auto-regroup: {W}x{H} x 1 spp, depth {a.depth}; {a.steps} steps of the walk of {a.walk} x the scene's size a step, one frame a step; "
          f"library defaults ratio {d.ratio:g}, check_every {d.check_every}; build {M._lib.load().mrt_build_id().decode()}", flush=True)
    if a.ratio is not None or a.check_every is not None:
        cfg = dict(ratio=d.ratio if a.ratio is None else a.ratio, check_every=d.check_every if a.check_every is None else a.check_every)
        run(name, spheres, cam, "regroup", path, every=N)
        run(name, spheres, cam, "auto", path, every=N, auto=cfg)
        sys.exit(0)
    print(f"(1) {name}: a regroup every {N} steps; the policy off; the policy at ratio 1e6, check_every 1 (every update checks, none fires)", flush=True)
    every_n = run(name, spheres, cam, "regroup", path, every=N)
    off = run(name, spheres, cam, "update", path, every=N)
    off_dev = run.last["dev"]
    on = run(name, spheres, cam, "auto", path, every=N, auto=dict(ratio=1e6, check_every=1))
    on_dev = run.last["dev"]
    cost_step, cost_dev, budget = (1.0 / on - 1.0 / off) * 1e3, on_dev - off_dev, 0.01 * 1e3 / every_n
    cost = max(cost_step, cost_dev, 0.0)
    k = 1
    while cost / k >= budget and k < 1024:
        k *= 2
    print(f"  a check that does not fire costs {cost_step:+.4f} ms of step time ({1e3 / off:.3f} -> {1e3 / on:.3f} ms a step), {cost_dev:+.4f} ms of the update's "
          f"device time (median {off_dev:.4f} -> {on_dev:.4f} ms); 1 % of the every-{N} step ({1e3 / every_n:.3f} ms) is {budget:.4f} ms: "
          f"the larger of the two costs, {cost:.4f} ms, stays under it from check_every {k}", flush=True)
    print(f"(2) {name}: ratios at check_every {k}", flush=True)
    rates = {r: run(name, spheres, cam, "auto", path, every=N, auto=dict(ratio=r, check_every=k)) for r in (1.5, 2.0, 3.0, 4.0)}
    print("  steps/s by ratio: " + ", ".join(f"{r:g}: {v:.1f}" for r, v in rates.items()) + f"; every {N}: {every_n:.1f}", flush=True)
    best = max(r for r in rates if rates[r] >= max(rates.values()) - a.spread)
    print(f"  the largest ratio within {a.spread:.1f} steps/s of the fastest: {best:g}", flush=True)
    slow = walk(spheres, a.steps, np.random.default_rng(1), 0.2 * a.walk)
    print(f"(3) {name}: the slow walk ({0.2 * a.walk:g} x the scene's size a step): every {N} against the policy at ratio {best:g}, check_every {k}", flush=True)
    run(name, spheres, cam, "regroup", slow, every=N)
    run(name, spheres, cam, "auto", slow, every=N, auto=dict(ratio=best, check_every=k))
    name, (spheres, cam) = scenes[0]
    path = walk(spheres, a.steps, np.random.default_rng(1))
    print(f"(4) {name} (a single block kernel): the policy off and on (ratio {best:g}, check_every {k})", flush=True)
    run(name, spheres, cam, "update", path, every=N)
    run(name, spheres, cam, "auto", path, every=N, auto=dict(ratio=best, check_every=k))
    sys.exit(0)

if a.regroup_every:
    N = a.regroup_every
    print(f"regroup: {W}x{H} x 1 spp, depth {a.depth}; the walk of {a.walk} x the scene's size a step; build {M._lib.load().mrt_build_id().decode()}", flush=True)
    scenes = (("C3 cover-glass", M.scene_cover(1, True)), ("C5 stress 100x100", M.scene_stress(1, 100)))
    paths = {name: walk(spheres, a.steps, np.random.default_rng(1)) for name, (spheres, cam) in scenes}
    print(f"(1) one regroup of the scene after {a.steps} steps, 20 calls", flush=True)
    for name, (spheres, cam) in scenes:
        regroup_cost(name, spheres, cam, paths[name])
    name, (spheres, cam) = scenes[1]
    print(f"(2) {name}, {a.steps} steps, one frame a step: the refit alone, a regroup every {N} steps, a rebuild every {N} steps", flush=True)
    for way in ("update", "regroup", "rebuild"):
        run(name, spheres, cam, way, paths[name], every=N)
    print("(3) no motion: as built against one regroup", flush=True)
    for name, (spheres, cam) in scenes[::-1]:
        static_cost(name, spheres, cam)
    sys.exit(0)

print(f"{W}x{H} x 1 spp, depth {a.depth}; {a.steps} steps of a random walk ({a.walk} x the scene's size a step), one frame a step", flush=True)
for name, (spheres, cam) in (("C3 cover-glass", M.scene_cover(1, True)), ("C5 stress 100x100", M.scene_stress(1, 100))):
    path = walk(spheres, a.steps, np.random.default_rng(1))
    print(f"{name}: {len(spheres)} spheres", flush=True)
    base = run(name, spheres, cam, "set_world", path)
    upd = run(name, spheres, cam, "update", path)
    print(f"  {name}: mrt_update_spheres / mrt_set_world = {upd / base:.2f} x the steps per second", flush=True)
