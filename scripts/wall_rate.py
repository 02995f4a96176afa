#!/usr/bin/env python3
"""Dev helper (GPU box): pipelined wall-clock Msamples/s of one workload under the tuning switches.
   [MRT_HIER=levels,top] [MRT_BOXES=0|1] [MRT_RNG=1] [MRT_HINT=div,mult] [MRT_READ_EVERY=1] [MRT_SHARD=rank,world] [MRT_STEADY=1]
   [MRT_PRESENT_EVERY=1 (a viewer on the present pass: mrt_present after every redraw, the newest image acquired without waiting)]
   [MRT_PRESENT_FORMAT=rgba8|bgra8|rgba16f|rgba32f (the format of those presents; default bgra8)]
   [MRT_PRESENT_COPY=0|1 (the present's copy on a stream of its own / on the context's stream)]
   [MRT_PRESENT_DENOISE=1 (the presents are denoised: noise tracking on, MRT_PRESENT_DENOISED; with MRT_PRESENT_EVERY=k, every k
    frames)]
   [MRT_PRESENT_VIEW=kind[:ramp] (the presents show a diagnostic view, MRT_PRESENT_VIEW: noise_se | noise_rel | tile_frames | depth |
    normal | albedo | sphere, ramp grey | heat; noise tracking on for the noise kinds)]
   [MRT_NOISE=1 (noise tracking on, no queries)] [MRT_NOISE_EVERY=k (tracking on, mrt_noise_query every k frames, the newest
    report taken without waiting)]
   python scripts/wall_rate.py scene w h spp steps"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import myraytracer_amd as M
a = sys.argv[1:]
scene, w, h, spp, steps = a[0], int(a[1]), int(a[2]), int(a[3]), int(a[4])
sp, cam = (M.scene_cover(1, scene == "cover-glass") if scene.startswith("cover") else M.scene_stress(1, 100) if scene == "stress" else M.scene_stress(1, int(scene[6:])) if scene.startswith("stress") else (M.scene_default(), None))
shard = tuple(int(x) for x in os.environ["MRT_SHARD"].split(",")) if os.environ.get("MRT_SHARD") else None
with M.State(M.Args(w, h, spp, 50, 1.0), seed=1, shard=shard) as st:
    if os.environ.get("MRT_HIER"):
        st.debug_set_hierarchy(*[int(x) for x in os.environ["MRT_HIER"].split(",")])
    if os.environ.get("MRT_BOXES"):
        st.debug_set_boxes(os.environ["MRT_BOXES"] == "1")
    if os.environ.get('MRT_SCHED'):
        a_ = [int(x) for x in os.environ['MRT_SCHED'].split(',')]
        st.debug_set_schedule(a_[0], a_[1])
    if os.environ.get("MRT_SLOTS"):
        st.debug_set_frames_in_flight(int(os.environ["MRT_SLOTS"]))
    if os.environ.get("MRT_HINT"):              # "div,mult": pin the launch schedule
        st.set_schedule_hint(*[int(x) for x in os.environ["MRT_HINT"].split(",")])
    read_every = bool(os.environ.get("MRT_READ_EVERY"))     # a viewer: the framebuffer is read back after every redraw
    present_every = int(os.environ.get("MRT_PRESENT_EVERY", "0") or "0")      # 1: after every redraw; k: every k-th
    present_denoise = bool(os.environ.get("MRT_PRESENT_DENOISE"))
    present_format = os.environ.get("MRT_PRESENT_FORMAT") or "bgra8"
    present_view = (os.environ.get("MRT_PRESENT_VIEW") or "").split(":")
    if os.environ.get("MRT_PRESENT_COPY"):
        st.debug_set_present_copy(int(os.environ["MRT_PRESENT_COPY"]))
    acquired, ring_depth = 0, 0
    noise_every = int(os.environ.get("MRT_NOISE_EVERY", "0"))
    if noise_every or os.environ.get("MRT_NOISE") or present_denoise or present_view[0].startswith("noise"):
        st.set_noise_tracking(True)
    reports = 0
    st.set_world(sp)
    if cam is not None: st.set_camera(cam)
    if os.environ.get("MRT_RNG"): st.set_rng_mode(int(os.environ["MRT_RNG"]))
    st.set_draw_counting(False)
    if present_view[0]: st.set_view(present_view[0], *present_view[1:2])
    for _ in range(int(os.environ.get('MRT_WARMUP', max(2, int(os.environ.get('MRT_SLOTS', '2')))))): st.redraw()      # (the launch-width controller settles within ~3 x the frames in flight)
    st.sync()
    c0 = st.read_counters()
    t0 = time.perf_counter()
    stamps = []
    for k in range(steps):
        st.redraw()
        stamps.append(time.perf_counter())         # (a call returns when the oldest frame in flight has ended: the back-pressure)
        if read_every: st.read_framebuffer()
        if present_every and (k + 1) % present_every == 0:
            st.present(present_format, flip=shard is None, denoise=present_denoise, **({"view": True} if present_view[0] else {}))
            got = st.acquire_presented(newest=True, wait=False, copy=False)
            acquired += got is not None
            ring_depth = got[1]["ring_depth"] if got else ring_depth
        if noise_every and (k + 1) % noise_every == 0:
            st.noise_query()
            reports += st.noise_result(wait=False) is not None
    st.sync()
    dt = time.perf_counter() - t0
    present_note = (f"presented{' denoised' if present_denoise else ''}{' view ' + ':'.join(present_view) if present_view[0] else ''} as {present_format} every {'frame' if present_every == 1 else f'{present_every} frames'} "
                    f"({acquired} of {steps // max(present_every, 1)} acquired without waiting, ring depth {ring_depth}, copy placement {os.environ.get('MRT_PRESENT_COPY', 'default (1)')}), ")
    c1 = st.read_counters()
    util = (c1["world_hit_calls"] - c0["world_hit_calls"]) / max(1, c1["lane_slots"] - c0["lane_slots"])
    print(f"{scene} {w}x{h}x{spp} HIER={os.environ.get('MRT_HIER')} BOXES={os.environ.get('MRT_BOXES')} RNG={os.environ.get('MRT_RNG')}: "
          f"{w * h * spp * steps / dt * 1e-6 / (shard[1] if shard else 1):.0f} Msamples/s, {dt / steps * 1e3:.1f} ms/step, lane util {util:.3f}, top {c1['sweep_records']}, "
          f"{'read back every frame, ' if read_every else ''}"
          f"{present_note if present_every else ''}"
          f"{'noise tracking on, ' if os.environ.get('MRT_NOISE') and not noise_every else ''}"
          f"{f'noise query every {noise_every} frames ({reports} results ready without waiting), ' if noise_every else ''}"
          f"schedule {st.get_schedule()}", flush=True)
    if os.environ.get("MRT_STEADY") and not read_every:
        # the pipelined rate WITHOUT the run's fill and drain: calls are paced by completions, so between the return of call a and
        # the return of the last call exactly (steps - 1 - a) frames have ended, with the pipeline full at both instants
        f = st.get_schedule()["frames_in_flight"]
        a = min(2 * f, steps // 3)
        n_done, span = steps - 1 - a, stamps[-1] - stamps[a]
        print(f"    steady state (frames ending between call {a} and call {steps - 1}, {f} in flight throughout): "
              f"{w * h * spp * n_done / span * 1e-6 / (shard[1] if shard else 1):.0f} Msamples/s per GPU over {span:.1f} s", flush=True)
