#!/usr/bin/env python3
"""Dev helper (GPU box): the camera-ray sphere lists against the cluster masks over image shapes around the host's rule (frames.cpp,
kCamListMinPixelsPerLane): wall time of mrt_redraw + mrt_sync per frame, median of the frames after the tables are built, with the
lists forced (mrt_debug_set_camera_masks(2)) and with the masks forced (3), schedule (1, 1).
   python scripts/cam_list_shapes.py [scene spp frames]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import myraytracer_amd as M
a = sys.argv[1:]
scene, spp, frames = (a[0], int(a[1]), int(a[2])) if len(a) >= 3 else ("cover-glass", 64, 24)
sp, cam = M.scene_cover(1, scene == "cover-glass")
LANES = 256 * 20 * 64
for w, h in ((1200, 675), (1408, 792), (1536, 864), (1600, 900), (1760, 990), (1920, 1080)):
    ms = {}
    for mode in (2, 3, 2, 3):
        with M.State(M.Args(w, h, spp, 50, 1.0), seed=1) as st:
            st.debug_set_camera_masks(mode)
            st.set_world(sp); st.set_camera(cam); st.set_schedule_hint(1, 1)
            t = []
            for k in range(frames):
                t0 = time.perf_counter(); st.redraw(); st.sync(); t.append((time.perf_counter() - t0) * 1e3)
            ms.setdefault(mode, []).append(sorted(t[6:])[len(t[6:]) // 2])
    l, m = min(ms[2]), min(ms[3])
    print(f"{scene} {w}x{h}x{spp}: {w * h / LANES:.2f} pixels per lane; lists {ms[2][0]:.3f} / {ms[2][1]:.3f} ms, masks {ms[3][0]:.3f} / {ms[3][1]:.3f} ms; lists / masks = {l / m:.3f}", flush=True)
