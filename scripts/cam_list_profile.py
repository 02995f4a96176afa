#!/usr/bin/env python3
"""Dev helper (GPU box): scripts/phase_profile.py's phase shares for the LAST of n frames of a setting, once per camera-table
mode (mrt_debug_set_camera_masks: 0 neither table, 1 the library's rule, 2 the sphere lists, 3 the cluster masks), with the
counters that tell wave iterations from lane slots: lane_slots counts a slot for every camera ray resolved in the lane, so with
the lists in force wave iterations = (lane slots - samples) / 64 (exact while no entry overflows).
   MRT_LIB_OVERRIDE=myraytracer_amd/lib/libmyraytracer_amd_stamps.so python scripts/cam_list_profile.py [scene w h spp frames [modes]]
A tree from before the lists knows modes 0 and 1 only.  A last argument `tail` names the phases of the tail-split build
(make stamps-tail, libmyraytracer_amd_stamps_tail.so: the walk's cycles are in the sweep's line)."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import myraytracer_amd as M
from myraytracer_amd import _lib
a = sys.argv[1:]
TAIL = bool(a) and a[-1] == "tail"
if TAIL: a.pop()
scene = a[0] if a else "cover-glass"
w, h, spp, frames = (int(x) for x in a[1:5]) if len(a) >= 5 else (1920, 1080, 512, 1)
modes = [int(x) for x in a[5].split(",")] if len(a) > 5 else [1, 0]
sp, cam = M.scene_cover(1, scene == "cover-glass")
NAMES = ["tail", "sweep", "node rounds", "root rounds", "no-scatter", "release/refill/acquire", "unpack"]
if TAIL:
    NAMES = ["tail: scatter + normalize", "sweep + walk", "tail: primary hit", "tail: shading", "no-scatter", "release/refill/acquire", "tail: rejection loop"]


def counters(st):
    raw = (C.c_uint64 * 16)()
    _lib.load().mrt_debug_read_counters(st._ctx, raw)
    return list(raw)


for mode in modes:
    with M.State(M.Args(w, h, spp, 50, 1.0), seed=1) as st:
        st._check(st._L.mrt_debug_set_camera_masks(st._ctx, mode), "mrt_debug_set_camera_masks")
        st.set_world(sp); st.set_camera(cam); st.set_schedule_hint(1, 1)
        for _ in range(frames - 1): st.redraw()
        st.sync(); before = counters(st)
        st.redraw(); st.sync()
        raw = [y - x for x, y in zip(before, counters(st))]
        info = st.debug_read_camera_masks(table=False)
        table = "lists" if info.get("lists") else "masks" if info["in_force"] else "none"
        iters = (raw[3] - (raw[0] if table == "lists" else 0)) / 64
        ph = [raw[6 + k] for k in range(6)] + [raw[5]]
        print(f"-- {scene} {w}x{h}x{spp}, frame {frames}, mode {mode}: table {table}; kernel ms {st.last_kernel_ms():.3f}, wave iterations {iters:.0f}, "
              f"samples {raw[0]}, world_hit calls {raw[1]}, lane slots {raw[3]}, member tests {raw[4]}; iteration slots per sample {64 * iters / raw[0]:.3f}")
        print("   cycles per wave iteration: " + "; ".join(f"{n} {v / iters:.0f}" for n, v in zip(NAMES, ph)) + f"; all {sum(ph) / iters:.0f}.  All phases {sum(ph):.4g} cycles; "
              f"node rounds per iteration {raw[12] / iters:.2f} ({raw[14] / max(1, raw[12]):.1f} items), root rounds {raw[13] / iters:.2f} ({raw[15] / max(1, raw[13]):.1f} items)")
