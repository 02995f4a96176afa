#!/usr/bin/env python3
"""Dev helper (GPU box): the four forms of the noise report's reduction (noise.hip), one query per frame, for a kernel trace:
     rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o prof -- python scripts/noise_reduce_rates.py [w h n]
   cover-glass at w x h (1920 x 1080) x 1 spp with noise tracking on.  n (40) times each, a whole frame and then one query:
   uniform K with a max-rel map, uniform K with a summed-S map; then every third tile two frames ahead (the accumulation has
   diverged: K per tile) and the same two maps.  The trace names the kernel of every form.  MRT_LIB_OVERRIDE selects another
   build of the library (the parent's, for profiles/noise_reduce_refactor.txt).
   python scripts/noise_reduce_rates.py --stats <dir> ...: the trace's average us per noise kernel of each <dir>, as a table."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(dirs):
    rows = {}
    for d in dirs:
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                if "noise_" in r["Name"]:
                    name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("mrt::", "")
                    rows.setdefault(name, {})[d] = f"{float(r['AverageNs']) / 1e3:7.2f} ({r['Calls']})"
    print(f"{'average us (calls)':42s}" + "".join(f"{os.path.basename(d.rstrip('/')):>16s}" for d in dirs))
    for name in sorted(rows):
        print(f"{name:42s}" + "".join(f"{rows[name].get(d, '-'):>16s}" for d in dirs))


if len(sys.argv) > 1 and sys.argv[1] == "--stats":
    stats(sys.argv[2:])
    sys.exit(0)

sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import myraytracer_amd as M  # noqa: E402

w, h, n = (int(x) for x in (sys.argv[1:4] + ["1920", "1080", "40"][len(sys.argv) - 1:]))
spheres, cam = M.scene_cover(1, True)
with M.State(M.Args(w, h, 1, 50, 1.0), seed=1) as st:
    st.set_world(spheres)
    st.set_camera(cam)
    st.set_noise_tracking(True)
    st.render(8)                                           # warm: buffers, tile costs, the schedule
    for diverged in (False, True):
        if diverged:
            st.sync()
            st.render_tiles(np.arange(0, st.tile_frames().size, 3, dtype=np.uint32), 2)
        for kind in ("max_rel", "sum_s"):
            for _ in range(n):
                st.redraw()
                st.noise_query(0.1, 0.05, tile_map=kind)
            rep = st.noise_result(wait=True)
            print(f"{'per-tile' if diverged else 'uniform'} K, {kind}: {n} queries, the last: seq {rep['seq']}, frames_done "
                  f"{rep['frames_done']}, above {rep['above']}, rel_rmse {rep['rel_rmse']:.6g}", flush=True)
    st.sync()
