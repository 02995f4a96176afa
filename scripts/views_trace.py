#!/usr/bin/env python3
"""Dev helper (GPU box): every diagnostic view (views.hip) presented as rgba32f at one size, for a kernel trace -- a uniform
accumulation first, then NOISE_SE / NOISE_REL / TILE_FRAMES once more on a diverged one (K and n_t per tile):
   rocprofv3 --kernel-trace --stats -d DIR -- python scripts/views_trace.py [w h [repeats]]
The stats name view_kernel<kind, per tile> per instantiation, next to present_float_kernel<0> of the same presents."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import myraytracer_amd as M
a = sys.argv[1:]
w, h = (int(a[0]), int(a[1])) if len(a) >= 2 else (1920, 1080)
repeats = int(a[2]) if len(a) >= 3 else 20
KINDS = ("noise_se", "noise_rel", "tile_frames", "depth", "normal", "albedo", "sphere")
sp, cam = M.scene_cover(1, True)
with M.State(M.Args(w, h, 1, 50, 1.0), seed=1) as st:
    st.set_noise_tracking(True)
    st.set_world(sp)
    st.set_camera(cam)
    st.render(4)
    for diverged in (False, True):
        if diverged:
            st.render_tiles(np.arange(((w + 7) // 8) * ((h + 7) // 8))[::2], 1)
        for kind in KINDS[:3] if diverged else KINDS:
            st.set_view(kind, "heat", 0.0, 0.1 if kind.startswith("noise") else 8.0)
            for _ in range(repeats):
                st.present("rgba32f", view=True)
                assert st.acquire_presented(newest=False, wait=True, copy=False) is not None
            print(f"{kind}{' per tile' if diverged else ''}: {repeats} presents of {w}x{h}", flush=True)
