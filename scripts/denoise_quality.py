#!/usr/bin/env python3
"""Dev helper (GPU box): RMSE of the noisy and the denoised preview against a 256-frame render (another seed) on the cover scene
without glass, 1 spp frames, uniform accumulation (max_framebuffer_weight 1) -- the curve of profiles/denoise_quality.txt.
   python scripts/denoise_quality.py [w h] [key=value denoise parameters ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import myraytracer_amd as M
pos = [x for x in sys.argv[1:] if "=" not in x]
kw = dict(x.split("=") for x in sys.argv[1:] if "=" in x)
kw = {k: (int(v) if k in ("iterations", "normal_exp") else float(v)) for k, v in kw.items()}
w, h = (int(pos[0]), int(pos[1])) if pos else (320, 192)
sp, cam = M.scene_cover(1, False)


def rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


with M.State(M.Args(w, h, 1, 50, 1.0), seed=101) as st:
    st.set_world(sp); st.set_camera(cam)
    st.render(256)
    ref = st.read_framebuffer()
with M.State(M.Args(w, h, 1, 50, 1.0), seed=7) as st:
    st.set_world(sp); st.set_camera(cam)
    st.set_noise_tracking(True)
    if kw: st.set_denoise_params(**kw)
    print(f"cover {w}x{h} x 1 spp, params {st.denoise_params()}")
    print("frames  rmse_noisy  rmse_denoised  ratio")
    for n in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        st.render(n - st.frames_done)
        a, b = rmse(st.read_framebuffer(), ref), rmse(st.read_denoised(), ref)
        print(f"{n:6d}  {a:10.5f}  {b:13.5f}  {b / a:5.3f}", flush=True)
