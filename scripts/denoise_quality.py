#!/usr/bin/env python3
"""Dev helper (GPU box): RMSE of the noisy and the denoised preview against a 256-frame render (another seed) on the cover scene
without glass, 1 spp frames, uniform accumulation (max_framebuffer_weight 1) -- the curve of profiles/denoise_quality.txt.
   python scripts/denoise_quality.py [w h] [key=value denoise parameters ...]
   python scripts/denoise_quality.py --variance [--out FILE] [w h] [key=value ...]: the three variance modes
   (mrt_set_denoise_variance) on the same frames, seeds 7 and 8 -- the table of profiles/denoise_variance_quality.txt, written
   to FILE (default: that file's table part on stdout only)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import myraytracer_amd as M
argv = sys.argv[1:]
variance = "--variance" in argv
out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
argv = [x for i, x in enumerate(argv) if x not in ("--variance", "--out") and (i == 0 or argv[i - 1] != "--out")]
pos = [x for x in argv if "=" not in x]
kw = dict(x.split("=") for x in argv if "=" in x)
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

def variance_curves():
    """Every mode on the same frames: the RMSE ratio denoised / noisy per mode, and each mode's against the accumulated one."""
    modes = ("accumulated", "prefiltered", "spatial-early")
    lines = []
    for seed in (7, 8):
        with M.State(M.Args(w, h, 1, 50, 1.0), seed=seed) as st:
            st.set_world(sp); st.set_camera(cam)
            st.set_noise_tracking(True)
            if kw: st.set_denoise_params(**kw)
            lines.append(f"cover {w}x{h} x 1 spp, seed {seed}, spatial_frames 3, params {st.denoise_params()}")
            lines.append("frames  rmse_noisy  " + "  ".join(f"{m:>13s}" for m in modes) + "   ratio to noisy: acc   pre   spa   ratio to accumulated: pre   spa")
            for n in (1, 2, 3, 4, 8, 16, 32, 64, 128, 256):
                st.render(n - st.frames_done)
                a = rmse(st.read_framebuffer(), ref)
                d = []
                for m in modes:
                    st.set_denoise_variance(m, 3)
                    d.append(rmse(st.read_denoised(), ref))
                lines.append(f"{n:6d}  {a:10.5f}  " + "  ".join(f"{x:13.5f}" for x in d) + "                   " +
                             " ".join(f"{x / a:5.3f}" for x in d) + "                         " + " ".join(f"{x / d[0]:5.3f}" for x in d[1:]))
                print(lines[-1], flush=True)
    return lines


if variance:
    text = "\n".join(variance_curves()) + "\n"
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    sys.exit(0)
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
