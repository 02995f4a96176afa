#!/usr/bin/env python3
"""Dev helper (GPU box): what the per-tile denoise of an adaptive accumulation costs against the uniform path of the same mode
(mrt_set_denoise_adaptive; include/myraytracer_amd.h, "Adaptive accumulations").

Cover-glass scene, 1920x1080 x 1 spp.  Context A renders `frames` uniform frames.  Context B is given A's framebuffer and S
(mrt_debug_load_accumulation) with a checkerboard of tile counts: `frames` and 2 (2 < spatial_frames 3, so that in SPATIAL_EARLY
half the tiles run the 49-tap estimate).  Both share one stream; HIP events on it around ONE mrt_present(DENOISED), guides kept,
per mode; the window holds the encode and the copy of the 8-bit image too, so the plain present of the same context is measured
the same way and subtracted.  The uniform path's kernels are the parent commit's, unchanged: that column is the parent's figure.

    python scripts/denoise_tiles_rates.py [--out profiles/denoise_tiles_rates.txt] [--steps 100] [--frames 8]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")
import numpy as np          # noqa: E402
import myraytracer_amd as M  # noqa: E402

W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_tiles_rates.txt"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    # the HIP runtime the library itself runs on (the package may have brought torch's copy in: a second one would not do)
    from myraytracer_amd import _lib
    _lib.load()
    loaded = [line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line]
    hip = C.CDLL(loaded[0] if loaded else "libamdhip64.so")
    vp = C.c_void_p
    for name, args in (("hipStreamCreate", [C.POINTER(vp)]), ("hipEventCreate", [C.POINTER(vp)]), ("hipEventRecord", [vp, vp]),
                       ("hipEventSynchronize", [vp]), ("hipEventElapsedTime", [C.POINTER(C.c_float), vp, vp])):
        getattr(hip, name).restype, getattr(hip, name).argtypes = C.c_int, args

    def ok(rc, what):
        if rc != 0:
            sys.exit(f"{what} -> {rc}")
    stream, e0, e1 = vp(), vp(), vp()
    ok(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    spheres, cam = M.scene_cover(1, True)

    def window(st, denoise):
        out = []
        for k in range(a.warmup + a.steps):
            ok(hip.hipEventRecord(e0, stream), "hipEventRecord")
            st.present("rgba8", flip=True, denoise=denoise)
            ok(hip.hipEventRecord(e1, stream), "hipEventRecord")
            ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
            if k >= a.warmup:
                out.append(ms.value)
            st.acquire_presented(newest=True, wait=True, copy=False)
            st.release_presented()
        return statistics.median(out), min(out), max(out)

    lines = [f"denoise_tiles_rates.py: cover-glass, {W}x{H} x 1 spp, depth 50, {a.frames} uniform frames; the per-tile context holds the same "
             f"framebuffer and S with a checkerboard of tile counts {a.frames} / 2 (spatial_frames 3)",
             f"HIP events around ONE mrt_present (rgba8, flipped; guides kept), median of {a.steps} after {a.warmup}, ms (min .. max); "
             "denoise = the window minus the plain present's median"]
    with M.State(M.Args(W, H, 1, 50, 1.0), seed=1, stream=stream.value) as A, M.State(M.Args(W, H, 1, 50, 1.0), seed=1, stream=stream.value) as B:
        for st in (A, B):
            st.set_world(spheres)
            st.set_camera(cam)
            st.set_noise_tracking(True)
        A.render(a.frames)
        ty, tx = (H + 7) // 8, (W + 7) // 8
        board = np.where((np.arange(ty)[:, None] + np.arange(tx)[None, :]) % 2 == 0, a.frames, 2).astype(np.uint32)
        B.set_denoise_adaptive(True)
        B.debug_load_accumulation(A.read_framebuffer(), A.read_noise(), board)
        plain = {}
        for name, st in (("uniform", A), ("per tile", B)):
            plain[name] = window(st, False)
            lines.append(f"    {name:9s} plain present                    {plain[name][0]:8.3f}   ({plain[name][1]:.3f} .. {plain[name][2]:.3f})")
        for mode in ("accumulated", "prefiltered", "spatial-early"):
            got = {}
            for name, st in (("uniform", A), ("per tile", B)):
                st.set_denoise_variance(mode, 3)
                st.read_denoised()                  # (the guides and the K table exist from here on)
                got[name] = window(st, True)
                lines.append(f"    {name:9s} denoised, {mode:13s}          {got[name][0]:8.3f}   ({got[name][1]:.3f} .. {got[name][2]:.3f})"
                             f"   denoise {got[name][0] - plain[name][0]:7.3f}")
            u, t = got["uniform"][0] - plain["uniform"][0], got["per tile"][0] - plain["per tile"][0]
            lines.append(f"    {mode}: per tile / uniform = {t / u:.3f}  (+{t - u:.3f} ms)")
    # the uniform path in its spatial phase (2 frames < spatial_frames): every pixel runs the 49-tap estimate there
    with M.State(M.Args(W, H, 1, 50, 1.0), seed=1, stream=stream.value) as E:
        E.set_world(spheres)
        E.set_camera(cam)
        E.set_noise_tracking(True)
        E.render(2)
        E.set_denoise_variance("spatial-early", 3)
        E.read_denoised()
        p0, d0 = window(E, False), window(E, True)
        lines.append(f"    uniform   at 2 frames, spatial-early (all spatial) {d0[0]:8.3f}   ({d0[1]:.3f} .. {d0[2]:.3f})   denoise {d0[0] - p0[0]:7.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
