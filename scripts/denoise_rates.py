#!/usr/bin/env python3
"""Dev helper (GPU box): the denoiser's passes, for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...).
   Per rep: mrt_set_camera (the guides go stale) and a DENOISED present (the guide rebuild, the filter's iterations and the
   encode, queued on the context's stream), then, with MRT_GUIDES_ONCE=1, reps more presents on the same guides.
   Then, per variance mode (mrt_set_denoise_variance; "spatial-early" with spatial_frames 64, so that the 4 frames done are in
   its spatial phase), reps more presents on the same guides: each mode's filter next to the accumulated mode's in the same run,
   first with the blend with the accumulation off (the filter as it always was), then with it on (mrt_set_denoise_mix: the last
   iteration runs as a non-last one and mix_kernel follows it).
   python scripts/denoise_rates.py scene w h reps [iterations]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import myraytracer_amd as M
a = sys.argv[1:]
scene, w, h, reps = a[0], int(a[1]), int(a[2]), int(a[3])
iters = int(a[4]) if len(a) > 4 else 5
sp, cam = (M.scene_cover(1, scene == "cover-glass") if scene.startswith("cover") else M.scene_stress(1, 100) if scene == "stress"
           else (M.scene_default(), None))
with M.State(M.Args(w, h, 1, 50, 1.0), seed=1) as st:
    st.set_world(sp)
    if cam is not None: st.set_camera(cam)
    st.set_noise_tracking(True)
    st.set_denoise_params(iterations=iters)
    st.render(4)
    st.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        if cam is not None: st.set_camera(cam)                # stale guides: the rebuild is queued with the present
        st.present("bgra8", denoise=True)
        st.acquire_presented(newest=True, wait=False, copy=False)
    st.sync()
    t1 = time.perf_counter()
    for _ in range(reps):
        st.present("bgra8", denoise=True)
        st.acquire_presented(newest=True, wait=False, copy=False)
    st.sync()
    t2 = time.perf_counter()
    print(f"{scene} {w}x{h}, {iters} iterations: {(t1 - t0) / reps * 1e3:.3f} ms per present with a guide rebuild, "
          f"{(t2 - t1) / reps * 1e3:.3f} ms per denoised present (wall, host-paced)", flush=True)
    for mode in ("accumulated", "prefiltered", "spatial-early"):
        st.set_denoise_variance(mode, 64)
        ms = []
        for mix in (False, True):
            st.set_denoise_mix(mix)
            st.present("bgra8", denoise=True)
            st.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                st.present("bgra8", denoise=True)
                st.acquire_presented(newest=True, wait=False, copy=False)
            st.sync()
            ms.append((time.perf_counter() - t0) / reps * 1e3)
        st.set_denoise_mix(False)
        print(f"    variance {mode}: {ms[0]:.3f} ms per denoised present, {ms[1]:.3f} ms with the blend (wall, host-paced)", flush=True)
