"""The denoiser's variance modes on the GPU (include/myraytracer_amd.h, "Variance modes"): the prefiltering a-trous kernels and
the spatial-variance kernel bit for bit against their float32 restatement (tests/denoise_var_ref.py), the context's modes against
that restatement of the same frames, the DENOISED present, the setter's refusals and persistence, and what the modes buy on the
cover scene's first frames."""
import ctypes as C

import numpy as np
import pytest

from denoise_ref import denoise, random_case
from denoise_var_ref import MODES, denoise_var, variance_of
from present_ref import encode_host

pytestmark = pytest.mark.gpu

MRT_ERR_INVALID_ARG, MRT_ERR_STATE = 1, 7
OTHER = {"sigma_l": 2.5, "normal_exp": 3, "sigma_z": 0.4, "sigma_a": 0.25}


def _state(mrt, w, h, spheres, cam, spp=1, depth=8, seed=3, **kw):
    st = mrt.State(mrt.Args(w, h, spp, depth, 1.0), seed=seed, **kw)
    st.set_world(spheres)
    if cam is not None:
        st.set_camera(cam)
    return st


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _case(rows, width):
    """random_case (non-finite texels and zero variances included); the images too low for its fixed positions get theirs in
    row 0."""
    rng = np.random.default_rng(rows * width)
    if rows >= 3:
        return random_case(rng, rows, width)
    rgba, S, guides = random_case(rng, rows, width, nonfinite=False, zero_var=False)
    rgba[0, 2, 0] = np.nan
    rgba[0, width - 1, 1] = np.inf
    S[0, width // 2] = np.nan
    S[0, 5] = np.inf
    S[0, width // 3] = 0.0
    S[0, 1] = 0.0
    return rgba, S, guides


SHAPES = [(37, 45), (8, 32), (61, 19), (3, 5), (1, 70)]


@pytest.mark.parametrize("rows,width", SHAPES)
@pytest.mark.parametrize("params", [{}, OTHER])
@pytest.mark.parametrize("variance", [1, 2])
def test_debug_denoise_variance_is_the_reference(mrt, rows, width, params, variance):
    rgba, S, guides = _case(rows, width)
    with _state(mrt, 16, 16, mrt.scene_default(), None) as st:
        for it in range(1, 6):                         # step 16 exceeds every one of these images
            for K in (0.2, np.inf):
                p = dict(params, iterations=it)
                got = st.debug_denoise(rgba, S, K, guides, p, variance=variance)
                want = denoise_var(rgba, S, K, guides, p, variance)
                assert np.array_equal(_bits(got), _bits(want)), (it, K)


def test_variance_0_through_the_new_diagnostic_is_debug_denoise(mrt):
    from myraytracer_amd import _lib
    from myraytracer_amd.api import pack_guides
    rgba, S, guides = _case(37, 45)
    g = pack_guides(guides)
    with _state(mrt, 16, 16, mrt.scene_default(), None) as st:
        for it in (1, 2, 5):
            for K in (0.2, np.inf):
                p = _lib.MrtDenoiseParams()
                assert st._L.mrt_get_denoise_params(st._ctx, C.byref(p)) == 0
                p.iterations = it
                out = np.empty_like(rgba)
                assert st._L.mrt_debug_denoise_variance(st._ctx, rgba.ctypes.data, S.ctypes.data, K, g.ctypes.data, 45, 37,
                                                        C.byref(p), 0, out.ctypes.data) == 0
                assert np.array_equal(_bits(out), _bits(st.debug_denoise(rgba, S, K, guides, {"iterations": it}))), (it, K)
        # a variance that does not exist, and a K the accumulated estimate cannot use (the spatial one ignores it)
        args = (st._ctx, rgba.ctypes.data, S.ctypes.data)
        tail = (g.ctypes.data, 45, 37, None)
        assert st._L.mrt_debug_denoise_variance(*args, 0.2, *tail, 3, out.ctypes.data) == MRT_ERR_INVALID_ARG
        assert st._L.mrt_debug_denoise_variance(*args, -1.0, *tail, 1, out.ctypes.data) == MRT_ERR_INVALID_ARG
        assert st._L.mrt_debug_denoise_variance(*args, -1.0, *tail, 2, out.ctypes.data) == 0
        assert np.array_equal(_bits(out), _bits(denoise_var(rgba, S, 0.0, guides, None, 2)))


def _reference_of(mrt, st, mode, spatial_frames=3):
    fb = st.read_framebuffer()
    K = mrt.noise_factor(st.frames_done, st.args.max_framebuffer_weight)
    variance = variance_of(mode, st.frames_done, spatial_frames)
    return denoise_var(fb, st.read_noise(), K, st.debug_read_guides(), st.denoise_params(), variance)


def test_read_denoised_follows_the_mode_frame_by_frame(mrt):
    spheres, cam = mrt.scene_cover(1, True)
    with _state(mrt, 100, 60, spheres, cam, spp=2, depth=12) as st:
        st.set_noise_tracking(True)
        st.debug_set_frames_in_flight(4)
        assert st.denoise_variance() == ("accumulated", 3)
        seen = set()
        for n in (1, 2, 3, 4, 8):                      # the spatial phase (1, 2), the switch (3) and the prefilter alone
            st.render(n - st.frames_done)
            st.set_denoise_variance("spatial-early", 3)
            assert st.denoise_variance() == ("spatial-early", 3)
            d2 = st.read_denoised()
            assert np.array_equal(_bits(d2), _bits(_reference_of(mrt, st, 2))), n
            st.set_denoise_variance("prefiltered")
            d1 = st.read_denoised()
            assert np.array_equal(_bits(d1), _bits(_reference_of(mrt, st, 1))), n
            # from the switch on mode 2 is mode 1; before it is not
            assert np.array_equal(_bits(d1), _bits(d2)) == (n >= 3), n
            seen.add(variance_of(2, n, 3))
        assert seen == {1, 2}
        st.set_denoise_variance(0)
        fb = st.read_framebuffer()
        K = mrt.noise_factor(st.frames_done, st.args.max_framebuffer_weight)
        want = denoise(fb, st.read_noise(), K, st.debug_read_guides(), st.denoise_params())
        assert np.array_equal(_bits(st.read_denoised()), _bits(want))
        # one iteration in the spatial phase: the estimate's buffer is not the output
        st.reset()
        st.set_noise_tracking(True)
        st.set_denoise_variance(2, 64)
        st.set_denoise_params(iterations=1)
        st.render(2)
        assert np.array_equal(_bits(st.read_denoised()), _bits(_reference_of(mrt, st, 2, 64)))


def test_denoised_present_in_the_spatial_phase(mrt):
    from myraytracer_amd import _lib
    L = _lib.load()
    spheres, cam = mrt.scene_cover(1, False)
    with _state(mrt, 72, 40, spheres, cam, spp=1, depth=8) as st:
        st.set_noise_tracking(True)
        st.set_denoise_variance("spatial-early")
        st.set_present_ring(8)
        refs = []
        for _ in range(4):                             # frames 1, 2: the spatial estimate; 3, 4: the prefilter
            st.redraw()
            st.present("bgra8", flip=True, denoise=True)
            refs.append(encode_host(L, st.read_denoised(), "bgra8", flip=True))
        for k in range(4):
            img, info = st.acquire_presented(newest=False, wait=True)
            assert info["frames_done"] == k + 1 and info["flags"] & _lib.PRESENT_DENOISED
            assert np.array_equal(img, refs[k]), k
        st.set_denoise_variance("accumulated")
        assert not np.array_equal(encode_host(L, st.read_denoised(), "bgra8", flip=True), refs[3])


def test_refusals_and_persistence(mrt):
    spheres, cam = mrt.scene_cover(1, False)
    with _state(mrt, 48, 32, spheres, cam) as st:
        st.set_noise_tracking(True)
        st.set_denoise_variance("spatial-early", 5)
        for bad in ((3, 3), (1, 0), (2, 65), (0xFFFFFFFF, 3)):
            with pytest.raises(mrt.MrtError) as e:
                st.set_denoise_variance(*bad)
            assert e.value.status == MRT_ERR_INVALID_ARG
            assert st.denoise_variance() == ("spatial-early", 5)
        with pytest.raises(ValueError):
            st.set_denoise_variance("spatial")
        for ok in ((0, 1), (1, 64), (2, 1), (2, 64)):  # spatial_frames is checked in every mode
            st.set_denoise_variance(*ok)
            assert st.denoise_variance() == (MODES[ok[0]], ok[1])
        st.set_denoise_variance("spatial-early", 5)
        st.redraw()
        st.reset()                                     # as the denoise parameters, the setting outlives the accumulation,
        st.set_noise_tracking(True)
        st.set_world(spheres)                          # the scene and the camera
        st.set_camera(cam)
        assert st.denoise_variance() == ("spatial-early", 5)
        st.render(2)
        for mode in MODES:                             # an adaptive accumulation is refused in every mode
            st.set_denoise_variance(mode)
            st.read_denoised()
        st.render_tiles([1, 2])
        for mode in MODES:
            st.set_denoise_variance(mode)
            for call in (st.read_denoised, lambda: st.present("rgba8", denoise=True)):
                with pytest.raises(mrt.MrtError) as e:
                    call()
                assert e.value.status == MRT_ERR_STATE
    with _state(mrt, 48, 32, spheres, cam) as st:      # ... it outlives mrt_set_shard, and a shard is refused in every mode
        st.set_denoise_variance("prefiltered", 7)
        st.set_shard(0, 2)
        assert st.denoise_variance() == ("prefiltered", 7)
        st.set_noise_tracking(True)
        st.redraw()
        for mode in MODES:
            st.set_denoise_variance(mode)
            for call in (st.read_denoised, lambda: st.present("rgba8", flip=False, denoise=True)):
                with pytest.raises(mrt.MrtError) as e:
                    call()
                assert e.value.status == MRT_ERR_STATE


def _rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def variance_quality_curve(mrt, frames=(1, 2, 4), w=320, h=192, seed=7):
    """RMSE of the noisy image and of its denoised preview in each mode -- the same frames -- against a 256-frame render with
    another seed, cover scene without glass, 1 spp frames, uniform accumulation (the setup of profiles/denoise_quality.txt):
    [(frames, noisy, accumulated, prefiltered, spatial-early)]."""
    spheres, cam = mrt.scene_cover(1, False)
    with _state(mrt, w, h, spheres, cam, spp=1, depth=50, seed=101) as st:
        st.render(256)
        ref = st.read_framebuffer()
    out = []
    with _state(mrt, w, h, spheres, cam, spp=1, depth=50, seed=seed) as st:
        st.set_noise_tracking(True)
        for n in frames:
            st.render(n - st.frames_done)
            row = [n, _rmse(st.read_framebuffer(), ref)]
            for mode in MODES:
                st.set_denoise_variance(mode)
                row.append(_rmse(st.read_denoised(), ref))
            out.append(tuple(row))
    return out


# The ratio of the mode's RMSE to the accumulated mode's on the same frames (profiles/denoise_variance_quality.txt, seed 7; how
# that table was obtained is stated there), and the bound asserted: that ratio + 0.05 (three times the spread between seeds),
# never above 1.
MEASURED = {("prefiltered", 2): 0.649, ("prefiltered", 4): 0.768, ("spatial-early", 1): 0.884}


def test_the_modes_improve_the_first_frames(mrt):
    curve = {row[0]: dict(zip(MODES, row[2:])) for row in variance_quality_curve(mrt)}
    for (mode, n), measured in MEASURED.items():
        ratio = curve[n][mode] / curve[n]["accumulated"]
        print(f"{mode} at {n} frames: {ratio:.4f} x the accumulated mode's RMSE (measured {measured})")
    for (mode, n), measured in MEASURED.items():
        assert curve[n][mode] < curve[n]["accumulated"], (mode, n, curve[n])
        assert curve[n][mode] / curve[n]["accumulated"] <= min(1.0, measured + 0.05), (mode, n, curve[n])
