"""The denoiser's blend with the accumulation on the GPU (include/myraytracer_amd.h, "Blend with the accumulation";
mrt_set_denoise_mix): the blend kernel behind every form of the filter bit for bit against its float32 restatement
(tests/denoise_mix_ref.py) -- through mrt_debug_denoise_mix on synthetic frames and through the product on the context's own
framebuffer, S, K and guides --, the DENOISED present, frames in flight, the per-tile filter, the gathered frame, the setting's
contract, what stays as it was (the setting off, the temporal image, every refusal) and what the blend buys on the cover scene.
Every comparison is on uint32 views."""
import numpy as np
import pytest

from denoise_mix_ref import QUALITY, denoise_mix, denoise_mix_tiles, rmse
from denoise_ref import denoise, random_case
from denoise_tiles_ref import library_k, tile_map
from denoise_var_ref import MODES, denoise_var, variance_of
from present_ref import encode_host

pytestmark = pytest.mark.gpu

MRT_ERR_INVALID_ARG, MRT_ERR_NO_SCENE, MRT_ERR_STATE = 1, 4, 7
W, H = 64, 40


def _state(mrt, w=W, h=H, seed=3, tracking=True, depth=8, **kw):
    st = mrt.State(mrt.Args(w, h, 1, depth, 1.0), seed=seed, **kw)
    spheres, cam = mrt.scene_cover(1, False)
    st.set_world(spheres)
    st.set_camera(cam)
    if tracking:
        st.set_noise_tracking(True)
    return st


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _refused(mrt, call, status=MRT_ERR_STATE):
    with pytest.raises(mrt.MrtError) as e:
        call()
    assert e.value.status == status


def _case(rows, width):
    """random_case (NaN / Inf texels and zero variances included); the images too small for its fixed positions get what fits."""
    rng = np.random.default_rng(rows * width)
    if rows >= 3 and width >= 3:
        return random_case(rng, rows, width)
    rgba, S, guides = random_case(rng, rows, width, nonfinite=False, zero_var=False)
    if width >= 3:
        rgba[0, 0, 0] = np.nan
        S[rows - 1, 1] = 0.0
        S[0, 2] = np.inf
    return rgba, S, guides


# W x H: smaller than the window in both axes; smaller in one; ragged against the 32 x 8 tile with 2 x 2 and 3 x 3 workgroups
@pytest.mark.parametrize("width,rows", [(1, 1), (3, 2), (33, 9), (70, 19)])
@pytest.mark.parametrize("variance", [0, 1, 2])
def test_debug_denoise_mix_is_the_reference(mrt, width, rows, variance):
    rgba, S, guides = _case(rows, width)
    default = mrt.denoise_mix_default()["gain"]
    with _state(mrt, 16, 16) as st:
        for it in (1, 2, 5):                            # both parities of the ping / pong buffer the blend reads, and 1
            for K in (0.2, np.inf):
                for gain in (0.25, default, 16.0):
                    got = st.debug_denoise_mix(rgba, S, K, guides, {"iterations": it}, variance, gain=gain)
                    want = denoise_mix(rgba, S, K, guides, {"iterations": it}, variance, gain)
                    assert np.array_equal(_bits(got), _bits(want)), (it, K, gain)
                # the blend off through the same entry point: mrt_debug_denoise_variance
                off = st.debug_denoise_mix(rgba, S, K, guides, {"iterations": it}, variance, enabled=False)
                assert np.array_equal(_bits(off), _bits(denoise_var(rgba, S, K, guides, {"iterations": it}, variance))), (it, K)
        if width >= 33:                                 # the two definitions broken on purpose are not what the device computes
            got = st.debug_denoise_mix(rgba, S, 0.2, guides, {"iterations": 5}, variance, gain=2.0)
            assert np.array_equal(_bits(got), _bits(denoise_mix(rgba, S, 0.2, guides, {"iterations": 5}, variance, 2.0)))
            for broken in ("v_plus_u", "dx_then_dy"):
                assert not np.array_equal(_bits(got), _bits(denoise_mix(rgba, S, 0.2, guides, {"iterations": 5}, variance, 2.0, broken)))
            for bad in (0.2, 17.0, float("nan")):
                _refused(mrt, lambda: st.debug_denoise_mix(rgba, S, 0.2, guides, None, variance, gain=bad), MRT_ERR_INVALID_ARG)


def _reference_of(mrt, st, gain=None):
    mode, spatial = st.denoise_variance()
    K = mrt.noise_factor(st.frames_done, st.args.max_framebuffer_weight)
    gain = st.denoise_mix()[1] if gain is None else gain
    return denoise_mix(st.read_framebuffer(), st.read_noise(), K, st.debug_read_guides(), st.denoise_params(),
                       variance_of(MODES.index(mode), st.frames_done, spatial), gain)


def test_the_product_is_the_reference_of_its_own_frame(mrt):
    from myraytracer_amd import _lib
    L = _lib.load()
    with _state(mrt) as st:
        assert st.denoise_mix() == (False, mrt.denoise_mix_default()["gain"])
        st.set_denoise_mix(True)
        for n in (1, 4, 20):                            # 1: K = +inf, the filter's image
            st.render(n - st.frames_done)
            for mode in MODES:
                st.set_denoise_variance(mode, 6)         # (4 frames: SPATIAL_EARLY is still in its spatial phase, with a finite K)
                for it, gain in ((5, None), (2, 3.0)):
                    st.set_denoise_params(**dict(mrt.denoise_params_default(), iterations=it))
                    st.set_denoise_mix(True, gain)
                    got = st.read_denoised()
                    assert np.array_equal(_bits(got), _bits(_reference_of(mrt, st))), (n, mode, it)
                    st.present("rgba8", flip=True, denoise=True)
                    img, info = st.acquire_presented(newest=True, wait=True)
                    assert info["flags"] & _lib.PRESENT_DENOISED
                    assert np.array_equal(img, encode_host(L, got, "rgba8", flip=True)), (n, mode, it)
                st.set_denoise_mix(True, mrt.denoise_mix_default()["gain"])
        # it did something, and the accumulation is left alone
        fb, S = st.read_framebuffer(), st.read_noise()
        on = st.read_denoised()
        st.set_denoise_mix(False)
        assert not np.array_equal(_bits(on), _bits(st.read_denoised()))
        assert np.array_equal(_bits(st.read_framebuffer()), _bits(fb)) and np.array_equal(_bits(st.read_noise()), _bits(S))
        assert st.debug_check_context() is None


def test_sixteen_frames_in_flight_match_the_synchronised_calls(mrt):
    from myraytracer_amd import _lib
    L = _lib.load()
    out = []
    for synchronised in (False, True):
        with _state(mrt) as st:
            st.set_denoise_mix(True)
            st.set_present_ring(18)
            for _ in range(16):
                st.redraw()
                st.present("rgba8", flip=False, denoise=True)
                if synchronised:
                    st.sync()
            imgs = [st.acquire_presented(newest=False, wait=True)[0].copy() for _ in range(16)]
            out.append((imgs, st.read_denoised()))
            if synchronised:
                assert np.array_equal(imgs[-1], encode_host(L, out[-1][1], "rgba8"))
                assert np.array_equal(_bits(out[-1][1]), _bits(_reference_of(mrt, st)))
    assert all(np.array_equal(a, b) for a, b in zip(out[0][0], out[1][0]))
    assert np.array_equal(_bits(out[0][1]), _bits(out[1][1]))


def test_the_per_tile_filter_is_blended_per_pixel(mrt):
    w, h = 45, 37                                       # 6 x 5 tiles, ragged in both axes
    rng = np.random.default_rng(w * h)
    rgba, S, _ = random_case(rng, h, w)
    counts = [0, 1, 2, 3, 4, 40]                        # tiles without an estimate (0 and 1 frames) next to tiles with many
    tiles = tile_map(rng, h, w, counts)
    assert set(counts) <= set(int(v) for v in tiles.ravel())
    k_of = library_k(1.0)
    with _state(mrt, w, h) as st:
        st.set_denoise_adaptive(True)
        st.debug_load_accumulation(rgba, S, tiles)
        guides = st.debug_read_guides()
        for mode in range(3):
            st.set_denoise_variance(mode, 4)
            for it, gain in ((1, 0.5), (5, None)):
                st.set_denoise_params(**dict(mrt.denoise_params_default(), iterations=it))
                st.set_denoise_mix(True, gain)
                got = st.read_denoised()
                want = denoise_mix_tiles(rgba, S, tiles, guides, st.denoise_params(), mode, 4, k_of, st.denoise_mix()[1])
                assert np.array_equal(_bits(got), _bits(want)), (mode, it)
        # a uniform map is the uniform path's blend
        st.debug_load_accumulation(tile_frames=np.full(tiles.shape, 9, np.uint32))
        st.set_denoise_variance(0, 4)
        want = denoise_mix(rgba, S, k_of(9), guides, st.denoise_params(), 0, st.denoise_mix()[1])
        assert np.array_equal(_bits(st.read_denoised()), _bits(want))


def test_a_gather_of_two_contexts_is_the_unsharded_blend(mrt):
    from myraytracer_amd import _lib
    L = _lib.load()
    ref = _state(mrt)
    shards = [_state(mrt, shard=(r, 2)) for r in range(2)]
    try:
        shards[0].set_gather_noise(True)
        for st in [ref] + shards:
            st.set_denoise_mix(True, 1.5)
        for n in (4, 20):
            for st in [ref] + shards:
                st.render(n - st.frames_done)
            mrt.gather(shards, 0)
            shards[0].render(3)                          # the gather's snapshot of K, whatever the root renders afterwards
            for mode in MODES:
                ref.set_denoise_variance(mode, 6)
                shards[0].set_denoise_variance(mode, 6)
                want, got = ref.read_denoised(), shards[0].read_gathered_denoised()
                assert np.array_equal(_bits(got), _bits(want)), (n, mode)
                assert np.array_equal(_bits(want), _bits(_reference_of(mrt, ref))), (n, mode)
            shards[0].present("rgba8", flip=True, gathered_denoised=True)
            img, _ = shards[0].acquire_presented(newest=True, wait=True)
            assert np.array_equal(img, encode_host(L, want, "rgba8", flip=True))
            shards[1].render(3)
        for call in (shards[1].read_denoised, lambda: shards[0].present("rgba8", flip=False, denoise=True)):
            _refused(mrt, call)                          # a shard's own denoise stays refused
    finally:
        for st in [ref] + shards:
            st.close()


def test_the_settings_contract(mrt):
    default = mrt.denoise_mix_default()["gain"]
    with _state(mrt) as st:
        st.render(4)
        off = st.read_denoised()
        assert np.array_equal(_bits(off), _bits(denoise(st.read_framebuffer(), st.read_noise(), mrt.noise_factor(4, 1.0),
                                                         st.debug_read_guides(), st.denoise_params())))
        for bad in ({"gain": 0.2}, {"gain": 16.5}, {"gain": float("nan")}, {"gain": float("inf")}):
            _refused(mrt, lambda: st.set_denoise_mix(True, **bad), MRT_ERR_INVALID_ARG)
        assert st.denoise_mix() == (False, default)      # nothing changed
        st.set_denoise_mix(True, 4.0)
        assert st.denoise_mix() == (True, 4.0)
        on = st.read_denoised()
        assert not np.array_equal(_bits(on), _bits(off))
        st.set_denoise_mix(False)                        # gain None: kept
        assert st.denoise_mix() == (False, 4.0)
        for mode in MODES:                               # on, then off: every image is what it was
            st.set_denoise_variance(mode, 3)
            K = mrt.noise_factor(4, 1.0)
            want = denoise_var(st.read_framebuffer(), st.read_noise(), K, st.debug_read_guides(), st.denoise_params(),
                               variance_of(MODES.index(mode), 4, 3))
            assert np.array_equal(_bits(st.read_denoised()), _bits(want)), mode
        st.set_denoise_variance("accumulated", 3)
        assert np.array_equal(_bits(st.read_denoised()), _bits(off))
        # the setting outlives the accumulation, the scene, the camera and the shard
        st.set_denoise_mix(True, 4.0)
        st.reset()
        assert st.denoise_mix() == (True, 4.0)
        st.set_noise_tracking(True)
        st.set_world(mrt.scene_default())
        spheres, cam = mrt.scene_cover(1, False)
        st.set_world(spheres)
        st.set_camera(cam)
        assert st.denoise_mix() == (True, 4.0)
        st.render(4)
        assert np.array_equal(_bits(st.read_denoised()), _bits(_reference_of(mrt, st)))
        st.reset()
        st.set_shard(0, 2)
        assert st.denoise_mix() == (True, 4.0)


def test_the_temporal_image_is_unchanged(mrt):
    out = []
    for mix in (False, True):
        with mrt.State(mrt.Args(W, H, 1, 8, 0.0), seed=3) as st:
            spheres, cam = mrt.scene_cover(1, False)
            st.set_world(spheres)
            st.set_camera(cam)
            st.set_noise_tracking(True)
            st.set_temporal(True)
            st.set_denoise_mix(mix, 2.0)
            for _ in range(3):
                st.redraw()
                st.temporal_step()
            st.present("rgba8", flip=False, temporal=True)
            img, _ = st.acquire_presented(newest=True, wait=True)
            out.append((st.read_temporal(), img.copy()))
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(out[0][1], out[1][1])


def test_every_refusal_is_unchanged(mrt):
    with _state(mrt, tracking=False) as st:
        st.set_denoise_mix(True)
        st.redraw()
        for call in (st.read_denoised, lambda: st.present("rgba8", denoise=True)):
            _refused(mrt, call)                          # noise tracking off
        st.reset()
        st.set_noise_tracking(True)
        st.redraw()
        _refused(mrt, lambda: st.present("rgba8", gathered=True, denoise=True), MRT_ERR_INVALID_ARG)
        _refused(mrt, lambda: st.present("rgba8", temporal=True, denoise=True), MRT_ERR_INVALID_ARG)
        _refused(mrt, st.read_temporal)                  # temporal reprojection off
        _refused(mrt, st.read_gathered_denoised)         # no gather
        st.render_tiles([1, 2, 7])                       # diverged without mrt_set_denoise_adaptive
        for call in (st.read_denoised, lambda: st.present("rgba8", denoise=True)):
            _refused(mrt, call)
        st.set_denoise_adaptive(True)
        st.read_denoised()
    with _state(mrt, shard=(0, 2)) as st:
        st.set_denoise_mix(True)
        st.redraw()
        for call in (st.read_denoised, lambda: st.present("rgba8", flip=False, denoise=True), st.debug_read_guides):
            _refused(mrt, call)
    with mrt.State(mrt.Args(W, H, 1, 8, 1.0), seed=3) as st:
        st.set_noise_tracking(True)
        st.set_denoise_mix(True)
        _refused(mrt, st.read_denoised, MRT_ERR_NO_SCENE)


# The host test's quality assertion on the device, at the same size: below both images at 32 and at 64 frames, at the default
# gain.  The device's frames are the oracle's bit for bit and its filter and blend the reference's, so the figures are the host's.
def test_the_blend_beats_both_images_at_32_and_64_frames(mrt):
    q = QUALITY
    with _state(mrt, q["w"], q["h"], seed=q["ref_seed"], tracking=False, depth=q["depth"]) as st:
        st.render(q["ref_frames"])
        ref = st.read_framebuffer()
    with _state(mrt, q["w"], q["h"], seed=q["seed"], depth=q["depth"]) as st:
        for n in q["counts"]:
            st.render(n - st.frames_done)
            st.set_denoise_mix(False)
            noisy, den = rmse(st.read_framebuffer(), ref), rmse(st.read_denoised(), ref)
            st.set_denoise_mix(True)
            mix = rmse(st.read_denoised(), ref)
            print(f"{n} frames: noisy {noisy:.5f}  denoised {den:.5f}  blend {mix:.5f}  ({mix / min(noisy, den):.3f} x the better one)")
            assert mix < noisy and mix < den, (n, noisy, den, mix)


def _read_pfm(path, w, h):
    raw = open(path, "rb").read()
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], np.float32).reshape(h, w, 3)


# --denoise-mix with a GAIN, without one in front of another flag, and without one at the end of the line
@pytest.mark.parametrize("flags,gain", [(["--denoise-mix", "2.5", "--frames", "8"], 2.5), (["--denoise-mix", "--frames", "8"], None),
                                        (["--frames", "8", "--denoise-mix"], None)])
def test_native_runner_blends_its_denoised_frame(mrt, tmp_path, flags, gain):
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "myraytracer_amd", "lib", "native_runner")
    out = str(tmp_path / "f.pfm")
    r = subprocess.run([exe, "--scene", "default", "--width", "48", "--height", "32", "--denoise-out", out] + flags,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with mrt.State(mrt.Args(48, 32, 1, 50, 1.0), seed=1) as st:
        st.set_world(mrt.scene_default())
        st.set_noise_tracking(True)
        st.render(8)
        plain = st.read_denoised()
        st.set_denoise_mix(True, gain)
        want = st.read_denoised()
    assert np.array_equal(_bits(_read_pfm(out, 48, 32)), _bits(want[..., :3]))
    assert not np.array_equal(_bits(want), _bits(plain))
    if gain is not None:                                 # without --denoise-out the flag is refused
        r = subprocess.run([exe, "--scene", "default", "--width", "48", "--height", "32"] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--denoise-out" in r.stderr
