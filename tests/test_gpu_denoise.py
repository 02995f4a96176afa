"""The denoiser on the GPU (include/myraytracer_amd.h, "denoiser"): the first-hit guides against the oracle's world_hit and hit
record, the a-trous filter bit for bit against its float32 restatement (tests/denoise_ref.py), the context's denoise and the
DENOISED present against that restatement of the same frame, and the quality it buys on a cover scene."""
import numpy as np
import pytest

from denoise_ref import centre_rays, denoise, expected_guides, random_case
from present_ref import encode_host

pytestmark = pytest.mark.gpu

MRT_ERR_INVALID_ARG, MRT_ERR_STATE = 1, 7


def _scene(mrt, name):
    if name == "default":
        return mrt.scene_default(), None
    if name == "stress":
        return mrt.scene_stress(1, 100)            # 10,000 spheres: the large-scene (box walk) instantiations
    return mrt.scene_cover(1, name == "cover-glass")


def _state(mrt, w, h, spheres, cam, spp=1, depth=8, seed=3, **kw):
    st = mrt.State(mrt.Args(w, h, spp, depth, 1.0), seed=seed, **kw)
    st.set_world(spheres)
    if cam is not None:
        st.set_camera(cam)
    return st


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name,w,h", [("default", 96, 54), ("cover-glass", 96, 54), ("stress", 64, 40)])
def test_guides_equal_the_oracle(mrt, name, w, h):
    from oracle import pyoracle as O
    spheres, cam = _scene(mrt, name)
    with _state(mrt, w, h, spheres, cam) as st:
        g = st.debug_read_guides()
    raw = mrt.camera_derive(cam) if cam is not None else None
    assert np.array_equal(_bits(g["rays"]), _bits(centre_rays(w, h, raw)))
    hit, t, normal, albedo = expected_guides(O, spheres, g["rays"])
    assert np.array_equal(g["index"].ravel(), hit)
    assert (hit < 0).any() and (hit >= 0).any()
    assert np.array_equal(_bits(g["t"]).ravel(), _bits(t))
    assert np.array_equal(_bits(g["normal"]).reshape(-1, 3), _bits(normal))
    assert np.array_equal(_bits(g["albedo"]).reshape(-1, 3), _bits(albedo))


def test_guides_follow_the_camera_and_the_scene(mrt):
    sp_a, cam_a = _scene(mrt, "cover-glass")
    sp_b, cam_b = _scene(mrt, "default")
    cam_c = mrt.Camera(mode=1, lookfrom=(3.0, 2.0, 4.0), lookat=(0.0, 0.0, -1.0), vup=(0.0, 1.0, 0.0), vfov_deg=30.0,
                       defocus_angle_deg=0.0, focus_dist=5.0)

    def fresh(spheres, cam):
        with _state(mrt, 80, 48, spheres, cam) as st:
            return st.debug_read_guides()

    def same(a, b):
        return all(np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)) for k in a)

    with _state(mrt, 80, 48, sp_a, cam_a) as st:
        g0 = st.debug_read_guides()
        assert same(g0, fresh(sp_a, cam_a))
        st.set_camera(cam_c)
        g1 = st.debug_read_guides()
        assert not same(g0, g1) and same(g1, fresh(sp_a, cam_c))
        st.set_world(sp_b)
        g2 = st.debug_read_guides()
        assert not same(g1, g2) and same(g2, fresh(sp_b, cam_c))


@pytest.mark.parametrize("rows,width", [(37, 45), (8, 32), (61, 19)])
@pytest.mark.parametrize("params", [{}, {"sigma_l": 2.5, "normal_exp": 3, "sigma_z": 0.4, "sigma_a": 0.25}])
def test_debug_denoise_is_the_reference(mrt, rows, width, params):
    rng = np.random.default_rng(rows * width)
    rgba, S, guides = random_case(rng, rows, width)
    spheres, cam = _scene(mrt, "default")
    with _state(mrt, 16, 16, spheres, cam) as st:
        for it in range(1, 6):
            for K in (0.2, np.inf):
                p = dict(params, iterations=it)
                got = st.debug_denoise(rgba, S, K, guides, p)
                want = denoise(rgba, S, K, guides, p)
                assert np.array_equal(_bits(got), _bits(want)), (it, K)


def _reference_of(mrt, st):
    fb = st.read_framebuffer()
    K = mrt.noise_factor(st.frames_done, st.args.max_framebuffer_weight)
    return denoise(fb, st.read_noise(), K, st.debug_read_guides(), st.denoise_params())


@pytest.mark.parametrize("slots", [0, 4])
def test_read_denoised_is_the_reference_of_the_frame(mrt, slots):
    spheres, cam = _scene(mrt, "cover-glass")
    with _state(mrt, 100, 60, spheres, cam, spp=2, depth=12) as st:
        st.set_noise_tracking(True)
        if slots:
            st.debug_set_frames_in_flight(slots)
        st.render(1)
        d1 = st.read_denoised()                       # one frame: K = +inf, the guides alone
        assert np.array_equal(_bits(d1), _bits(_reference_of(mrt, st)))
        st.render(7)                                  # frames in flight when the denoise is queued
        d = st.read_denoised()
        assert np.array_equal(_bits(d), _bits(_reference_of(mrt, st)))
        st.set_denoise_params(iterations=3, sigma_l=2.0)
        st.render(2)
        d = st.read_denoised()
        assert np.array_equal(_bits(d), _bits(_reference_of(mrt, st)))


def test_denoised_presents_fifo_and_mailbox(mrt):
    from myraytracer_amd import _lib
    L = _lib.load()
    spheres, cam = _scene(mrt, "cover")
    with _state(mrt, 72, 40, spheres, cam, spp=1, depth=8) as st:
        st.set_noise_tracking(True)
        st.set_present_ring(8)
        refs = []
        for _ in range(5):
            st.redraw()
            st.present("bgra8", flip=True, denoise=True)
            refs.append(encode_host(L, st.read_denoised(), "bgra8", flip=True))
        for k in range(5):                             # FIFO: every image, oldest first
            img, info = st.acquire_presented(newest=False, wait=True)
            assert info["frames_done"] == k + 1 and info["flags"] & _lib.PRESENT_DENOISED
            assert np.array_equal(img, refs[k]), k
        for _ in range(3):
            st.redraw()
            st.present("rgba8", flip=False, denoise=True)
        st.sync()
        img, info = st.acquire_presented(newest=True, wait=True)   # mailbox: the newest
        assert info["frames_done"] == 8
        assert np.array_equal(img, encode_host(L, st.read_denoised(), "rgba8"))
        st.present("rgba8", flip=False)                # without the flag: the framebuffer itself
        img, info = st.acquire_presented(newest=True, wait=True)
        assert not info["flags"] & _lib.PRESENT_DENOISED
        assert np.array_equal(img, encode_host(L, st.read_framebuffer(), "rgba8"))


def test_denoised_presents_change_nothing(mrt):
    spheres, cam = _scene(mrt, "cover-glass")
    out = []
    for present in (False, True):
        with _state(mrt, 96, 54, spheres, cam, spp=2, depth=50, seed=4) as st:
            st.set_noise_tracking(True)
            for _ in range(16):
                st.redraw()
                if present:
                    st.present("bgra8", flip=True, denoise=True)
                    st.acquire_presented(newest=True, wait=False)
            out.append((st.read_framebuffer(), st.read_noise(), st.read_counters(), st.frames_done))
    (fb0, s0, c0, n0), (fb1, s1, c1, n1) = out
    assert np.array_equal(_bits(fb0), _bits(fb1)) and np.array_equal(_bits(s0), _bits(s1))
    assert c0 == c1 and n0 == n1 == 16


def test_presenting_denoised_every_frame_does_not_drain_the_pipeline(mrt):
    from myraytracer_amd import _lib
    L = _lib.load()
    spheres, cam = mrt.scene_cover(1, True)
    with _state(mrt, 640, 360, spheres, cam, spp=64, depth=50, seed=5) as st:
        st.set_noise_tracking(True)
        st.set_schedule_hint(8, 1)
        shares, seen = [], []
        for _ in range(12):
            st.redraw()
            st.present("rgba8", flip=True, denoise=True)
            r = st.acquire_presented(newest=True, wait=False)
            if r is not None:
                seen.append(r[1]["frames_done"])
            shares.append(st.get_schedule()["last_launch_div"])
        running = min(8, st.get_schedule()["max_concurrent_frames"] or 8)
        assert shares[0] == 8 and shares[1:] == [running] * 11, shares
        assert seen == sorted(seen)
        st.sync()
        img, info = st.acquire_presented(newest=True, wait=True)
        assert info["frames_done"] == 12 and info["seq"] == 12
        assert np.array_equal(img, encode_host(L, st.read_denoised(), "rgba8", flip=True))


def _rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def denoise_quality_curve(mrt, frames=(4, 16, 64, 256), w=320, h=192):
    """RMSE of the noisy and the denoised image against a 256-frame render (another seed), both uniform accumulation of 1 spp
    frames on the cover scene without glass: [(frames, noisy, denoised)]."""
    spheres, cam = mrt.scene_cover(1, False)
    with _state(mrt, w, h, spheres, cam, spp=1, depth=50, seed=101) as st:
        st.render(256)
        ref = st.read_framebuffer()
    out = []
    with _state(mrt, w, h, spheres, cam, spp=1, depth=50, seed=7) as st:
        st.set_noise_tracking(True)
        for n in frames:
            st.render(n - st.frames_done)
            out.append((n, _rmse(st.read_framebuffer(), ref), _rmse(st.read_denoised(), ref)))
    return out


def test_denoising_improves_an_early_preview(mrt):
    # measured with the default parameters (profiles/denoise_quality.txt): 0.72 x the noisy RMSE after 4 frames, 0.96 x after 64
    curve = dict((n, (a, b)) for n, a, b in denoise_quality_curve(mrt, (4, 64)))
    noisy, den = curve[4]
    assert den <= 0.8 * noisy, curve
    noisy, den = curve[64]
    assert den <= noisy, curve


def test_refusals(mrt):
    spheres, cam = _scene(mrt, "cover")
    with _state(mrt, 48, 32, spheres, cam) as st:
        st.redraw()
        for call in (st.read_denoised, lambda: st.present("rgba8", denoise=True)):
            with pytest.raises(mrt.MrtError) as e:        # noise tracking off
                call()
            assert e.value.status == MRT_ERR_STATE
        st.reset()
        st.set_noise_tracking(True)
        st.redraw()
        with pytest.raises(mrt.MrtError) as e:
            st.present("rgba8", gathered=True, denoise=True)
        assert e.value.status == MRT_ERR_INVALID_ARG
        for bad in ({"iterations": 0}, {"iterations": 9}, {"sigma_l": -1.0}, {"sigma_z": float("nan")}, {"sigma_a": 0.0},
                    {"normal_exp": 17}):
            with pytest.raises(mrt.MrtError) as e:
                st.set_denoise_params(**bad)
            assert e.value.status == MRT_ERR_INVALID_ARG
        assert st.denoise_params() == mrt.denoise_params_default()
        st.read_denoised()                                # and it still works
    with _state(mrt, 48, 32, spheres, cam, shard=(0, 2)) as st:
        st.set_noise_tracking(True)
        st.redraw()
        for call in (st.read_denoised, lambda: st.present("rgba8", flip=False, denoise=True), st.debug_read_guides):
            with pytest.raises(mrt.MrtError) as e:
                call()
            assert e.value.status == MRT_ERR_STATE
