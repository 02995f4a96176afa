"""The denoise of an adaptive accumulation on the GPU (include/myraytracer_amd.h, "Adaptive accumulations";
mrt_set_denoise_adaptive): the per-tile field and a-trous kernels bit for bit against their float32 restatement
(tests/denoise_tiles_ref.py) on injected accumulations (mrt_debug_load_accumulation) and on a real adaptive run, the reduction to
the uniform path, the setting's contract, and native_runner --adaptive --denoise-out.  Every comparison is on uint32 views."""
import os
import subprocess

import numpy as np
import pytest

from denoise_ref import random_case
from denoise_tiles_ref import denoise_tiles, library_k, tile_map
from denoise_var_ref import MODES
from present_ref import encode_host

pytestmark = pytest.mark.gpu

MRT_ERR_INVALID_ARG, MRT_ERR_STATE = 1, 7
OTHER = {"sigma_l": 2.5, "normal_exp": 3, "sigma_z": 0.4, "sigma_a": 0.25}
LIBDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "myraytracer_amd", "lib")
SPATIAL_FRAMES = 4
COUNTS = [0, 1, 2, SPATIAL_FRAMES - 1, SPATIAL_FRAMES, 40]


def _state(mrt, w, h, seed=3, tracking=True, adaptive=True):
    st = mrt.State(mrt.Args(w, h, 1, 8, 1.0), seed=seed)
    st.set_world(mrt.scene_default())
    if tracking:
        st.set_noise_tracking(True)
    st.set_denoise_adaptive(adaptive)
    return st


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _refused(mrt, call, status=MRT_ERR_STATE):
    with pytest.raises(mrt.MrtError) as e:
        call()
    assert e.value.status == status


# W x H: 3 x 2 whole tiles; ragged in both axes (5 x 4 tiles); one band shorter than a tile; ragged, more than one block in y
@pytest.mark.parametrize("width,height", [(24, 16), (37, 29), (70, 3), (45, 37)])
def test_injected_accumulations_are_the_reference(mrt, width, height):
    rng = np.random.default_rng(width * height)
    rgba, S, _ = random_case(rng, height, width)            # colour and S with NaN / Inf texels and zero S; the guides are the scene's
    tiles = tile_map(rng, height, width, COUNTS)
    assert set(COUNTS) <= set(int(v) for v in tiles.ravel())
    k_of = library_k(1.0)
    with _state(mrt, width, height) as st:
        st.debug_load_accumulation(rgba, S, tiles)
        assert st.frames_done == 0
        assert np.array_equal(_bits(st.read_framebuffer()), _bits(rgba)) and np.array_equal(_bits(st.read_noise()), _bits(S))
        assert np.array_equal(st.tile_frames(), tiles)
        guides = st.debug_read_guides()
        for mode in range(3):
            st.set_denoise_variance(mode, SPATIAL_FRAMES)
            for params in ({}, OTHER):
                for it in (1, 5):
                    st.set_denoise_params(**dict(mrt.denoise_params_default(), **params, iterations=it))
                    got = st.read_denoised()
                    want = denoise_tiles(rgba, S, tiles, guides, st.denoise_params(), mode, SPATIAL_FRAMES, k_of)
                    assert np.array_equal(_bits(got), _bits(want)), (mode, params, it)
                    # exactly the colours that came in not finite go out so (a texel whose S is not finite keeps its colour)
                    assert np.array_equal(np.isfinite(got[..., :3]).all(-1), np.isfinite(rgba[..., :3]).all(-1))


def test_a_uniform_map_is_the_uniform_path(mrt):
    w, h = 48, 32
    with _state(mrt, w, h, adaptive=False) as a, _state(mrt, w, h) as b:
        for n in (1, 2, 5):
            a.render(n - a.frames_done)
            fb, S = a.read_framebuffer(), a.read_noise()
            b.debug_load_accumulation(fb, S, np.full((4, 6), n, np.uint32))
            for mode in MODES:
                a.set_denoise_variance(mode, 3)
                b.set_denoise_variance(mode, 3)
                assert np.array_equal(_bits(b.read_denoised()), _bits(a.read_denoised())), (n, mode)


def test_a_real_adaptive_run(mrt):
    from myraytracer_amd import _lib
    L = _lib.load()
    with _state(mrt, 48, 32) as st:
        st.render(4)
        for _ in range(2):
            st.noise_query()
            rep = st.noise_result(wait=True)
            used, selected = st.render_adaptive(2, rep["seq"])
            assert used == rep["seq"] and 0 < selected < 24
        fb, S, tiles = st.read_framebuffer(), st.read_noise(), st.tile_frames()
        assert len(np.unique(tiles)) > 1 and tiles.min() == 4
        guides = st.debug_read_guides()
        for mode in range(3):
            st.set_denoise_variance(mode, 6)                 # (the tiles left at 4 frames are in their spatial phase in mode 2)
            got = st.read_denoised()
            want = denoise_tiles(fb, S, tiles, guides, st.denoise_params(), mode, 6, library_k(1.0))
            assert np.array_equal(_bits(got), _bits(want)), mode
            assert np.array_equal(_bits(st.read_denoised()), _bits(got))
            st.present("rgba8", flip=True, denoise=True)
            img, info = st.acquire_presented(newest=True, wait=True)
            assert info["flags"] & _lib.PRESENT_DENOISED
            assert np.array_equal(img, encode_host(L, got, "rgba8", flip=True))
        assert not np.array_equal(_bits(got), _bits(fb))
        # the denoise reads the accumulation and leaves it alone
        assert np.array_equal(_bits(st.read_framebuffer()), _bits(fb)) and np.array_equal(_bits(st.read_noise()), _bits(S))
        assert np.array_equal(st.tile_frames(), tiles)


def test_the_settings_contract(mrt):
    w, h = 48, 32
    with _state(mrt, w, h, adaptive=False) as st:
        assert st.denoise_adaptive() is False               # off by default: refused after divergence, as ever
        st.render(2)
        off = st.read_denoised()
        st.set_denoise_adaptive(True)                        # on, not diverged: the uniform path's bits
        assert st.denoise_adaptive() is True
        assert np.array_equal(_bits(st.read_denoised()), _bits(off))
        st.set_denoise_adaptive(False)
        st.render_tiles([1, 2, 7])
        for call in (st.read_denoised, lambda: st.present("rgba8", denoise=True), st.debug_read_guides):
            _refused(mrt, call)
        st.set_denoise_adaptive(True)
        on = st.read_denoised()
        st.present("rgba8", denoise=True)
        st.set_denoise_adaptive(False)                       # off again: refused again
        for call in (st.read_denoised, lambda: st.present("rgba8", denoise=True)):
            _refused(mrt, call)
        st.set_denoise_adaptive(True)
        assert np.array_equal(_bits(st.read_denoised()), _bits(on))
        _refused(mrt, lambda: st.present("rgba8", flip=False, denoise=True, gathered=True), MRT_ERR_INVALID_ARG)
        # the setting outlives the accumulation, the scene, the camera and the shard
        st.reset()
        assert st.denoise_adaptive() is True
        st.set_noise_tracking(True)
        st.set_world(mrt.scene_default())
        spheres, cam = mrt.scene_cover(1, False)
        st.set_world(spheres)
        st.set_camera(cam)
        assert st.denoise_adaptive() is True
        st.render(1)
        st.render_tiles([0])
        st.read_denoised()
        st.reset()
        st.set_shard(0, 2)
        assert st.denoise_adaptive() is True
        st.set_noise_tracking(True)
        st.redraw()
        for call in (st.read_denoised, lambda: st.present("rgba8", flip=False, denoise=True)):     # a shard stays refused
            _refused(mrt, call)
        _refused(mrt, lambda: st.debug_load_accumulation(tile_frames=np.zeros(24, np.uint32)))
    with _state(mrt, w, h, tracking=False) as st:            # tracking off stays refused, diverged or not
        st.render(2)
        _refused(mrt, st.read_denoised)
        st.render_tiles([3])
        _refused(mrt, st.read_denoised)
        # the diagnostic: S needs tracking; a count the K table is not made for; colour and the map alone are fine
        _refused(mrt, lambda: st.debug_load_accumulation(S=np.zeros((h, w), np.float32)))
        bad = np.zeros((4, 6), np.uint32)
        bad[1, 2] = 1 << 20
        before = st.tile_frames()
        _refused(mrt, lambda: st.debug_load_accumulation(tile_frames=bad), MRT_ERR_INVALID_ARG)
        assert np.array_equal(st.tile_frames(), before)
        st.debug_load_accumulation(rgba=np.ones((h, w, 4), np.float32), tile_frames=np.full((4, 6), 9, np.uint32))
        assert (st.read_framebuffer() == 1).all() and (st.tile_frames() == 9).all() and st.frames_done == 3
        st.debug_load_accumulation()                         # nothing given: nothing changes
        assert (st.tile_frames() == 9).all()


def _read_pfm(path, w, h):
    raw = open(path, "rb").read()
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], np.float32).reshape(h, w, 3)


# target 0.2: the case as first stated -- on this scene it is met at the first check, before any subset frame, so the run stays
# uniform; target 0.02 is not met within the 24 frames, so the later chunks are subset frames and the denoise is the per-tile one
@pytest.mark.parametrize("target,diverges", [("0.2", False), ("0.02", True)])
def test_native_runner_denoises_its_adaptive_run(mrt, tmp_path, target, diverges):
    exe = os.path.join(LIBDIR, "native_runner")
    out = str(tmp_path / "f.pfm")
    r = subprocess.run([exe, "--scene", "default", "--width", "48", "--height", "32", "--target-noise", target, "--check-every", "4",
                        "--frames", "24", "--adaptive", "--denoise-out", out], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    with mrt.State(mrt.Args(48, 32, 1, 50, 1.0), seed=1) as st:
        st.set_world(mrt.scene_default())
        st.render_until(float(target), 24, check_every=4, adaptive=True)
        st.set_denoise_adaptive(True)
        want = st.read_denoised()
        tiles = st.tile_frames()
    print(f"target {target}: n_t from {tiles.min()} to {tiles.max()}")
    assert np.array_equal(_bits(_read_pfm(out, 48, 32)), _bits(want[..., :3]))
    assert (len(np.unique(tiles)) > 1) == diverges
