"""The noise estimate across shards and the gathered frame's denoise (include/myraytracer_amd.h, "the noise estimate across
shards"): mrt_set_gather_noise, mrt_read_gathered_noise, mrt_read_gathered_denoised, MRT_PRESENT_GATHERED_DENOISED,
mrt_debug_read_gathered_guides, and native_runner --devices ... --denoise-out.

Shards are several contexts on device 0, as in tests/test_gpu_multi.py.  No tolerance anywhere: the reference of every check is
the UNSHARDED context of the same seed and frames, compared bit for bit as uint32 views -- a shard's rows and its S are the
unsharded ones (tests/test_gpu_noise.py), every context holds the same scene and camera, and the filter reads (colour, S, K,
guides) in the layout of world == 1."""
import os
import subprocess
import sys

import numpy as np
import pytest

from present_ref import encode_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "myraytracer_amd", "lib")

# (world, root, W, H): two even shards; three of 6 bands with a ragged edge; ONE band, so four of five shards hold only padding;
# eight shards of 25 bands, i.e. uneven band counts
SHAPES = [(2, 1, 96, 54), (3, 2, 70, 45), (5, 0, 33, 7), (8, 0, 64, 200)]
SPP, DEPTH, SEED = 2, 50, 7
MODES = ("accumulated", "prefiltered", "spatial-early")
ERR_INVALID_ARG, ERR_STATE = 1, 7


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def where(a, b):
    neq = np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)
    return f"{int(neq.sum())} of {neq.size} words differ, the first at {tuple(int(i[0]) for i in np.nonzero(neq))}" if neq.any() else "identical"


def scene(mrt):
    return mrt.scene_cover(1, True)


def make(mrt, w, h, world, cam="scene", tracking=True, root=None, gather_noise=True):
    """the unsharded context and the `world` shards of it, all with the same scene, camera and seed"""
    sc, look_at = scene(mrt)
    out = []
    for shard in [None] + [(r, world) for r in range(world)]:
        st = mrt.State(mrt.Args(w, h, SPP, DEPTH), seed=SEED, shard=shard)
        if tracking:
            st.set_noise_tracking(True)
        st.set_world(sc)
        if cam == "scene":
            st.set_camera(look_at)
        elif cam is not None:
            st.set_camera(cam)
        out.append(st)
    if root is not None and gather_noise:
        out[1 + root].set_gather_noise(True)
    return out[0], out[1:]


def close(ref, shards):
    for st in [ref] + list(shards):
        st.close()


def frame(ref, shards):
    ref.redraw()
    for st in shards:
        st.redraw()                     # asynchronous: no sync between the shards or before the gather


@pytest.mark.parametrize("world,root,w,h", SHAPES)
def test_the_gathered_noise_is_the_unsharded_noise(mrt, world, root, w, h):
    """(1) S travels with the colour, in both forms of the copies, and the colour is what it was"""
    ref, shards = make(mrt, w, h, world, root=root)
    try:
        frame(ref, shards)
        frame(ref, shards)
        fb, s = ref.read_framebuffer(), ref.read_noise()
        R = shards[root]
        for per_band in (False, True):
            R.debug_set_gather_per_band(per_band)
            mrt.gather(shards, root)
            got_s, got = R.read_gathered_noise(), R.read_gathered()
            assert same(got_s, s), f"S, per_band {per_band}: {where(got_s, s)}"
            assert same(got, fb), f"colour, per_band {per_band}: {where(got, fb)}"
        assert R.debug_check_context() is None
    finally:
        close(ref, shards)


@pytest.mark.parametrize("camera", ["pinhole", "look-at"])
@pytest.mark.parametrize("world,root,w,h", SHAPES)
def test_the_roots_guides_are_the_full_images(mrt, world, root, w, h, camera):
    """(2) the guide pass over the full image on a root that holds only its own bands (its tile count and seed texture are a
    shard's): every field of every pixel"""
    ref, shards = make(mrt, w, h, world, cam=None if camera == "pinhole" else "scene", root=root)
    try:
        want, got = ref.debug_read_guides(), shards[root].debug_read_gathered_guides()
        assert sorted(got) == sorted(want) == ["albedo", "index", "normal", "rays", "t"]
        for k in want:
            assert same(got[k], want[k]), f"{k}: {where(got[k], want[k])}"
        assert (want["index"] >= 0).any()
        with pytest.raises(mrt.MrtError) as e:          # the old refusal holds
            shards[root].debug_read_guides()
        assert e.value.status == ERR_STATE
    finally:
        close(ref, shards)


@pytest.mark.parametrize("world,root,w,h", SHAPES)
def test_the_gathered_denoise_is_the_unsharded_denoise(mrt, world, root, w, h):
    """(3) every variance mode after 1 frame (K = +inf), 2 and 4 frames -- with spatial_frames = 3 on both sides of
    SPATIAL_EARLY's switch -- and with parameters that are not the defaults"""
    ref, shards = make(mrt, w, h, world, root=root)
    R = shards[root]
    try:
        for n in (1, 2, 3, 4):
            frame(ref, shards)
            if n == 3:
                continue
            mrt.gather(shards, root)
            wants = {}
            for mode in MODES:
                ref.set_denoise_variance(mode, 3)
                R.set_denoise_variance(mode, 3)
                wants[mode], got = ref.read_denoised(), R.read_gathered_denoised()
                assert same(got, wants[mode]), f"{n} frames, {mode}: {where(got, wants[mode])}"
            if n == 2:
                assert not same(wants["accumulated"], ref.read_framebuffer())           # (the filter did something)
                prm = dict(iterations=3, sigma_l=2.5, normal_exp=8, sigma_z=0.5, sigma_a=0.3)
                ref.set_denoise_params(**prm)
                R.set_denoise_params(**prm)
                for mode in MODES[:2]:
                    ref.set_denoise_variance(mode, 3)
                    R.set_denoise_variance(mode, 3)
                    other, got = ref.read_denoised(), R.read_gathered_denoised()
                    assert same(got, other), f"non-default parameters, {mode}: {where(got, other)}"
                    assert not same(other, wants[mode])
                ref.set_denoise_params(**mrt.denoise_params_default())
                R.set_denoise_params(**mrt.denoise_params_default())
        assert R.debug_check_context() is None
    finally:
        close(ref, shards)


def test_a_gather_of_one_is_read_denoised(mrt):
    """world == 1: the gathered frame's denoise on the context itself is mrt_read_denoised's image"""
    ref, shards = make(mrt, 70, 45, 1, root=0)
    try:
        frame(ref, shards)
        frame(ref, shards)
        mrt.gather(shards, 0)
        assert same(shards[0].read_gathered_denoised(), ref.read_denoised())
        assert same(shards[0].read_gathered_denoised(), shards[0].read_denoised())
        assert same(shards[0].read_gathered_noise(), ref.read_noise())
    finally:
        close(ref, shards)


def test_the_denoise_uses_the_gathers_snapshot(mrt):
    """(4) K and frames_done are the gather's: the shards (the root among them) render one more frame without a gather and the
    gathered frame's denoise is still the unsharded one AT 2 FRAMES -- in the accumulated mode the live K would differ, in
    SPATIAL_EARLY with spatial_frames = 3 the live frame count (3) would pick the other variance.  A second gather: 3 frames."""
    world, root, w, h = 3, 2, 70, 45
    ref, shards = make(mrt, w, h, world, root=root)
    R = shards[root]
    try:
        frame(ref, shards)
        frame(ref, shards)
        mrt.gather(shards, root)
        want2 = {}
        for mode in MODES:
            ref.set_denoise_variance(mode, 3)
            want2[mode] = ref.read_denoised()
        frame(ref, shards)                              # no gather
        assert R.frames_done == 3
        want3 = {}
        for mode in MODES:
            ref.set_denoise_variance(mode, 3)
            want3[mode] = ref.read_denoised()
            assert not same(want3[mode], want2[mode])
            R.set_denoise_variance(mode, 3)
            got = R.read_gathered_denoised()
            assert same(got, want2[mode]), f"{mode}, after a frame without a gather: {where(got, want2[mode])}"
        mrt.gather(shards, root)
        for mode in MODES:
            R.set_denoise_variance(mode, 3)
            got = R.read_gathered_denoised()
            assert same(got, want3[mode]), f"{mode}, after the second gather: {where(got, want3[mode])}"
    finally:
        close(ref, shards)


def test_a_new_camera_rebuilds_the_roots_guides(mrt):
    """(5) mrt_set_camera marks the guides stale on a shard too"""
    world, root, w, h = 3, 2, 70, 45
    ref, shards = make(mrt, w, h, world, root=root)
    R = shards[root]
    _, cam = scene(mrt)
    moved = mrt.Camera(mode=cam.mode, lookfrom=(cam.lookfrom[0] + 2.0, cam.lookfrom[1] + 0.5, cam.lookfrom[2] - 1.0), lookat=cam.lookat,
                       vup=cam.vup, vfov_deg=cam.vfov_deg + 10.0, defocus_angle_deg=cam.defocus_angle_deg, focus_dist=cam.focus_dist)
    try:
        frame(ref, shards)
        mrt.gather(shards, root)
        first = ref.read_denoised()
        assert same(R.read_gathered_denoised(), first)               # (the guides of the first camera exist now)
        for st in [ref] + shards:
            st.set_camera(moved)
        frame(ref, shards)
        mrt.gather(shards, root)
        want, got = ref.read_denoised(), R.read_gathered_denoised()
        assert same(got, want), where(got, want)
        assert not same(want, first)
        g, gw = R.debug_read_gathered_guides(), ref.debug_read_guides()
        assert all(same(g[k], gw[k]) for k in gw)
    finally:
        close(ref, shards)


def test_present_of_the_denoised_gathered_frame(mrt):
    """(6) MRT_PRESENT_GATHERED_DENOISED: the encode of mrt_read_gathered_denoised's image, the unsharded present(denoise=True)"""
    from myraytracer_amd import _lib
    world, root, w, h = 3, 2, 70, 45
    ref, shards = make(mrt, w, h, world, root=root)
    R = shards[root]
    try:
        frame(ref, shards)
        frame(ref, shards)
        mrt.gather(shards, root)
        R.present("rgba8", flip=True, gathered_denoised=True)
        img, info = R.acquire_presented()
        assert info["flags"] == _lib.PRESENT_FLIP_Y | _lib.PRESENT_GATHERED_DENOISED == 33
        assert (info["rows"], info["width"], info["frames_done"]) == (h, w, 2)
        want = encode_host(_lib.load(), R.read_gathered_denoised(), "rgba8", flip=True)
        assert np.array_equal(img, want)
        ref.present("rgba8", flip=True, denoise=True)
        img1, _ = ref.acquire_presented()
        assert np.array_equal(img, img1)
        assert not np.array_equal(img, encode_host(_lib.load(), R.read_gathered(), "rgba8", flip=True))
        R.present("bgra8", flip=False, gathered_denoised=True)
        img2, info2 = R.acquire_presented()
        assert info2["flags"] == 32 and np.array_equal(img2, encode_host(_lib.load(), R.read_gathered_denoised(), "bgra8", flip=False))
    finally:
        close(ref, shards)


def _refused(mrt, status, call, *a, **kw):
    with pytest.raises(mrt.MrtError) as e:
        call(*a, **kw)
    assert e.value.status == status, e.value
    return str(e.value)


def test_refusals(mrt):
    """(7)"""
    world, root, w, h = 2, 1, 96, 54
    ref, shards = make(mrt, w, h, world, root=root, gather_noise=False)
    R = shards[root]
    reads = (R.read_gathered_noise, R.read_gathered_denoised)
    try:
        frame(ref, shards)
        for rd in reads:                                    # before a gather
            assert "nothing gathered" in _refused(mrt, ERR_STATE, rd)
        _refused(mrt, ERR_STATE, R.present, gathered_denoised=True)
        mrt.gather(shards, root)                            # the setting is off
        for rd in reads:
            assert "no S" in _refused(mrt, ERR_STATE, rd)
        _refused(mrt, ERR_STATE, R.present, gathered_denoised=True)
        R.set_gather_noise(True)                            # on, but the latest gather carried none
        for rd in reads:
            _refused(mrt, ERR_STATE, rd)
        mrt.gather(shards, root)
        assert same(R.read_gathered_noise(), ref.read_noise())
        R.set_gather_noise(True)                            # (no change: nothing is dropped)
        assert same(R.read_gathered_denoised(), ref.read_denoised())
        R.set_gather_noise(False)                           # a toggle drops it ...
        for rd in reads:
            _refused(mrt, ERR_STATE, rd)
        R.set_gather_noise(True)                            # ... until the next gather
        for rd in reads:
            _refused(mrt, ERR_STATE, rd)
        mrt.gather(shards, root)
        assert same(R.read_gathered_noise(), ref.read_noise())
        # the new flag is a source of its own
        for other in ("gathered", "denoise", "temporal"):
            _refused(mrt, ERR_INVALID_ARG, R.present, gathered_denoised=True, **{other: True})
        # the old refusals hold
        assert "shard" in _refused(mrt, ERR_STATE, R.read_denoised)
        assert "no S" in _refused(mrt, ERR_INVALID_ARG, R.present, gathered=True, denoise=True)
        # one shard a frame ahead
        shards[0].redraw()
        msg = _refused(mrt, ERR_STATE, mrt.gather, shards, root)
        assert "ctxs[0]" in msg and "frames" in msg
        assert same(R.read_gathered(), ref.read_framebuffer())          # (nothing was queued)
        R.redraw()
        ref.redraw()
        mrt.gather(shards, root)
        assert same(R.read_gathered_denoised(), ref.read_denoised())
        # mrt_set_shard drops the gathered S
        for st in shards:
            st.reset()
        R.set_shard(root, world)
        for rd in reads:
            _refused(mrt, ERR_STATE, rd)
        assert R.debug_check_context() is None
        # a capacity that is too small
        from myraytracer_amd import _lib
        L = _lib.load()
        for st in shards:
            st.redraw()
        mrt.gather(shards, root)
        buf = np.empty(w * h * 4, np.float32)
        assert L.mrt_read_gathered_noise(R._ctx, buf.ctypes.data, w * h - 1) == 6
        assert L.mrt_read_gathered_denoised(R._ctx, buf.ctypes.data, w * h * 4 - 1) == 6
        assert L.mrt_read_gathered_denoised(R._ctx, buf.ctypes.data, w * h * 4) == 0
    finally:
        close(ref, shards)


def test_a_shard_without_noise_tracking_refuses_the_gather(mrt):
    """(7) ... before anything is queued: the previous gathered frame reads back unchanged"""
    world, root, w, h = 2, 1, 96, 54
    sc, cam = scene(mrt)
    shards = []
    try:
        for r in range(world):
            st = mrt.State(mrt.Args(w, h, SPP, DEPTH), seed=SEED, shard=(r, world))
            if r == root:
                st.set_noise_tracking(True)
            st.set_world(sc)
            st.set_camera(cam)
            st.redraw()
            shards.append(st)
        R = shards[root]
        mrt.gather(shards, root)                            # the setting is off: as always
        before = R.read_gathered()
        for st in shards:
            st.redraw()
        R.set_gather_noise(True)
        msg = _refused(mrt, ERR_STATE, mrt.gather, shards, root)
        assert "ctxs[0]" in msg and "noise tracking" in msg
        assert same(R.read_gathered(), before)
        _refused(mrt, ERR_STATE, R.read_gathered_noise)
        # without a scene: MRT_ERR_NO_SCENE
        with mrt.State(mrt.Args(w, h, SPP, DEPTH), seed=SEED) as bare:
            with pytest.raises(mrt.MrtError) as e:
                bare.debug_read_gathered_guides()
            assert e.value.status == 4
    finally:
        for st in shards:
            st.close()


def _read_device(ptr, shape):
    """float32 device memory at `ptr`, copied out by the HIP runtime the library itself runs on (already in the process)"""
    import ctypes as C
    from myraytracer_amd import _lib
    hip = C.CDLL(_lib._needed_hip_soname(), mode=os.RTLD_NOW | os.RTLD_NOLOAD)
    hip.hipMemcpy.restype, hip.hipMemcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(shape, np.float32)
    assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


def test_the_setting_off_changes_nothing(mrt):
    """(8) the gather with the setting off (noise tracking on) is the gather as it was, and the device pointer is the colour's
    with the setting on too"""
    world, root, w, h = 3, 2, 70, 45
    ref, shards = make(mrt, w, h, world, root=root, gather_noise=False)
    R = shards[root]
    try:
        frame(ref, shards)
        fb = ref.read_framebuffer()
        for on in (False, True):
            R.set_gather_noise(on)
            mrt.gather(shards, root)
            assert same(R.read_gathered(), fb)              # (synchronises)
            assert R.gathered_device_ptr() != 0
            view = _read_device(R.gathered_device_ptr(), (h, w, 4))
            assert same(view, fb), f"setting {on}: mrt_gathered_device_ptr does not point at the colour"
    finally:
        close(ref, shards)


def test_gather_rccl_carries_the_noise():
    """RCCL: a caller-made communicator of one rank (what one GPU allows), in a fresh process, one run"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_gather_noise_check.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_native_runner_denoises_the_gathered_frame(tmp_path):
    """native_runner --devices 0,0,0 --denoise-out: the bytes of the one-device run, and --out is what it was"""
    exe = os.path.join(LIBDIR, "native_runner")
    common = ["--width", "120", "--height", "68", "--samples-per-frame", "2", "--ray-depth", "50", "--frames", "3", "--seed", "3",
              "--scene", "cover-glass", "--denoise-variance", "spatial-early:4"]
    files = {}
    for name, extra in (("one", []), ("three", ["--devices", "0,0,0"])):
        files[name] = (str(tmp_path / f"{name}.pfm"), str(tmp_path / f"{name}_den.pfm"))
        r = subprocess.run([exe] + common + extra + ["--out", files[name][0], "--denoise-out", files[name][1]], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    assert "3 GPU(s)" in r.stdout
    for k in (0, 1):
        assert open(files["one"][k], "rb").read() == open(files["three"][k], "rb").read()
    assert open(files["one"][0], "rb").read() != open(files["one"][1], "rb").read()
    # --adaptive keeps its refusal
    r = subprocess.run([exe] + common + ["--devices", "0,0", "--target-noise", "0.1", "--adaptive"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "one GPU" in r.stderr
