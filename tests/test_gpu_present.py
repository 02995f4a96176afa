"""The present pass on the GPU (mrt_present / mrt_present_acquire, include/myraytracer_amd.h): the reference's pass 2 of
State::redraw (lib.rs:270-297, sample_framebuffer.wgsl) as a device kernel into 8-bit sRGB, read back through a ring of
pinned buffers without waiting for the frames in flight.  Every image must be bit-identical to the host's encoding
(mrt_srgb8 + the linear alpha rule, tests/present_ref.py) of the exact-float read-back of the same frame."""
import numpy as np
import pytest

from present_ref import alpha8_host, encode_host, srgb8_host

pytestmark = pytest.mark.gpu

MRT_ERR_INVALID_ARG, MRT_ERR_STATE = 1, 7


def _L(mrt):
    return mrt._lib.load()


def _scene(mrt, st, name):
    if name == "default":
        st.set_world(mrt.scene_default())
    else:
        spheres, cam = mrt.scene_cover(1, name == "cover-glass")
        st.set_world(spheres)
        st.set_camera(cam)


def _encoding_inputs(mrt):
    t = mrt.srgb8_thresholds()[1:]
    f0, f2 = np.float32(0), np.float32(2)
    vals = [t, np.nextafter(t, f0), np.nextafter(t, f2),
            np.array([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0xFF800001, 0x7FA00000], np.uint32).view(np.float32),
            np.array([np.inf, -np.inf, -0.0, 0.0, 1.0, np.nextafter(f2 / 2, f0), 1e-45, -1e-45, 1.1754942e-38, 5e-39, 2.0,
                      -0.5, 3.4028235e38], np.float32),
            np.arange(0, 0x3F800001, 4099, dtype=np.uint32).view(np.float32)]       # a strided sweep of [0, 1]
    v = np.concatenate(vals).astype(np.float32)
    v = np.concatenate([v, np.roll(v, 1), np.roll(v, 2), np.roll(v, 3)])          # every value in every channel
    return v[: len(v) // 4 * 4].reshape(-1, 4)


def test_encoding_is_bit_identical_to_the_host(mrt):
    L = _L(mrt)
    texels = _encoding_inputs(mrt)
    rgb = srgb8_host(L, texels[:, :3])
    alpha = alpha8_host(texels[:, 3])
    with mrt.State(mrt.Args(16, 16, 1, 8, 1.0), seed=1) as st:
        for width in (1, 3, 5, 63, 64, 65, 1920):
            rows = -(-len(texels) // width)
            pad = rows * width - len(texels)
            src = np.concatenate([texels, np.zeros((pad, 4), np.float32)]).reshape(rows, width, 4)
            want = np.zeros((rows * width, 4), np.uint8)
            want[: len(texels), :3], want[: len(texels), 3] = rgb, alpha
            want = want.reshape(rows, width, 4)
            for fmt in ("rgba8", "bgra8"):
                for flip in (False, True):
                    got = st.debug_present_encode(src, fmt, flip)
                    w = want[..., [2, 1, 0, 3]] if fmt == "bgra8" else want
                    w = w[::-1] if flip else w
                    bad = np.argwhere(got != w)
                    assert bad.size == 0, (width, fmt, flip, bad[:4].tolist(),
                                           [src[::-1][tuple(b[:2])].tolist() if flip else src[tuple(b[:2])].tolist() for b in bad[:2]])


@pytest.mark.parametrize("scene,w,h,spp,depth,fmt", [("default", 80, 45, 4, 8, "rgba8"), ("default", 80, 45, 4, 8, "bgra8"),
                                                     ("cover-glass", 97, 31, 2, 50, "rgba8"), ("cover", 97, 31, 2, 50, "bgra8")])
def test_a_rendered_frame_presents_as_the_host_encodes_it(mrt, scene, w, h, spp, depth, fmt):
    L = _L(mrt)
    with mrt.State(mrt.Args(w, h, spp, depth, 1.0), seed=3) as st:
        _scene(mrt, st, scene)
        for _ in range(3):
            st.redraw()
        st.present(fmt, flip=True)
        img, info = st.acquire_presented(newest=True, wait=True)
        ref = st.read_framebuffer()
        assert info["frames_done"] == 3 and info["seq"] == 1 and info["width"] == w and info["rows"] == h
        assert info["row_bytes"] == 4 * w and info["flags"] == 1 and info["format"] == (2 if fmt == "bgra8" else 1)
        assert np.array_equal(img, encode_host(L, ref, fmt, flip=True))
        st.render(3)                                      # after mrt_render(k): the batch's last frame
        st.present(fmt, flip=False)
        img, info = st.acquire_presented(newest=True, wait=True)
        assert info["frames_done"] == 6 and info["seq"] == 2
        assert np.array_equal(img, encode_host(L, st.read_framebuffer(), fmt, flip=False))
        st.release_presented()


def test_every_frame_in_fifo_order_matches_serial_frames(mrt):
    L = _L(mrt)
    args = mrt.Args(96, 54, 4, 50, 1.0)
    frames = 12
    got = {}
    with mrt.State(args, seed=9) as st:
        _scene(mrt, st, "cover-glass")
        st.set_schedule_hint(4, 1)
        st.set_present_ring(4)
        outstanding = 0
        for _ in range(frames):
            st.redraw()
            st.present("rgba8", flip=True)
            outstanding += 1
            if outstanding == 3:
                img, info = st.acquire_presented(newest=False, wait=True)
                got[info["frames_done"]] = (img, info)
                outstanding -= 1
        assert st.get_schedule()["frames_in_flight"] >= min(4, st.get_schedule()["max_concurrent_frames"] or 4)
        while outstanding:
            img, info = st.acquire_presented(newest=False, wait=True)
            got[info["frames_done"]] = (img, info)
            outstanding -= 1
        st.release_presented()
        assert st.acquire_presented(newest=False, wait=True) is None
    assert sorted(got) == list(range(1, frames + 1))
    assert [got[k][1]["seq"] for k in range(1, frames + 1)] == list(range(1, frames + 1))
    assert all(i["dropped"] == 0 and i["ring_depth"] == 4 for _, i in got.values())
    with mrt.State(args, seed=9) as st:
        _scene(mrt, st, "cover-glass")
        st.debug_set_frames_in_flight(1)
        for k in range(1, frames + 1):
            st.redraw()
            st.sync()
            ref = encode_host(L, st.read_framebuffer(), "rgba8", flip=True)
            assert np.array_equal(got[k][0], ref), k


def test_presenting_changes_nothing(mrt):
    args = mrt.Args(96, 54, 2, 50, 1.0)
    out = []
    for present in (False, True):
        with mrt.State(args, seed=4) as st:
            _scene(mrt, st, "cover-glass")
            for _ in range(24):
                st.redraw()
                if present:
                    st.present("bgra8", flip=True)
                    st.acquire_presented(newest=True, wait=False)
            out.append((st.read_framebuffer(), st.read_counters(), st.frames_done, list(st.locals.rng_shuffle)))
    (fb0, c0, n0, s0), (fb1, c1, n1, s1) = out
    assert np.array_equal(fb0.view(np.uint32), fb1.view(np.uint32))
    assert c0 == c1 and n0 == n1 == 24 and s0 == s1


def test_presenting_every_frame_does_not_drain_the_pipeline(mrt):
    """test_gpu_schedule's caller that reads back every frame drops to the whole chip per launch; one that presents every
    frame and acquires the newest image without waiting keeps its frames in flight and its narrow launches."""
    L = _L(mrt)
    spheres, cam = mrt.scene_cover(1, True)
    with mrt.State(mrt.Args(640, 360, 64, 50, 1.0), seed=5) as st:
        st.set_world(spheres); st.set_camera(cam)
        st.set_schedule_hint(8, 1)
        shares, seen = [], []
        for _ in range(12):
            st.redraw()
            st.present("rgba8", flip=True)
            r = st.acquire_presented(newest=True, wait=False)
            if r is not None:
                seen.append(r[1]["frames_done"])
            shares.append(st.get_schedule()["last_launch_div"])
        # (a launch is never narrower than the frames that can really run side by side: 8 here, or the hardware queues' limit)
        running = min(8, st.get_schedule()["max_concurrent_frames"] or 8)
        assert shares[0] == 8 and shares[1:] == [running] * 11, shares
        assert seen == sorted(seen)
        st.sync()
        img, info = st.acquire_presented(newest=True, wait=True)
        assert info["frames_done"] == 12 and info["seq"] == 12 and info["ring_depth"] >= 4
        assert np.array_equal(img, encode_host(L, st.read_framebuffer(), "rgba8", flip=True))


@pytest.mark.parametrize("world", [2, 3, 4])
def test_gathered_present_on_the_root(mrt, world):
    L = _L(mrt)
    args = mrt.Args(72, 50, 2, 50, 1.0)
    root = world - 1
    refs = {}
    with mrt.State(args, seed=6) as whole:
        _scene(mrt, whole, "cover-glass")
        for k in (1, 2):
            whole.redraw()
            refs[k] = whole.read_framebuffer()
    states = [mrt.State(args, seed=6, shard=(i, world)) for i in range(world)]
    try:
        for s in states:
            _scene(mrt, s, "cover-glass")
        R = states[root]
        with pytest.raises(mrt.MrtError) as e:
            R.present("rgba8", flip=True, gathered=True)              # nothing gathered yet
        assert e.value.status == MRT_ERR_STATE
        for s in states:
            s.redraw()
        mrt.gather(states, root)
        R.present("rgba8", flip=True, gathered=True)                  # frame 1 ...
        for s in states:
            s.redraw()
        mrt.gather(states, root)                                      # ... then frame 2 is gathered over it
        img, info = R.acquire_presented(newest=False, wait=True)
        assert info["frames_done"] == 1 and info["rows"] == 50 and info["flags"] == 3
        assert np.array_equal(img, encode_host(L, refs[1], "rgba8", flip=True))
        R.present("bgra8", flip=False, gathered=True)
        img, info = R.acquire_presented(newest=True, wait=True)
        assert info["frames_done"] == 2
        assert np.array_equal(img, encode_host(L, R.read_gathered(), "bgra8", flip=False))
        assert np.array_equal(R.read_gathered().view(np.uint32), refs[2].view(np.uint32))
    finally:
        for s in states:
            s.close()


def test_a_shard_presents_its_packed_rows(mrt):
    L = _L(mrt)
    with mrt.State(mrt.Args(70, 45, 2, 50, 1.0), seed=2, shard=(1, 3)) as st:
        _scene(mrt, st, "cover")
        st.redraw(); st.redraw()
        with pytest.raises(mrt.MrtError) as e:
            st.present("rgba8", flip=True)
        assert e.value.status == MRT_ERR_INVALID_ARG
        st.present("rgba8", flip=False)
        img, info = st.acquire_presented(newest=True, wait=True)
        rows = st.shard_info()[2]
        assert img.shape == (rows, 70, 4) and info["rows"] == rows
        assert np.array_equal(img, encode_host(L, st.read_framebuffer(), "rgba8", flip=False))


def test_errors_and_lifetimes(mrt):
    import ctypes as C
    L = _L(mrt)
    with mrt.State(mrt.Args(64, 40, 2, 8, 1.0), seed=8) as st:
        _scene(mrt, st, "cover")
        for call in (lambda: st.acquire_presented(), lambda: st.release_presented(),
                     lambda: st.present("rgba8", gathered=True)):
            with pytest.raises(mrt.MrtError) as e:
                call()
            assert e.value.status == MRT_ERR_STATE
        for bad in (0, 3, -1):
            assert L.mrt_present(st._ctx, bad, 0) == MRT_ERR_INVALID_ARG
        assert L.mrt_present(st._ctx, 1, 4) == MRT_ERR_INVALID_ARG
        px = C.POINTER(C.c_uint8)()
        assert L.mrt_present_acquire(st._ctx, 2, 0, C.byref(px), None) == MRT_ERR_INVALID_ARG
        for bad in (1, 19):
            with pytest.raises(mrt.MrtError) as e:
                st.set_present_ring(bad)
            assert e.value.status == MRT_ERR_INVALID_ARG
        st.redraw()
        st.present()
        st.present()
        st.reset()                                    # the outstanding images are discarded
        assert st.acquire_presented(wait=True) is None
        st.redraw()
        st.present()
        view, info = st.acquire_presented(wait=True, copy=False)
        assert info["seq"] == 3 and info["frames_done"] == 1 and not view.flags.owndata
        with pytest.raises(mrt.MrtError) as e:
            st.set_present_ring(3)                    # an image is held
        assert e.value.status == MRT_ERR_STATE
        st.release_presented()
        st.set_present_ring(3)
        st.set_present_ring(0)
    # destroy with copies in flight and an image held
    st = mrt.State(mrt.Args(1280, 720, 16, 50, 1.0), seed=8)
    _scene(mrt, st, "cover-glass")
    st.redraw()
    st.present()
    st.acquire_presented(wait=True, copy=False)
    for _ in range(3):
        st.redraw()
        st.present()
    st.close()
