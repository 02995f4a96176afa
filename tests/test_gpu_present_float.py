"""The present pass's linear formats on the GPU (MRT_PRESENT_RGBA16F_LINEAR / MRT_PRESENT_RGBA32F_LINEAR, "rgba16f" / "rgba32f"):
the floats themselves through the ring of pinned buffers, without waiting for the frames in flight.  An rgba32f image must hold
the bits of the exact-float read-back of the same source, an rgba16f image mrt_half_bits (tests/test_present_float_host.py) of
every channel of it.  Texels of the tests' own reach the kernel through the context's framebuffer (debug_load_accumulation)."""
import os
import subprocess

import numpy as np
import pytest

from present_float_ref import boundary_set, image_of, rolled_texels, specials
from present_ref import encode_host

pytestmark = pytest.mark.gpu

MRT_ERR_INVALID_ARG, MRT_ERR_STATE = 1, 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = {"rgba16f": (16, 8, np.float16), "rgba32f": (32, 16, np.float32)}       # name: format, bytes per pixel, dtype


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cover(mrt, st, glass=False):
    spheres, cam = mrt.scene_cover(1, glass)
    st.set_world(spheres)
    st.set_camera(cam)


def _check(mrt, st, src, fmt, flip, frames_done=None, **source):
    """present `fmt` of a source whose exact floats are `src` ([rows, width, 4], row 0 = bottom) and hold the image against it"""
    code, bpp, dtype = FORMATS[fmt]
    st.present(fmt, flip=flip, **source)
    img, info = st.acquire_presented(newest=True, wait=True)
    st.release_presented()                      # (a held image would keep a wider format from regrowing the ring)
    rows, width, _ = src.shape
    assert img.dtype == dtype and img.shape == (rows, width, 4)
    assert (info["format"], info["row_bytes"], info["rows"], info["width"]) == (code, width * bpp, rows, width)
    assert (info["flags"] & 1) == int(flip)
    if frames_done is not None:
        assert info["frames_done"] == frames_done
    want = src[::-1] if flip else src
    if fmt == "rgba32f":
        got, want = img.view(np.uint32), _u32(want)
    else:
        got, want = img.view(np.uint16), mrt._lib.half_bits(want)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (fmt, flip, source, len(bad), [(b.tolist(), hex(int(got[tuple(b)])), hex(int(want[tuple(b)]))) for b in bad[:4]])
    return info


@pytest.mark.parametrize("width", [640, 641])
def test_encoding_of_every_rounding_boundary(mrt, width):
    """the host tests' boundary set and specials, every value in every channel: rows a multiple of 4 texels wide (two 16-B
    stores per quad) and not (8-B stores, a partial last quad)"""
    src = image_of(rolled_texels(np.concatenate([boundary_set(), specials()])), width)
    assert 490 <= src.shape[0] <= 500
    with mrt.State(mrt.Args(width, src.shape[0], 1, 8, 1.0), seed=1) as st:
        st.debug_load_accumulation(src)
        assert np.array_equal(_u32(st.read_framebuffer()), _u32(src))
        for fmt in FORMATS:
            for flip in (False, True):
                _check(mrt, st, src, fmt, flip)


@pytest.mark.parametrize("height", [1, 9])
@pytest.mark.parametrize("width", [1, 3, 4, 5, 8])
def test_smallest_shapes(mrt, width, height):
    """texels that name their place (x, y, channel), one NaN and one inf among them: a partial quad, a flip off by one row or a
    wrong row stride shows here"""
    y, x, ch = np.meshgrid(np.arange(height), np.arange(width), np.arange(4), indexing="ij")
    src = (64.0 * y + 4.0 * x + ch + 0.5).astype(np.float32)
    flat = src.reshape(-1)
    flat[len(flat) // 2] = np.array([0xFFA00001], np.uint32).view(np.float32)[0]
    flat[-1] = -np.inf
    with mrt.State(mrt.Args(width, height, 1, 8, 1.0), seed=1) as st:
        st.debug_load_accumulation(src)
        for fmt in FORMATS:
            for flip in (False, True):
                _check(mrt, st, src, fmt, flip)


def test_framebuffer_denoised_and_temporal_sources(mrt):
    with mrt.State(mrt.Args(80, 45, 2, 50, 1.0), seed=3) as st:
        st.set_noise_tracking(True)
        _cover(mrt, st)
        st.set_temporal(True)
        for _ in range(3):
            st.redraw()
            st.temporal_step()
        reads = {"framebuffer": ({}, st.read_framebuffer()), "denoised": ({"denoise": True}, st.read_denoised()),
                 "temporal": ({"temporal": True}, st.read_temporal())}
        assert not np.array_equal(_u32(reads["framebuffer"][1]), _u32(reads["denoised"][1]))
        for source, src in reads.values():
            for fmt in FORMATS:
                for flip in (False, True):
                    _check(mrt, st, src, fmt, flip, frames_done=3, **source)
        st.render(2)                                                    # after mrt_render(k): the batch's last frame, unread
        st.present("rgba32f", flip=False)
        img, info = st.acquire_presented(newest=True, wait=True)
        assert info["frames_done"] == 5 and np.array_equal(img.view(np.uint32), _u32(st.read_framebuffer()))


def test_gathered_sources_on_the_root(mrt):
    world, root = 3, 2
    states = [mrt.State(mrt.Args(80, 45, 2, 50, 1.0), seed=6, shard=(i, world)) for i in range(world)]
    try:
        for s in states:
            s.set_noise_tracking(True)
            _cover(mrt, s)
        R = states[root]
        R.set_gather_noise(True)
        for _ in range(2):
            for s in states:
                s.redraw()
        mrt.gather(states, root)
        for s in states:
            s.redraw()                                                  # (the root is one frame past its gather)
        gathered, denoised = R.read_gathered(), R.read_gathered_denoised()
        assert not np.array_equal(_u32(gathered), _u32(denoised))
        for fmt in FORMATS:
            for flip in (False, True):
                _check(mrt, R, gathered, fmt, flip, gathered=True)
                _check(mrt, R, denoised, fmt, flip, frames_done=2, gathered_denoised=True)
    finally:
        for s in states:
            s.close()


def test_a_shard_presents_its_packed_rows(mrt):
    with mrt.State(mrt.Args(70, 45, 2, 50, 1.0), seed=2, shard=(1, 3)) as st:
        _cover(mrt, st)
        st.redraw(); st.redraw()
        rows = st.shard_info()[2]
        packed = st.read_framebuffer()
        assert packed.shape == (rows, 70, 4)
        for fmt in FORMATS:
            with pytest.raises(mrt.MrtError) as e:
                st.present(fmt, flip=True)
            assert e.value.status == MRT_ERR_INVALID_ARG
            _check(mrt, st, packed, fmt, False, frames_done=2)


def test_every_frame_in_fifo_order_with_sixteen_frames_in_flight(mrt):
    args = mrt.Args(64, 40, 2, 50, 1.0)
    frames, keep = 24, 12
    got = {}
    with mrt.State(args, seed=9) as st:
        _cover(mrt, st, glass=True)
        st.debug_set_frames_in_flight(16)
        outstanding = 0

        def take():
            img, info = st.acquire_presented(newest=False, wait=True)
            assert info["frames_done"] not in got
            got[info["frames_done"]] = (img, info)
        for _ in range(frames):
            st.redraw()
            st.present("rgba32f", flip=False)
            outstanding += 1
            if outstanding == keep:
                take()
                outstanding -= 1
        for _ in range(outstanding):
            take()
        st.release_presented()
        assert st.acquire_presented(newest=False, wait=True) is None
    assert sorted(got) == list(range(1, frames + 1))
    assert [got[k][1]["seq"] for k in range(1, frames + 1)] == list(range(1, frames + 1))
    assert all(i["dropped"] == 0 and i["ring_depth"] > keep for _, i in got.values()), [i for _, i in got.values()][:3]
    with mrt.State(args, seed=9) as st:
        _cover(mrt, st, glass=True)
        st.debug_set_frames_in_flight(1)
        for k in range(1, frames + 1):
            st.redraw()
            st.sync()
            assert np.array_equal(got[k][0].view(np.uint32), _u32(st.read_framebuffer())), k


def test_a_wider_format_regrows_the_ring(mrt):
    L = mrt._lib.load()
    w, h = 64, 40
    with mrt.State(mrt.Args(w, h, 2, 8, 1.0), seed=8) as st:
        _cover(mrt, st)
        st.redraw()
        fb = st.read_framebuffer()
        st.present("rgba8", flip=False)
        st.present("bgra8", flip=False)
        st.present("rgba32f", flip=False)                   # the entries grow: the two images queued are discarded
        img, info = st.acquire_presented(newest=False, wait=True)
        assert (info["seq"], info["dropped"], info["format"], info["row_bytes"]) == (3, 2, 32, 16 * w)
        assert np.array_equal(img.view(np.uint32), _u32(fb))
        depth = info["ring_depth"]
        # the large entries serve every format from here on: nothing queued is lost to a narrower or an equal one (depth - 1
        # presents outstanding at the most, none held)
        assert depth >= 4
        st.release_presented()
        st.present("rgba32f", flip=True)
        st.present("rgba8", flip=False)
        st.present("rgba16f", flip=False)
        want = [(4, 32, 16 * w, _u32(fb[::-1])), (5, 1, 4 * w, encode_host(L, fb, "rgba8", flip=False)),
                (6, 16, 8 * w, mrt._lib.half_bits(fb))]
        for seq, fmt, row_bytes, bits in want:
            img, info = st.acquire_presented(newest=False, wait=True)
            assert (info["seq"], info["dropped"], info["format"], info["row_bytes"], info["ring_depth"]) == (seq, 0, fmt, row_bytes, depth)
            assert np.array_equal(img.view(bits.dtype), bits), seq
        st.release_presented()
        st.present("rgba32f", flip=False)
        img, info = st.acquire_presented(newest=False, wait=True)
        assert (info["seq"], info["dropped"], info["format"]) == (7, 0, 32) and np.array_equal(img.view(np.uint32), _u32(fb))
    with mrt.State(mrt.Args(w, h, 2, 8, 1.0), seed=8) as st:
        _cover(mrt, st)
        st.redraw()
        st.present("rgba8", flip=False)
        view, info = st.acquire_presented(wait=True, copy=False)
        assert info["format"] == 1 and view.dtype == np.uint8 and not view.flags.owndata
        for fmt in ("rgba16f", "rgba32f"):
            with pytest.raises(mrt.MrtError) as e:
                st.present(fmt, flip=False)                 # the image outgrows the entries while one of them is held
            assert e.value.status == MRT_ERR_STATE
        st.release_presented()
        st.present("rgba16f", flip=False)
        st.present("rgba32f", flip=False)                   # (grows once more: the rgba16f image is discarded)
        view, info = st.acquire_presented(newest=False, wait=True, copy=False)
        assert (info["seq"], info["dropped"], info["format"]) == (3, 1, 32) and view.dtype == np.float32 and not view.flags.owndata
        assert np.array_equal(view.view(np.uint32), _u32(st.read_framebuffer()))


def test_the_pinned_budget_caps_the_depth(mrt):
    """2048 x 2048 x 16 B: 256e6 / 67,108,864 = 3 entries, fewer than a new context's 2 frames in flight + 2"""
    w = h = 2048
    with mrt.State(mrt.Args(w, h, 1, 8, 1.0), seed=1) as st:
        assert st.get_schedule()["frames_in_flight"] + 2 > 3
        st.present("rgba32f", flip=False)                   # (no frame rendered: the framebuffer as created)
        img, info = st.acquire_presented(wait=True, copy=False)
        assert info["ring_depth"] == max(2, 256_000_000 // (w * h * 16)) == 3
        assert info["row_bytes"] == 16 * w and img.shape == (h, w, 4) and info["frames_done"] == 0


def test_refusals(mrt):
    L = mrt._lib.load()
    with mrt.State(mrt.Args(64, 40, 2, 8, 1.0), seed=8) as st:
        _cover(mrt, st)
        st.redraw()
        for bad in (0, 3, -1, 4, 15, 17, 33):
            assert L.mrt_present(st._ctx, bad, 0) == MRT_ERR_INVALID_ARG, bad
        # an unknown flag; GATHERED | DENOISED; TEMPORAL with either; GATHERED_DENOISED with any other source
        for flags in (4, 64, 2 | 8, 16 | 2, 16 | 8, 32 | 2, 32 | 8, 32 | 16):
            for fmt in (1, 2, 16, 32):
                assert L.mrt_present(st._ctx, fmt, flags) == MRT_ERR_INVALID_ARG, (fmt, flags)
        # sources this context does not have: as for the 8-bit formats
        for fmt in ("rgba8", "rgba16f", "rgba32f"):
            for source in ({"gathered": True}, {"denoise": True}, {"temporal": True}, {"gathered_denoised": True}):
                with pytest.raises(mrt.MrtError) as e:
                    st.present(fmt, **source)
                assert e.value.status == MRT_ERR_STATE, (fmt, source)
        with pytest.raises(mrt.MrtError):
            st.acquire_presented()                          # nothing was queued by any of them


def _read_pfm(path, w, h):
    raw = open(path, "rb").read()
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], np.float32).reshape(h, w, 3)


def test_native_runner_writes_snapshots(mrt, tmp_path):
    exe = os.path.join(ROOT, "myraytracer_amd", "lib", "native_runner")
    common = [exe, "--scene", "cover", "--width", "64", "--height", "40", "--samples-per-frame", "2", "--frames", "6"]
    r = subprocess.run(common + ["--snapshot-every", "2", "--snapshot-out", str(tmp_path / "s"), "--out", str(tmp_path / "final.pfm")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == ["final.pfm", "s00002.pfm", "s00004.pfm", "s00006.pfm"]
    with mrt.State(mrt.Args(64, 40, 2), seed=1) as st:
        _cover(mrt, st)
        for n in (2, 4, 6):
            st.render(2)
            want = st.read_framebuffer()[..., :3]
            assert np.array_equal(_read_pfm(tmp_path / f"s{n:05d}.pfm", 64, 40).view(np.uint32), _u32(want)), n
        assert np.array_equal(_read_pfm(tmp_path / "final.pfm", 64, 40).view(np.uint32), _u32(want))
    r = subprocess.run(common + ["--snapshot-every", "2", "--snapshot-out", str(tmp_path / "t"), "--target-noise", "0.1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--snapshot-every" in r.stderr, r.stdout + r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("t")]
