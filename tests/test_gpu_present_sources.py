"""The image sources of mrt_present and of the float read-backs (present.cpp, denoise.cpp: ImageSource), from outside.

The refusal table: for every combination of the five present flag bits (FLIP_Y, GATHERED, DENOISED, TEMPORAL,
GATHERED_DENOISED) and one word with an undefined bit, the (status, mrt_last_error text) of mrt_present(ctx, RGBA32F, flags) in
four contexts, and the same pair for mrt_read_denoised / mrt_read_temporal / mrt_read_gathered_denoised with a buffer that is
large enough and with cap = 1.  tests/golden/present_source_refusals.json holds what the library answered BEFORE the sources
got one table (the flag chain, the shims and the three read-backs written out); the test asks for the same answers, messages
byte for byte.  `python tests/test_gpu_present_sources.py --record` rewrites the file from the library in use
(MRT_LIB_OVERRIDE selects another build); under pytest the module only compares.

Source parity: an rgba32f image presented without flip holds the bits of its source's read-back."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "present_source_refusals.json")
W, H, SPP, DEPTH, SEED = 20, 12, 2, 8, 5         # 20 x 12: partial 8 x 8 tiles in both directions, two bands
RGBA32F = 32
UNDEFINED_BIT = 64 | 2 | 8                      # (with two source bits: the unknown bit is refused first)
WORDS = [w for w in range(64) if not w & 4] + [UNDEFINED_BIT]       # (bit 2 is no flag)
READS = ("mrt_read_denoised", "mrt_read_temporal", "mrt_read_gathered_denoised")
CONTEXTS = ("created", "temporal", "plain", "shard")


def _context(mrt, kind):
    """(a) created, no scene; (b) default scene, noise tracking and temporal on, 2 frames, one step; (c) the same with both off;
    (d) rank 0 of a world of 2 (noise tracking on) after 2 frames, nothing gathered"""
    st = mrt.State(mrt.Args(W, H, SPP, DEPTH), seed=SEED, shard=(0, 2) if kind == "shard" else None)
    if kind == "created":
        return st
    if kind in ("temporal", "shard"):
        st.set_noise_tracking(True)
    st.set_world(mrt.scene_default())
    if kind == "temporal":
        st.set_temporal(True)
    st.redraw()
    st.redraw()
    if kind == "temporal":
        st.temporal_step()
    return st


def _answer(L, ctx, status):
    return [int(status), L.mrt_last_error(ctx).decode() if status else ""]


def answers(mrt):
    """{context: {"present": {flags: [status, message]}, "read": {entry point: {"full" | "cap1": [status, message]}}}}"""
    L = mrt._lib.load()
    out = {}
    for kind in CONTEXTS:
        st = _context(mrt, kind)
        try:
            present = {}
            for flags in WORDS:
                status = L.mrt_present(st._ctx, RGBA32F, flags)
                present[str(flags)] = _answer(L, st._ctx, status)
                if status == 0:                     # (so that one context serves every word)
                    assert st.acquire_presented(newest=True, wait=True) is not None
                    st.release_presented()
            buf = np.empty(W * H * 4, np.float32)
            read = {name: {label: _answer(L, st._ctx, getattr(L, name)(st._ctx, buf.ctypes.data, cap))
                           for label, cap in (("full", buf.size), ("cap1", 1))} for name in READS}
            out[kind] = {"present": present, "read": read}
        finally:
            st.close()
    return out


def test_the_words_are_every_combination_and_one_undefined_bit(mrt):
    L = mrt._lib
    bits = (L.PRESENT_FLIP_Y, L.PRESENT_GATHERED, L.PRESENT_DENOISED, L.PRESENT_TEMPORAL, L.PRESENT_GATHERED_DENOISED)
    every = {sum(b for i, b in enumerate(bits) if k >> i & 1) for k in range(32)}
    assert len(WORDS) == 33 and set(WORDS[:32]) == every and len(every) == 32 and WORDS[32] & ~sum(bits)


def test_refusals_are_the_recorded_ones(mrt):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = answers(mrt)
    assert sorted(got) == sorted(want) == sorted(CONTEXTS)
    for kind in CONTEXTS:
        assert sorted(want[kind]["present"], key=int) == sorted(map(str, WORDS), key=int)
        for flags in map(str, WORDS):
            assert got[kind]["present"][flags] == want[kind]["present"][flags], (kind, "mrt_present", int(flags))
        for name in READS:
            for label in ("full", "cap1"):
                assert got[kind]["read"][name][label] == want[kind]["read"][name][label], (kind, name, label)
    # (the table is not all refusals, nor all of one kind)
    assert {a[0] for k in CONTEXTS for a in want[k]["present"].values()} >= {0, 1, 7}
    assert want["temporal"]["read"]["mrt_read_temporal"] == {"full": [0, ""], "cap1": [6, "mrt_read_temporal: need 960 floats"]}


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _presented(st, **source):
    st.present("rgba32f", flip=False, **source)
    img, info = st.acquire_presented(newest=True, wait=True)
    st.release_presented()
    return img, info


def test_every_source_is_its_read_back(mrt):
    """The five sources and a shard's own rows at 20 x 12 -- partial tiles in both directions, the second band four rows of
    image and four of padding.  At 80 x 45 and 70 x 45 tests/test_gpu_present_float.py holds most of these cells already
    (test_framebuffer_denoised_and_temporal_sources: accumulated, denoised and temporal with frames_done;
    test_gathered_sources_on_the_root: both gathered sources and the gather's snapshot in frames_done;
    test_a_shard_presents_its_packed_rows: a shard's rows); what no test held is the gathered frame's frames_done -- the
    context's count, not the gather's -- and any source at a size whose last tile row and column are partial."""
    with mrt.State(mrt.Args(W, H, SPP, DEPTH), seed=SEED) as st:
        st.set_noise_tracking(True)
        st.set_world(mrt.scene_default())
        st.set_temporal(True)
        st.redraw()
        st.redraw()
        st.temporal_step()
        for source, read in (({}, st.read_framebuffer), ({"denoise": True}, st.read_denoised), ({"temporal": True}, st.read_temporal)):
            img, info = _presented(st, **source)
            assert np.array_equal(img.view(np.uint32), _u32(read())), source
            assert (info["rows"], info["width"], info["frames_done"]) == (H, W, 2), source
    shards = [mrt.State(mrt.Args(W, H, SPP, DEPTH), seed=SEED, shard=(r, 2)) for r in range(2)]
    try:
        for s in shards:
            s.set_noise_tracking(True)
            s.set_world(mrt.scene_default())
        R = shards[0]
        R.set_gather_noise(True)
        for _ in range(2):
            for s in shards:
                s.redraw()
        mrt.gather(shards, 0)
        R.redraw()                                          # the root is one frame past its gather
        img, info = _presented(R, gathered=True)
        assert np.array_equal(img.view(np.uint32), _u32(R.read_gathered()))
        assert (info["rows"], info["frames_done"]) == (H, 3)
        img, info = _presented(R, gathered_denoised=True)
        assert np.array_equal(img.view(np.uint32), _u32(R.read_gathered_denoised()))
        assert (info["rows"], info["frames_done"]) == (H, 2)
        for s, frames in zip(shards, (3, 2)):               # a shard's own present: its packed rows, one band of 8
            img, info = _presented(s)
            assert np.array_equal(img.view(np.uint32), _u32(s.read_framebuffer()))
            assert (info["rows"], info["frames_done"]) == (8, frames)
    finally:
        for s in shards:
            s.close()


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_present_sources.py --record")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import myraytracer_amd
    with open(GOLDEN, "w") as f:
        json.dump(answers(myraytracer_amd), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {GOLDEN} from {myraytracer_amd._lib.LIB_PATH}")
