"""The camera-ray cluster masks on the device (myraytracer_amd/csrc/cam_mask.hip; the sweep's AND: kernels.hip).

The build kernel's table against the float64 reference of tests/camera_mask_ref.py and the oracle's `required` set on the cases
of tests/camera_mask_cases.py; frames with the masks in force bit-identical to the oracle's and to the same context with the
masks switched off, with equal samples / world_hit_calls / rng_draws and strictly fewer member tests; the table rebuilt after
mrt_set_camera and after mrt_update_spheres + mrt_regroup_spheres; a large scene runs without masks.

A frame of fewer than 512 samples per pixel builds a stale table only once its scene / camera / shard has survived a frame
(frames.cpp, camera_masks): the masks are in force from the second frame on, whatever the timing."""
import numpy as np
import pytest

import camera_mask_ref as R
from camera_mask_cases import CASES, case
from common import mismatch_report, oracle_render

pytestmark = pytest.mark.gpu
KEYS = ("samples", "world_hit_calls", "rng_draws")


def _frames(mrt, sc, cam, W, H, spp, depth, frames, masks=True, shard=None, rng_mode=0, batch_form=0, seed=3):
    """(framebuffer, counters, mask info after the last frame); batch_form 2 / 3: one mrt_redraw, then ONE mrt_render of the other
    frames with the batch's form forced (2: a lane keeps its pixel for the batch's frames, 3: the frames as queue layers)"""
    with mrt.State(mrt.Args(W, H, spp, depth, 1.0), seed=seed, shard=shard) as st:
        st.debug_set_camera_masks(masks)
        st.set_world(sc)
        if cam is not None:
            st.set_camera(cam)
        if rng_mode:
            st.set_rng_mode(rng_mode)
        if batch_form:
            st.debug_set_frame_batching(batch_form)
            st.redraw()
            st.render(frames - 1)
        else:
            for _ in range(frames):
                st.redraw()
        st.sync()
        return st.read_framebuffer(), st.read_counters(), st.debug_read_camera_masks(table=False)


@pytest.mark.parametrize("name", CASES)
def test_device_masks_cover_the_required_set_and_are_as_tight_as_the_reference(mrt, oracle, name):
    c = case(mrt, oracle, name)
    with mrt.State(mrt.Args(c["W"], c["H"], 1, 4, 1.0), seed=3) as st:
        st.set_world(c["sc"])
        if c["cam"] is not None:
            st.set_camera(c["cam"])
        first = st.debug_read_camera_masks()
        assert first["entries"] == (R.local_texels(c["W"], c["H"]) + 7) // 8 and first["words"] == 4
        assert not first["in_force"] and not first["built"] and (first["masks"] == 0xFFFFFFFF).all()     # all ones until built
        st.redraw()
        assert not st.debug_read_camera_masks(table=False)["in_force"]          # 1 spp: not before the setting has survived a frame
        st.redraw()
        st.sync()
        got = st.debug_read_camera_masks()
        hier = st.debug_read_hierarchy()
    assert got["in_force"] and got["built"]
    # the device's own member records are the host builder's (the reference reads those)
    assert np.array_equal(np.asarray(hier["nodes"], np.float32).reshape(-1, 4)[:len(c["members"])].view(np.uint32), c["members"].view(np.uint32))
    ri, si = R.missing_pairs(got["masks"], c["ray_tex"], c["required"], c["cluster_of"])
    assert len(ri) == 0, f"{name}: {len(ri)} required (ray, sphere) pairs lie in a cluster the device's entry does not set"
    ref = R.camera_masks_ref(c["members"], c["n_top"], c["direct_first"], c["raw"], c["W"], c["H"])
    dev_bits, ref_bits = R.mask_bits(got["masks"]).sum(1).mean(), R.mask_bits(ref).sum(1).mean()
    print(f"{name}: {dev_bits:.3f} bits per entry on the device, {ref_bits:.3f} in the reference")
    assert dev_bits <= 1.25 * ref_bits


# expect: whether the last launch runs with the masks (and the run has strictly fewer member tests than without them)
RUNS = {
    "cover-glass 64x36": dict(case="cover-glass", spp=4, depth=50, frames=3, expect=True),
    "21x13": dict(case="21x13", spp=4, depth=50, frames=3, expect=True),
    # mrt_render(3) after one frame: the batch's lanes keep their pixels and make a camera ray per frame -- with masks
    "mrt_render(3), in the lane": dict(case="cover-glass", spp=2, depth=50, frames=4, batch_form=2, expect=True),
    # ... the same batch as layers of the tile queue: `texel` carries the layer's offset, the launch runs without masks
    "mrt_render(3), queue layers": dict(case="cover-glass", spp=2, depth=50, frames=4, batch_form=3, expect=False),
    "counter rng": dict(case="cover-glass", spp=4, depth=50, frames=3, rng_mode=1, expect=True),
    # counter mode beyond one block of samples: layers of the queue whose `texel` stays the pixel's own -- with masks
    "counter rng, 3 layers": dict(case="21x13", spp=130, depth=50, frames=2, rng_mode=1, expect=True),
    # a frame at the threshold builds before its first launch
    "512 spp, first frame": dict(case="21x13", spp=512, depth=8, frames=1, expect=True),
}


@pytest.mark.parametrize("run", list(RUNS))
def test_frames_with_masks_equal_the_oracle_and_the_frames_without(mrt, oracle, run):
    r = dict(RUNS[run])
    c = case(mrt, oracle, r.pop("case"))
    spp, depth, frames, expect = r.pop("spp"), r.pop("depth"), r.pop("frames"), r.pop("expect")
    cnt = oracle.Counters()
    ref = oracle_render(oracle, c["sc"], c["cam"], c["W"], c["H"], spp, depth, 3, frames=frames, counters=cnt, rng_mode=r.get("rng_mode", 0))
    on, con, info = _frames(mrt, c["sc"], c["cam"], c["W"], c["H"], spp, depth, frames, True, **r)
    off, coff, info_off = _frames(mrt, c["sc"], c["cam"], c["W"], c["H"], spp, depth, frames, False, **r)
    assert not info_off["in_force"]
    assert info["in_force"] == expect and info["built"] == expect
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32)), mismatch_report(on, off)
    assert np.array_equal(on.view(np.uint32), ref.view(np.uint32)), mismatch_report(on, ref)
    assert tuple(con[k] for k in KEYS) == tuple(coff[k] for k in KEYS) == (cnt.samples, cnt.world_hit_calls, cnt.rng_draws)
    print(f"{run}: member tests {con['member_tests']} with masks, {coff['member_tests']} without")
    if expect:
        assert con["member_tests"] < coff["member_tests"]
    else:
        assert con["member_tests"] == coff["member_tests"]


def test_a_shard_of_three_renders_its_rows_of_the_whole_frame(mrt, oracle):
    """shard (1, 3) of 40x24: one band, rows 8 .. 15; 40 x 8 texels, entries of 8 texels within a row"""
    c = case(mrt, oracle, "cover-glass")
    W, H, spp, depth, frames = 40, 24, 4, 50, 3
    ref = oracle_render(oracle, c["sc"], c["cam"], W, H, spp, depth, 3, frames=frames)
    on, con, info = _frames(mrt, c["sc"], c["cam"], W, H, spp, depth, frames, True, shard=(1, 3))
    off, coff, _ = _frames(mrt, c["sc"], c["cam"], W, H, spp, depth, frames, False, shard=(1, 3))
    assert info["in_force"] and info["entries"] == 40
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32)), mismatch_report(on, off)
    assert tuple(con[k] for k in KEYS) == tuple(coff[k] for k in KEYS)
    for lr in range(0, on.shape[0], 8):
        g = mrt.shard_global_row(lr, 1, 3)
        if g < H:
            assert np.array_equal(on[lr:lr + 8].view(np.uint32), ref[g:g + 8].view(np.uint32)), g
    assert con["member_tests"] < coff["member_tests"]


def test_a_new_camera_gets_new_masks(mrt, oracle):
    a, b = case(mrt, oracle, "cover-glass"), case(mrt, oracle, "inside-a-cluster")
    W, H, spp, depth = 64, 36, 4, 50
    fresh, cf, _ = _frames(mrt, b["sc"], b["cam"], W, H, spp, depth, 3)
    with mrt.State(mrt.Args(W, H, spp, depth, 1.0), seed=3) as st:
        st.set_world(a["sc"])
        st.set_camera(a["cam"])
        st.redraw(); st.redraw()
        assert st.debug_read_camera_masks(table=False)["in_force"]
        st.set_camera(b["cam"])
        assert not st.debug_read_camera_masks(table=False)["built"]
        st.reset()
        st.redraw()
        assert not st.debug_read_camera_masks(table=False)["in_force"]          # stale: the old camera's table is not used
        st.redraw(); st.redraw()
        st.sync()
        info = st.debug_read_camera_masks()
        got, cg = st.read_framebuffer(), st.read_counters()
    assert info["in_force"] and info["built"]
    assert np.array_equal(got.view(np.uint32), fresh.view(np.uint32)), mismatch_report(got, fresh)
    assert tuple(cg[k] for k in KEYS) == tuple(cf[k] for k in KEYS)
    ri, _ = R.missing_pairs(info["masks"], b["ray_tex"], b["required"], b["cluster_of"])
    assert len(ri) == 0


def test_moved_and_regrouped_spheres_get_new_masks(mrt, oracle):
    c = case(mrt, oracle, "cover-glass")
    W, H, spp, depth = 64, 36, 4, 50
    rng = np.random.default_rng(23)
    moved = c["sc"].copy()
    k = 120                                                         # the first spheres after the ground: small ones on the plane
    moved["center"][1:1 + k, 0] += rng.uniform(-1.5, 1.5, k).astype(np.float32)
    moved["center"][1:1 + k, 2] += rng.uniform(-1.5, 1.5, k).astype(np.float32)
    xyzr = np.concatenate([moved["center"][1:1 + k], moved["radius"][1:1 + k, None]], 1).astype(np.float32)
    fresh, cf, _ = _frames(mrt, moved, c["cam"], W, H, spp, depth, 3)
    fresh_off, _, _ = _frames(mrt, moved, c["cam"], W, H, spp, depth, 3, masks=False)
    assert np.array_equal(fresh.view(np.uint32), fresh_off.view(np.uint32))
    with mrt.State(mrt.Args(W, H, spp, depth, 1.0), seed=3) as st:
        st.set_world(c["sc"])
        st.set_camera(c["cam"])
        st.redraw(); st.redraw()
        before = st.debug_read_camera_masks()
        assert before["in_force"]
        st.update_spheres(1, xyzr)
        st.regroup_spheres()
        assert not st.debug_read_camera_masks(table=False)["built"]
        st.reset()
        st.redraw(); st.redraw(); st.redraw()
        st.sync()
        after = st.debug_read_camera_masks()
        got, cg = st.read_framebuffer(), st.read_counters()
    assert after["in_force"] and after["built"] and not np.array_equal(before["masks"], after["masks"])
    assert np.array_equal(got.view(np.uint32), fresh.view(np.uint32)), mismatch_report(got, fresh)
    assert tuple(cg[k] for k in KEYS) == tuple(cf[k] for k in KEYS)


def test_a_large_scene_runs_without_masks(mrt):
    sc, cam = mrt.scene_stress(1, 100)
    on, con, info = _frames(mrt, sc, cam, 64, 36, 1, 4, 2)
    off, coff, _ = _frames(mrt, sc, cam, 64, 36, 1, 4, 2, masks=False)
    assert info["entries"] == 0 and not info["in_force"] and not info["built"]
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
    assert con == coff
