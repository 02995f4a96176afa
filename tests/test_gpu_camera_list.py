"""The camera-ray sphere lists on the device (the build: myraytracer_amd/csrc/cam_mask.hip; the primary hit in the lane: kernels.hip).

The device's table against the float64 reference of tests/camera_list_ref.py and the oracle's `required` set; frames with the
lists in force bit-identical to the oracle's and to the same context with the lists (and masks) switched off, with equal samples /
world_hit_calls / rng_draws and per-pixel costs and strictly fewer member tests; the variations that decide whether a launch gets
the lists; an entry with more members than the cap, whose camera rays take world_hit.

A frame of fewer than the build threshold's samples per pixel builds a stale table only once its scene / camera / shard has
survived a frame (frames.cpp, camera_masks): the lists are in force from the second frame on, whatever the timing.  Images of
these sizes are bound by their pixel chains and would get the masks by the library's rule: the tests ask for the lists
(mrt_debug_set_camera_masks(2)); the rule itself has the last test."""
import numpy as np
import pytest

import camera_list_ref as L
import camera_mask_ref as R
from camera_list_cases import OVERFLOW_ENTRY, OVERFLOW_SHAPE, case
from common import mismatch_report, oracle_render, to_oracle_camera, to_oracle_spheres

pytestmark = pytest.mark.gpu
KEYS = ("samples", "world_hit_calls", "rng_draws")
SEED, SPP = 3, 16


def _frames(mrt, c, depth, frames=3, lists=True, shard=None, rng_mode=0, batch_form=0, in_flight=0, spp=SPP, W=None, H=None):
    """(framebuffer, counters, per-pixel costs of the last launch, table info, the lists' table); batch_form 2 / 3: one mrt_redraw,
    then ONE mrt_render of the other frames (2: a lane keeps its pixel for the batch's frames, 3: the frames as queue layers)"""
    with mrt.State(mrt.Args(W or c["W"], H or c["H"], spp, depth, 1.0), seed=SEED, shard=shard) as st:
        st.debug_set_camera_masks(2 if lists else 0)               # 2: the lists whatever the image's size
        st.set_world(c["sc"])
        if c["cam"] is not None:
            st.set_camera(c["cam"])
        if rng_mode:
            st.set_rng_mode(rng_mode)
        if in_flight:
            st.debug_set_frames_in_flight(in_flight)
        if batch_form:
            st.debug_set_frame_batching(batch_form)
            st.redraw()
            st.render(frames - 1)
        else:
            for _ in range(frames):
                st.redraw()
        st.sync()
        return st.read_framebuffer(), st.read_counters(), st.debug_read_pixel_costs(), st.debug_read_camera_masks(table=False), st.debug_read_camera_lists()


def _oracle_trips(oracle, c, depth, frame, rng_mode=0):
    trips = np.zeros((c["H"], c["W"]), np.uint32)
    oracle.render_frame(c["W"], c["H"], SPP, depth, oracle.pack_world(to_oracle_spheres(oracle, c["sc"])), to_oracle_camera(oracle, c["cam"]),
                        oracle.fill_seeds(SEED, c["W"], c["H"]), oracle.frame_shuffle(SEED, frame), rng_mode=rng_mode, trips=trips)
    return trips


def _same(on, off, what=KEYS):
    fb, cnt, px = on[:3]
    assert np.array_equal(fb.view(np.uint32), off[0].view(np.uint32)), mismatch_report(fb, off[0])
    assert tuple(cnt[k] for k in what) == tuple(off[1][k] for k in what)
    assert np.array_equal(px, off[2])


@pytest.mark.parametrize("shape", [(24, 16), (70, 43)])
@pytest.mark.parametrize("name", ["cover-glass", "default"])
def test_the_device_table_is_the_references(mrt, oracle, name, shape):
    c = case(mrt, oracle, name, *shape, rays=True)
    with mrt.State(mrt.Args(*shape, 1, 4, 1.0), seed=SEED) as st:
        st.debug_set_camera_masks(2)
        st.set_world(c["sc"])
        if c["cam"] is not None:
            st.set_camera(c["cam"])
        first = st.debug_read_camera_lists()
        assert first.shape == ((R.local_texels(*shape) + 7) // 8, 4) and (first[:, 0] == L.OVERFLOW).all()     # until built: world_hit
        st.redraw(); st.redraw()
        st.sync()
        info, words = st.debug_read_camera_masks(), st.debug_read_camera_lists()
    assert info["in_force"] and info["built"]
    got, over = L.unpack(words, c["n_slots"])
    ref = c["lists"]
    assert np.array_equal(over, ref.sum(1) > L.CAP)
    extra = got & ~ref
    assert not extra.any(), f"{int(extra.sum())} slots on the device's lists that the reference lacks"
    ri, _ = L.missing_pairs(got, over, c["ray_tex"], c["required"], c["slot_of"])
    assert len(ri) == 0, f"{len(ri)} required (ray, sphere) pairs are not on the device's list of the ray's entry"
    assert np.array_equal(got[~over], ref[~over])
    # the masks of the same build: a cluster's bit is the OR of its members
    pad = np.zeros((len(got), 4 * R.MAX_RECORDS), bool)
    pad[:, :c["n_slots"]] = got
    assert np.array_equal(pad.reshape(len(got), R.MAX_RECORDS, 4).any(2)[~over], R.mask_bits(info["masks"])[~over])


@pytest.mark.parametrize("depth", [50, 1, 0])
@pytest.mark.parametrize("shape", [(24, 16), (70, 43)])
@pytest.mark.parametrize("name", ["cover-glass", "default"])
def test_frames_with_lists_equal_the_oracle_and_the_frames_without(mrt, oracle, name, shape, depth):
    c = case(mrt, oracle, name, *shape)
    cnt = oracle.Counters()
    ref = oracle_render(oracle, c["sc"], c["cam"], *shape, SPP, depth, SEED, frames=3, counters=cnt)
    on, off = _frames(mrt, c, depth), _frames(mrt, c, depth, lists=False)
    assert on[3]["in_force"] and on[3]["lists"] and on[3]["built"] and not off[3]["in_force"]
    _same(on, off)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32)), mismatch_report(on[0], ref)
    assert tuple(on[1][k] for k in KEYS) == (cnt.samples, cnt.world_hit_calls, cnt.rng_draws)
    assert np.array_equal(on[2], _oracle_trips(oracle, c, depth, 2))
    assert on[1]["world_hit_calls"] <= on[1]["lane_slots"]
    print(f"{name} {shape} depth {depth}: member tests {on[1]['member_tests']} with lists, {off[1]['member_tests']} without; "
          f"lane slots {on[1]['lane_slots']} / {off[1]['lane_slots']}")
    if depth:
        assert on[1]["member_tests"] < off[1]["member_tests"]
    else:
        assert on[1]["member_tests"] == off[1]["member_tests"] == 0


# expect: whether the last launch runs with the lists
VARIATIONS = {
    "counter rng": dict(rng_mode=1, expect=True),
    # mrt_render(3) after one frame: the batch's lanes keep their pixels and make a camera ray per frame -- with lists
    "mrt_render(3), in the lane": dict(frames=4, batch_form=2, expect=True),
    # ... the same batch as layers of the tile queue: `texel` carries the layer's offset, the launch runs without them
    "mrt_render(3), queue layers": dict(frames=4, batch_form=3, expect=False),
    "two frames in flight": dict(frames=5, in_flight=2, expect=True),
}


@pytest.mark.parametrize("run", list(VARIATIONS))
def test_variations_of_the_launch(mrt, oracle, run):
    r = dict(VARIATIONS[run])
    expect = r.pop("expect")
    c = case(mrt, oracle, "cover-glass", 24, 16)
    cnt = oracle.Counters()
    ref = oracle_render(oracle, c["sc"], c["cam"], 24, 16, SPP, 50, SEED, frames=r.get("frames", 3), counters=cnt, rng_mode=r.get("rng_mode", 0))
    on, off = _frames(mrt, c, 50, **r), _frames(mrt, c, 50, lists=False, **r)
    assert on[3]["in_force"] == on[3]["lists"] == expect and on[3]["built"] == expect and not off[3]["in_force"]
    _same(on, off)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32)), mismatch_report(on[0], ref)
    assert tuple(on[1][k] for k in KEYS) == (cnt.samples, cnt.world_hit_calls, cnt.rng_draws)
    if expect:
        assert on[1]["member_tests"] < off[1]["member_tests"]
    else:
        assert on[1]["member_tests"] == off[1]["member_tests"]


def test_a_shard_of_three_renders_its_rows_of_the_whole_frame(mrt, oracle):
    """shard (1, 3) of 40x24: one band, rows 8 .. 15; 40 x 8 texels, entries of 8 texels within a row"""
    c = case(mrt, oracle, "cover-glass", 40, 24)
    ref = oracle_render(oracle, c["sc"], c["cam"], 40, 24, SPP, 50, SEED, frames=3)
    on, off = _frames(mrt, c, 50, shard=(1, 3)), _frames(mrt, c, 50, lists=False, shard=(1, 3))
    assert on[3]["in_force"] and on[3]["entries"] == 40
    _same(on, off)
    for lr in range(0, on[0].shape[0], 8):
        g = mrt.shard_global_row(lr, 1, 3)
        if g < 24:
            assert np.array_equal(on[0][lr:lr + 8].view(np.uint32), ref[g:g + 8].view(np.uint32)), g
    want = L.camera_lists_ref(c["members"], c["n_top"], c["direct_first"], c["raw"], 40, 24, rank=1, world=3)
    got, over = L.unpack(on[4], c["n_slots"])
    assert np.array_equal(over, want.sum(1) > L.CAP) and np.array_equal(got[~over], want[~over])
    assert on[1]["member_tests"] < off[1]["member_tests"]


def test_stale_tables_are_not_used_and_are_rebuilt(mrt, oracle):
    """after a camera change, and after mrt_update_spheres + mrt_regroup_spheres"""
    a, b = case(mrt, oracle, "cover-glass", 24, 16), case(mrt, oracle, "cover-pinhole", 24, 16)
    rng = np.random.default_rng(23)
    moved = b["sc"].copy()
    k = 120                                                         # the first spheres after the ground: small ones on the plane
    moved["center"][1:1 + k, 0] += rng.uniform(-1.5, 1.5, k).astype(np.float32)
    moved["center"][1:1 + k, 2] += rng.uniform(-1.5, 1.5, k).astype(np.float32)
    xyzr = np.concatenate([moved["center"][1:1 + k], moved["radius"][1:1 + k, None]], 1).astype(np.float32)
    fresh_b = _frames(mrt, b, 50, lists=False)
    fresh_moved = _frames(mrt, dict(b, sc=moved), 50, lists=False)
    with mrt.State(mrt.Args(24, 16, SPP, 50, 1.0), seed=SEED) as st:
        st.debug_set_camera_masks(2)
        st.set_world(a["sc"])
        st.set_camera(a["cam"])
        st.redraw(); st.redraw()
        assert st.debug_read_camera_masks(table=False)["in_force"]
        before = st.debug_read_camera_lists()
        st.set_camera(b["cam"])
        assert not st.debug_read_camera_masks(table=False)["built"]
        st.reset()
        st.redraw()
        assert not st.debug_read_camera_masks(table=False)["in_force"]          # stale: the old camera's table is not used
        st.redraw(); st.redraw()
        st.sync()
        info, words = st.debug_read_camera_masks(table=False), st.debug_read_camera_lists()
        assert info["in_force"] and info["built"] and not np.array_equal(words, before)
        got, over = L.unpack(words, b["n_slots"])
        assert np.array_equal(got[~over], b["lists"][~over]) and np.array_equal(over, b["lists"].sum(1) > L.CAP)
        _same((st.read_framebuffer(), st.read_counters(), st.debug_read_pixel_costs()), fresh_b)
        st.update_spheres(1, xyzr)
        st.regroup_spheres()
        assert not st.debug_read_camera_masks(table=False)["built"]
        st.reset()
        st.redraw(); st.redraw(); st.redraw()
        st.sync()
        info, again = st.debug_read_camera_masks(table=False), st.debug_read_camera_lists()
        assert info["in_force"] and info["built"] and not np.array_equal(words, again)
        _same((st.read_framebuffer(), st.read_counters(), st.debug_read_pixel_costs()), fresh_moved)


def test_an_overflowed_entry_takes_world_hit(mrt, oracle):
    W, H = OVERFLOW_SHAPE
    c = case(mrt, oracle, "overflow", W, H)
    assert list(np.nonzero(c["lists"].sum(1) > L.CAP)[0]) == [OVERFLOW_ENTRY]        # (the reference, here on the CPU)
    cnt = oracle.Counters()
    ref = oracle_render(oracle, c["sc"], c["cam"], W, H, SPP, 50, SEED, frames=3, counters=cnt)
    on, off = _frames(mrt, c, 50), _frames(mrt, c, 50, lists=False)
    assert on[3]["in_force"]
    assert list(np.nonzero(on[4][:, 0] == L.OVERFLOW)[0]) == [OVERFLOW_ENTRY]
    _same(on, off)
    assert np.array_equal(on[0].view(np.uint32), ref.view(np.uint32)), mismatch_report(on[0], ref)
    assert tuple(on[1][k] for k in KEYS) == (cnt.samples, cnt.world_hit_calls, cnt.rng_draws)
    assert np.array_equal(on[2], _oracle_trips(oracle, c, 50, 2))


def test_the_librarys_rule_gives_a_small_image_the_masks_and_the_switch_either_table(mrt, oracle):
    """24x16 is far below 5 pixels per lane the chip holds: bound by its pixel chains, it keeps the masks (frames.cpp, camera_masks)"""
    c = case(mrt, oracle, "cover-glass", 24, 16)
    got = {}
    for mode in (1, 2, 3):
        with mrt.State(mrt.Args(24, 16, SPP, 50, 1.0), seed=SEED) as st:
            st.debug_set_camera_masks(mode)
            st.set_world(c["sc"])
            st.set_camera(c["cam"])
            st.redraw(); st.redraw()
            st.sync()
            info = st.debug_read_camera_masks(table=False)
            got[mode] = (st.read_framebuffer(), st.read_counters(), info)
            assert info["in_force"] and info["lists"] == (mode == 2)
    for mode in (2, 3):
        assert np.array_equal(got[mode][0].view(np.uint32), got[1][0].view(np.uint32))
        assert tuple(got[mode][1][k] for k in KEYS) == tuple(got[1][1][k] for k in KEYS)
    assert got[1][1]["member_tests"] == got[3][1]["member_tests"] != got[2][1]["member_tests"]


def test_the_librarys_rule_gives_a_full_size_image_the_lists(mrt):
    """1920x1080 is 6.3 pixels per lane a 256-CU chip holds, above the rule's 5: under the default setting the second frame of a
    setting at 1 spp builds the tables and runs with the lists (and a 1200x675 image, 2.5, with the masks)"""
    sc, cam = mrt.scene_cover(1, True)
    for (w, h), lists in (((1920, 1080), True), ((1200, 675), False)):
        with mrt.State(mrt.Args(w, h, 1, 8, 1.0), seed=SEED) as st:
            st.set_world(sc)
            st.set_camera(cam)
            st.redraw()
            assert not st.debug_read_camera_masks(table=False)["in_force"]
            st.redraw()
            st.sync()
            info = st.debug_read_camera_masks(table=False)
        assert info["in_force"] and info["built"] and info["lists"] == lists, (w, h, info)
