"""The wave votes of the small-scene frame kernel (kernels.hip: the votes, masks and counts kept on the scalar side) at the smallest
shapes where each of them is all-false, all-true or mixed within one wave.

Every frame is compared bit for bit with the oracle's, with equal samples / world_hit_calls / rng_draws and equal per-pixel costs:
  * a 1x1 and a 3x2 image (one lane, and a partial wave most of whose lanes never hold a task), an 8x8 image (one full tile) and a
    9x9 image (four tiles, three of them with ragged edges: the refill's vote over pixels inside the image);
  * the cover scene at 1 and 3 samples per pixel and depth 0, 1 and 4: every lane starts a sample at once, no lane traces
    (depth 0), the lanes of a path's last bounce leave the loop together;
  * the shipped 4-sphere scene (its ground sphere direct) and one-sphere scenes (no direct sphere; with the sphere behind the
    camera no list has a slot and no lane ever hits);
  * the camera-ray lists forced (mrt_debug_set_camera_masks(2)), the masks forced (3) and both off; the stream RNG, and once the
    counter RNG;
  * an accumulation of three frames and one mrt_render batch in both batch forms (a lane keeps its pixel for the batch's frames /
    the frames as queue layers): what a lane holds per pixel has to survive its move to the next frame of a batch and be replaced
    when it takes a new pixel.

The lists and the masks are in force from a setting's second frame on (frames.cpp, camera_masks), so every case renders three."""
import functools

import numpy as np
import pytest

from common import mismatch_report, oracle_render, to_oracle_camera, to_oracle_spheres

pytestmark = pytest.mark.gpu
KEYS = ("samples", "world_hit_calls", "rng_draws")
SEED, FRAMES = 5, 3
MODES = {"lists": 2, "masks": 3, "off": 0}


@functools.lru_cache(maxsize=None)
def _scene(mrt, name):
    """(spheres, Camera or None)"""
    if name == "cover-glass":
        return mrt.scene_cover(1, True)
    sc = mrt.scene_default()
    if name == "default":
        return sc, None
    one = sc[1:2].copy()                                # the sphere straight ahead of the pinhole, radius 0.5
    if name == "one-behind":
        one["center"][0] = (0.0, 0.0, 3.0)              # behind the camera: no ray of the image can touch it
    return one, None


@functools.lru_cache(maxsize=None)
def _reference(oracle, mrt, name, W, H, spp, depth, frames, rng_mode):
    """(framebuffer after `frames` frames, (samples, world_hit_calls, rng_draws) of all frames, the last frame's per-pixel trips)"""
    sc, cam = _scene(mrt, name)
    cnt = oracle.Counters()
    ref = oracle_render(oracle, sc, cam, W, H, spp, depth, SEED, frames=frames, counters=cnt, rng_mode=rng_mode)
    trips = np.zeros((H, W), np.uint32)
    oracle.render_frame(W, H, spp, depth, oracle.pack_world(to_oracle_spheres(oracle, sc)), to_oracle_camera(oracle, cam),
                        oracle.fill_seeds(SEED, W, H), oracle.frame_shuffle(SEED, frames - 1), rng_mode=rng_mode, trips=trips)
    ref.setflags(write=False)
    trips.setflags(write=False)
    return ref, (cnt.samples, cnt.world_hit_calls, cnt.rng_draws), trips


def _render(mrt, name, W, H, spp, depth, mode, frames=FRAMES, rng_mode=0, batch_form=0):
    """(framebuffer, counters, per-pixel costs of the last launch, table info)"""
    sc, cam = _scene(mrt, name)
    with mrt.State(mrt.Args(W, H, spp, depth, 1.0), seed=SEED) as st:
        st.debug_set_camera_masks(mode)
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
        return st.read_framebuffer(), st.read_counters(), st.debug_read_pixel_costs(), st.debug_read_camera_masks(table=False)


def _check(mrt, oracle, name, W, H, spp, depth, mode, rng_mode=0):
    ref, counts, trips = _reference(oracle, mrt, name, W, H, spp, depth, FRAMES, rng_mode)
    fb, cnt, px, info = _render(mrt, name, W, H, spp, depth, MODES[mode], rng_mode=rng_mode)
    assert info["in_force"] == (mode != "off") and info["lists"] == (mode == "lists"), info
    assert np.array_equal(fb.view(np.uint32), ref.view(np.uint32)), mismatch_report(fb, ref)
    assert tuple(cnt[k] for k in KEYS) == counts
    assert np.array_equal(px, trips)
    assert cnt["world_hit_calls"] <= cnt["lane_slots"]
    return cnt


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (8, 8), (9, 9)])
def test_single_pixel_partial_wave_one_tile_and_ragged_images(mrt, oracle, shape, mode):
    _check(mrt, oracle, "cover-glass", *shape, 3, 4, mode)


@pytest.mark.parametrize("mode", ["lists", "off"])
@pytest.mark.parametrize("depth", [0, 1, 4])
@pytest.mark.parametrize("spp", [1, 3])
def test_vote_extremes_on_the_cover_scene(mrt, oracle, spp, depth, mode):
    cnt = _check(mrt, oracle, "cover-glass", 9, 9, spp, depth, mode)
    assert cnt["samples"] == FRAMES * 81 * spp
    if depth == 0:
        assert cnt["world_hit_calls"] == cnt["member_tests"] == 0         # no lane ever traces


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["default", "one", "one-behind"])
def test_direct_sphere_and_list_extremes(mrt, oracle, name, mode):
    cnt = _check(mrt, oracle, name, 9, 9, 3, 4, mode)
    if name == "one-behind":
        assert cnt["world_hit_calls"] == cnt["samples"]                   # every camera ray misses: one call per sample


def test_the_counter_rng_with_the_lists(mrt, oracle):
    _check(mrt, oracle, "cover-glass", 9, 9, 3, 4, "lists", rng_mode=1)


@pytest.mark.parametrize("batch_form", [2, 3])
def test_an_accumulation_and_one_batch_of_either_form(mrt, oracle, batch_form):
    """three frames one by one (in _check), then one frame and ONE mrt_render of three more: form 2 runs with the lists and its lanes
    move from frame to frame of their pixel, form 3 queues the frames as layers and runs without"""
    _check(mrt, oracle, "cover-glass", 9, 9, 3, 4, "lists")
    ref, counts, _ = _reference(oracle, mrt, "cover-glass", 9, 9, 3, 4, 4, 0)
    on = _render(mrt, "cover-glass", 9, 9, 3, 4, MODES["lists"], frames=4, batch_form=batch_form)
    off = _render(mrt, "cover-glass", 9, 9, 3, 4, MODES["off"], frames=4, batch_form=batch_form)
    assert on[3]["in_force"] == on[3]["lists"] == (batch_form == 2) and not off[3]["in_force"]
    for fb, cnt, px, _ in (on, off):
        assert np.array_equal(fb.view(np.uint32), ref.view(np.uint32)), mismatch_report(fb, ref)
        assert tuple(cnt[k] for k in KEYS) == counts
    assert np.array_equal(on[2], off[2])
