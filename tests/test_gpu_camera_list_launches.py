"""The camera-ray sphere lists (myraytracer_amd/csrc/cam_mask.hip; the SC = 3 instantiations of render_kernel) in every form of
launch that can get them, each against the oracle.  tests/test_gpu_camera_list.py pins the table and the plain frame; its images
have no more tiles than launched waves, so every wave renders one tile and leaves.  Here:

  a. every SC = 3 instantiation -- {stream, counter RNG} x {SGPR-fed, matrix-core sweep} x {with, without the draw counter}, main
     and pilot -- by its mrt_debug_last_launch word (bit 6), on 408 tiles and one wave per CU;
  b. three and more tiles per launched wave, the queue in index order and sorted: a wave refills from the queue while some lanes
     are mid-path and others start samples that are resolved in the lane;
  c. counter mode over several 64-sample blocks (queue layers);
  d. the build threshold of a first frame (96 samples per pixel and launch), for a plain frame and an in-lane batch;
  e. frames of 0 samples;
  f. subset frames (mrt_render_tiles): the mixed schedules of tests/test_gpu_adaptive.py with either table forced, and a sorted
     list of two thirds of the tiles at the shape of (b);
  g. the lists and the masks by turns on one built generation, four frames in flight.

Unless a test says otherwise it compares bit for bit with the oracle the framebuffer, samples / world_hit_calls / rng_draws
(rng_draws where the draw counter is on) and the per-pixel costs of the last launch, compares the same with a second context that
runs without tables, and asserts strictly fewer member tests with the lists where depth > 0.  (The cases, _same and the oracle
helpers are the ones of tests/test_gpu_camera_list.py and tests/common.py; that file's _frames and _oracle_trips fix the seed and
16 spp and set neither schedule nor sweep, hence _context and _oracle here.)"""
import math

import numpy as np
import pytest

import adaptive_ref
import camera_list_ref as L
import test_gpu_adaptive as TA
from camera_list_cases import case, scene_of
from common import mismatch_report, oracle_render, to_oracle_camera, to_oracle_spheres
from test_gpu_camera_list import KEYS, _same

pytestmark = pytest.mark.gpu
LISTS_ALWAYS_SPP = 96           # frames.cpp, kCamListAlwaysSpp: a first frame of that many samples per pixel and launch builds


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _wide_shape():
    """256 pixels wide, 32 tiles per row, and so many rows that the image has at least three tiles per CU -- per launched wave
    under mrt_debug_set_schedule(2, 1), one wave per CU: 192 rows and 768 tiles on 256 CUs"""
    return 256, 8 * math.ceil(3 * _cus() / 32)


def _context(mrt, sc, cam, shape, spp, depth, seed, tables, rng_mode=0, schedule=None, sweep=0, count=True, tile_sort=True,
             in_flight=0, batching=None):
    st = mrt.State(mrt.Args(*shape, spp, depth, 1.0), seed=seed)
    try:
        if schedule is not None:
            st.debug_set_schedule(*schedule)
        st.debug_set_camera_masks(tables)
        if sweep:
            st.debug_set_sweep(sweep)
        st.set_world(sc)
        if cam is not None:
            st.set_camera(cam)
        if rng_mode:
            st.set_rng_mode(rng_mode)
        if not count:
            st.set_draw_counting(False)
        if not tile_sort:
            st.debug_set_tile_sort(False)
        if in_flight:
            st.debug_set_frames_in_flight(in_flight)
        if batching is not None:
            st.debug_set_frame_batching(batching)
    except BaseException:
        st.close()
        raise
    return st


def _read(st):
    st.sync()
    return st.read_framebuffer(), st.read_counters(), st.debug_read_pixel_costs()


def _oracle(oracle, sc, cam, shape, spp, depth, seed, frames, rng_mode=0):
    """(framebuffer after `frames` frames, (samples, world_hit_calls, rng_draws), the last frame's per-pixel trips)"""
    cnt = oracle.Counters()
    ref = oracle_render(oracle, sc, cam, *shape, spp, depth, seed, frames=frames, counters=cnt, rng_mode=rng_mode)
    trips = np.zeros(shape[::-1], np.uint32)
    oracle.render_frame(*shape, spp, depth, oracle.pack_world(to_oracle_spheres(oracle, sc)), to_oracle_camera(oracle, cam),
                        oracle.fill_seeds(seed, *shape), oracle.frame_shuffle(seed, frames - 1), rng_mode=rng_mode, trips=trips)
    return ref, (cnt.samples, cnt.world_hit_calls, cnt.rng_draws), trips


def _equals_the_oracle(got, ref, what="", count=True):
    fb, cnt, px = got[:3]
    keys = KEYS if count else KEYS[:2]
    assert np.array_equal(fb.view(np.uint32), ref[0].view(np.uint32)), what + ": " + mismatch_report(fb, ref[0])
    assert tuple(cnt[k] for k in keys) == ref[1][:len(keys)], what
    if not count:
        assert cnt["rng_draws"] == 0, what
    assert np.array_equal(px, ref[2]), f"{what}: the per-pixel costs of {int((px != ref[2]).sum())} pixels differ from the oracle's trips"


def _fewer_member_tests(on, off, depth, what=""):
    if depth:
        assert on[1]["member_tests"] < off[1]["member_tests"], what
    else:
        assert on[1]["member_tests"] == off[1]["member_tests"] == 0, what


# ------------------------------------------------------------------ a. every SC = 3 instantiation

def test_every_list_instantiation_against_the_oracle(mrt, oracle):
    """The shape and schedule of tests/test_gpu_parity.py::test_every_render_kernel_instantiation_against_the_oracle: 408 tiles on
    one wave per CU.  The frame of interest is the SECOND mrt_redraw of a fresh context (frames.cpp): at 16 spp the first frame
    builds no table (16 < 96, no frame survived yet) and runs SC = 0 behind slot 0's pilot; the second lands on slot 1, whose cost
    estimate is still invalid -- a pilot launch again -- after the generation has survived a frame: the table is built and the
    pilot and the main launch both get the lists.  The second frame's queue is sorted by that pilot's costs."""
    shape, spp, depth, seed = (192, 136), 16, 12, 12
    sc, cam = scene_of(mrt, "cover-glass")
    seen_main, seen_pilot = set(), set()
    for ctr in (0, 1):
        ref = _oracle(oracle, sc, cam, shape, spp, depth, seed, 2, ctr)
        for sweep in (1, 2):
            for count in (True, False):
                what = f"ctr={ctr} sweep={sweep} count={count}"
                runs = {}
                for tables in (2, 0):
                    with _context(mrt, sc, cam, shape, spp, depth, seed, tables, ctr, (2, 1), sweep, count) as st:
                        st.redraw()
                        first = st.debug_last_launch()
                        assert not st.debug_read_camera_masks(table=False)["in_force"], what
                        st.redraw()
                        info, (main, pilot) = st.debug_read_camera_masks(table=False), st.debug_last_launch()
                        runs[tables] = _read(st)
                        kind = st.debug_read_tile_schedule()[2]
                    bits = 8 | (4 if ctr else 0) | (16 if sweep == 2 else 0)
                    lists = 64 if tables == 2 else 0
                    assert first == ((1 if count else 0) | bits, 2 | bits), (what, first)         # bit 6 is 0 without a table
                    assert info["in_force"] == info["lists"] == info["built"] == (tables == 2), (what, info)
                    assert main == lists | (1 if count else 0) | bits, (what, main)
                    assert pilot == lists | 2 | bits, (what, pilot)
                    assert kind["kind"] == "sorted" and kind["pilot"] and kind["entries"] == 408, (what, kind)
                    if tables == 2:
                        seen_main.add(main)
                        seen_pilot.add(pilot)
                    _equals_the_oracle(runs[tables], ref, what, count)
                _same(runs[2], runs[0], KEYS if count else KEYS[:2])
                _fewer_member_tests(runs[2], runs[0], depth, what)
    assert len(seen_main) == 8 and len(seen_pilot) == 4, (sorted(seen_main), sorted(seen_pilot))


# ------------------------------------------------------------------ b. several tiles per wave, index order and sorted

@pytest.mark.parametrize("name", ["cover-glass", "default"])
def test_waves_that_take_three_tiles_and_more(mrt, oracle, name):
    """4 spp, no pilot (4 < 8 x the pilot's 2): frames 1 and 2 land on slots without a cost estimate and run in index order, frame
    3 lands on slot 0 again and is sorted by frame 1's costs; frames 2 and 3 run with the lists."""
    shape, spp, depth, seed, frames = _wide_shape(), 4, 8, 5, 3
    sc, cam = scene_of(mrt, name)
    ref = _oracle(oracle, sc, cam, shape, spp, depth, seed, frames)
    runs = {}
    for run, (tables, tile_sort) in {"sorted": (2, True), "index": (2, False), "off": (0, True)}.items():
        with _context(mrt, sc, cam, shape, spp, depth, seed, tables, schedule=(2, 1), tile_sort=tile_sort) as st:
            for _ in range(frames):
                st.redraw()
            info, main = st.debug_read_camera_masks(table=False), st.debug_last_launch()[0]
            runs[run] = _read(st)
            _, order, kind = st.debug_read_tile_schedule()
        n_tiles = shape[0] // 8 * (shape[1] // 8)
        assert kind["entries"] == n_tiles >= 3 * _cus(), (run, kind, _cus())
        assert kind["kind"] == ("sorted" if tile_sort else "index") and not kind["pilot"], (run, kind)
        if tile_sort:
            assert sorted(order) == list(range(n_tiles)) and list(order) != list(range(n_tiles)), run
        assert info["in_force"] == info["lists"] == (tables == 2) and bool(main & 64) == (tables == 2), (run, info, main)
        _equals_the_oracle(runs[run], ref, f"{name} {run}")
    for run in ("sorted", "index"):
        _same(runs[run], runs["off"])
        _fewer_member_tests(runs[run], runs["off"], depth, run)


# ------------------------------------------------------------------ c. counter mode over several blocks

def test_counter_mode_over_three_blocks(mrt, oracle):
    """130 spp in counter mode: blocks of 64, 64 and 2 samples as three layers of the tile queue, which counter mode's `texel`
    allows with the lists (frames.cpp, own_texel); 130 >= 96: the first frame builds and runs with them already"""
    shape, spp, depth, seed = (24, 16), 130, 50, 3
    sc, cam = scene_of(mrt, "cover-glass")
    ref = _oracle(oracle, sc, cam, shape, spp, depth, seed, 2, 1)
    runs = {}
    for tables in (2, 0):
        with _context(mrt, sc, cam, shape, spp, depth, seed, tables, rng_mode=1) as st:
            st.redraw()
            first = st.debug_read_camera_masks(table=False)
            assert first["in_force"] == first["lists"] == first["built"] == (tables == 2), first
            st.redraw()
            info, main = st.debug_read_camera_masks(table=False), st.debug_last_launch()[0]
            runs[tables] = _read(st)
        assert info["in_force"] == info["lists"] == (tables == 2) and main & (64 | 4) == (64 if tables == 2 else 0) | 4, (info, main)
        _equals_the_oracle(runs[tables], ref, f"tables {tables}")
    _same(runs[2], runs[0])
    _fewer_member_tests(runs[2], runs[0], depth)


# ------------------------------------------------------------------ d. the build threshold

@pytest.mark.parametrize("spp", [LISTS_ALWAYS_SPP - 1, LISTS_ALWAYS_SPP])
def test_a_first_frame_builds_from_96_samples_on(mrt, oracle, spp):
    shape, depth, seed = (24, 16), 50, 3
    sc, cam = scene_of(mrt, "cover-glass")
    expect = spp >= LISTS_ALWAYS_SPP
    ref = _oracle(oracle, sc, cam, shape, spp, depth, seed, 1)
    runs = {}
    for tables in (2, 0):
        with _context(mrt, sc, cam, shape, spp, depth, seed, tables) as st:
            st.redraw()
            info, main = st.debug_read_camera_masks(table=False), st.debug_last_launch()[0]
            runs[tables] = _read(st)
        on = expect and tables == 2
        assert info["in_force"] == info["lists"] == info["built"] == on and bool(main & 64) == on, (spp, tables, info, main)
        _equals_the_oracle(runs[tables], ref, f"{spp} spp, tables {tables}")
    _same(runs[2], runs[0])
    if expect:
        _fewer_member_tests(runs[2], runs[0], depth)
    else:
        assert runs[2][1]["member_tests"] == runs[0][1]["member_tests"]


@pytest.mark.parametrize("spp", [31, 32])
def test_a_first_in_lane_batch_builds_from_96_samples_a_lane_on(mrt, oracle, spp):
    """mrt_debug_set_frame_batching(2) and mrt_render(3) on a fresh context: ONE launch (6 tiles are far fewer than two per wave
    the chip holds, so mrt_render wants a batch of as many frames as it is given), in the lane -- samples per frame x frames per
    lane is 96 at 32 spp and 93 at 31.  One launch: frames_done is 3 and the per-pixel costs are those of the batch's last frame."""
    shape, depth, seed = (24, 16), 50, 3
    sc, cam = scene_of(mrt, "cover-glass")
    expect = 3 * spp >= LISTS_ALWAYS_SPP
    ref = _oracle(oracle, sc, cam, shape, spp, depth, seed, 3)
    runs = {}
    for tables in (2, 0):
        with _context(mrt, sc, cam, shape, spp, depth, seed, tables, batching=2) as st:
            st.render(3)
            info, main = st.debug_read_camera_masks(table=False), st.debug_last_launch()[0]
            assert st.frames_done == 3 and len(st.kernel_ms_history()) == 1       # one render launch
            runs[tables] = _read(st)
        on = expect and tables == 2
        assert info["in_force"] == info["lists"] == info["built"] == on and bool(main & 64) == on, (spp, tables, info, main)
        _equals_the_oracle(runs[tables], ref, f"3 x {spp} spp, tables {tables}")
    _same(runs[2], runs[0])
    if expect:
        _fewer_member_tests(runs[2], runs[0], depth)


# ------------------------------------------------------------------ e. nothing to draw

@pytest.mark.parametrize("rng_mode", [0, 1])
def test_frames_of_no_samples(mrt, oracle, rng_mode):
    """0 spp: every frame's mean is 0 / 0 as the reference has it; the second frame builds the table (the generation survived a
    frame) and the launches run with the lists and nothing to resolve"""
    shape, depth, seed = (24, 16), 50, 3
    sc, cam = scene_of(mrt, "cover-glass")
    ref = _oracle(oracle, sc, cam, shape, 0, depth, seed, 3, rng_mode)
    assert ref[1][:2] == (0, 0)
    runs = {}
    for tables in (2, 0):
        with _context(mrt, sc, cam, shape, 0, depth, seed, tables, rng_mode=rng_mode) as st:
            for _ in range(3):
                st.redraw()
            info = st.debug_read_camera_masks(table=False)
            runs[tables] = _read(st)
        assert info["in_force"] == info["lists"] == (tables == 2), (tables, info)
        _equals_the_oracle(runs[tables], ref, f"tables {tables}")
        assert runs[tables][1]["samples"] == runs[tables][1]["world_hit_calls"] == runs[tables][1]["member_tests"] == 0
    _same(runs[2], runs[0])


# ------------------------------------------------------------------ f. subset frames

@pytest.mark.parametrize("tables", [2, 3])
@pytest.mark.parametrize("schedule", ["single", "multi", "pinned-8x2"])
@pytest.mark.parametrize("scene,rng_mode", [("default", 0), ("cover-glass", 0), ("cover", 1), ("default", 1)])
def test_mixed_schedules_with_either_table_forced(mrt, oracle, scene, rng_mode, schedule, tables):
    """tests/test_gpu_adaptive.py::test_mixed_schedules_match_the_oracle_bit_for_bit's body -- framebuffer, S and the per-tile
    frame counts against tests/adaptive_ref.py -- with the lists (2) or the masks (3) forced: a subset launch's tile_order is the
    caller's list or its sorted copy, and `texel >> 3` indexes the table.  Every schedule begins with a whole frame, so every
    render_tiles launch finds a generation that has survived one."""
    seen = []

    def after_tiles(st):
        info = st.debug_read_camera_masks(table=False)
        seen.append((info["in_force"], info["lists"], bool(st.debug_last_launch()[0] & 64)))
    TA.mixed_schedule_matches_the_oracle(mrt, oracle, scene, rng_mode, 1.0, schedule, tables, after_tiles)
    assert len(seen) >= 1 and all(s == (True, tables == 2, tables == 2) for s in seen), seen


def test_a_sorted_list_of_two_thirds_of_the_tiles(mrt, oracle):
    """at the shape of (b): three whole frames, then mrt_render_tiles on a shuffled list of two thirds of the tiles, twice; the
    list has more tiles than the launch has waves and the slot has costs: the queue is the sorted list"""
    shape, spp, depth, seed = _wide_shape(), 4, 8, 5
    W, H = shape
    means = TA.Means(oracle, mrt, "cover-glass", seed, W, H, spp, depth)
    acc = adaptive_ref.Accum(H, W, 1.0)
    tiles = np.random.default_rng(31).permutation(acc.n_tiles)[:2 * acc.n_tiles // 3].astype(np.uint32)
    sc, cam = scene_of(mrt, "cover-glass")
    with _context(mrt, sc, cam, shape, spp, depth, seed, 2, schedule=(2, 1)) as st:
        st.set_noise_tracking(True)
        for _ in range(3):
            st.redraw()
            acc.frame(means[acc.frames_done])
        for _ in range(2):
            st.render_tiles(tiles, 1)
            acc.frame(means[acc.frames_done], tiles)
            info, main = st.debug_read_camera_masks(table=False), st.debug_last_launch()[0]
            assert info["in_force"] and info["lists"] and main & 64, (info, main)
        st.sync()
        _, order, kind = st.debug_read_tile_schedule()
        assert kind["kind"] == "sorted-list" and kind["entries"] == len(tiles) > _cus(), kind
        assert sorted(order) == sorted(tiles) and list(order) != list(tiles)
        assert st.frames_done == acc.frames_done == 5
        assert np.array_equal(st.tile_frames(), acc.tile_frames())
        fb = st.read_framebuffer()
        assert np.array_equal(fb.view(np.uint32), acc.fb.view(np.uint32)), mismatch_report(fb, acc.fb)
        assert np.array_equal(st.read_noise().view(np.uint32), acc.S.view(np.uint32))


# ------------------------------------------------------------------ g. lists and masks on one generation

def test_lists_and_masks_by_turns_on_one_generation(mrt, oracle):
    """four frames in flight, a launch per frame: two frames with the lists, then one frame each with the masks, the lists, no
    table, the lists and the masks once more -- seven frames, the last five queued without a wait; every slot builds for itself
    before its first frame with a table, and every build writes the same words"""
    shape, spp, depth, seed = (24, 16), 16, 50, 3
    c = case(mrt, oracle, "cover-glass", *shape)
    ref = _oracle(oracle, c["sc"], c["cam"], shape, spp, depth, seed, 7)
    with _context(mrt, c["sc"], c["cam"], shape, spp, depth, seed, 2, in_flight=4, batching=0) as st:
        st.redraw()
        assert not st.debug_read_camera_masks(table=False)["in_force"]
        st.redraw()
        info = st.debug_read_camera_masks(table=False)
        assert info["in_force"] and info["lists"] and info["built"]
        words = st.debug_read_camera_lists()
        for tables in (3, 2, 0, 2, 3):
            st.debug_set_camera_masks(tables)
            st.redraw()
            info, main = st.debug_read_camera_masks(table=False), st.debug_last_launch()[0]
            assert (info["in_force"], info["lists"], bool(main & 64)) == (tables != 0, tables == 2, tables == 2), (tables, info, main)
            assert info["built"]
        got = _read(st)
        assert np.array_equal(st.debug_read_camera_lists(), words)
    _equals_the_oracle(got, ref)
    on, over = L.unpack(words, c["n_slots"])
    assert np.array_equal(over, c["lists"].sum(1) > L.CAP) and np.array_equal(on[~over], c["lists"][~over])
