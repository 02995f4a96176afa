"""The scheduling state behind "persistent waves on a heaviest-first tile queue", which never reaches a pixel and which no image
test can therefore see: every tile's cost (the largest number of bounce-loop trips of its pixels, written by the finalize and
per-tile blend kernels and, before a slot's first frame, by the pilot launch), the three-launch bucket sort of csrc/tile_order.hip
(whole frame and a subset frame's list), and frames.cpp's choice of the cost array that orders a frame.

Read through two diagnostics -- mrt_debug_sort_tiles (the sort on caller-supplied costs) and mrt_debug_read_tile_schedule (a
slot's costs, the order its last launch was given and how it came about) -- and judged by tests/tile_order_ref.py, a plain
numpy statement of "heaviest first" that tests/test_tile_order_host.py shows to reject the orders of subtly wrong kernels.
Costs are compared with the pixels' own counts and, per pixel, with the CPU oracle's world_hit calls."""
import functools

import numpy as np
import pytest

from common import to_oracle_camera, to_oracle_spheres
from tile_order_ref import check_order, cost_families, order_violations, tile_max

pytestmark = pytest.mark.gpu

SEED, DEPTH, SPP, PILOT_SPP = 5, 8, 16, 2
MRT_ERR_INVALID_ARG, MRT_ERR_NO_SCENE = 1, 4


# ---- helpers

class _Ctx:
    """A State that must still be sound (mrt_debug_check_context) when the test is done with it."""

    def __init__(self, mrt, w, h, spp=SPP, scene="cover-glass", camera="own", shard=None, schedule=None):
        self.st = mrt.State(mrt.Args(w, h, spp, DEPTH, 1.0), seed=SEED, shard=shard)
        if schedule is not None:
            self.st.debug_set_schedule(*schedule)                        # (pilot spp, waves per CU: before anything is rendered)
        sc, cam = _scene(scene, camera)
        self.st.set_world(sc)
        if cam is not None:
            self.st.set_camera(cam)

    def __enter__(self):
        return self.st

    def __exit__(self, exc_type, *exc):
        try:
            if exc_type is None:
                why = self.st.debug_check_context()
                assert why is None, why
        finally:
            self.st.close()


def _scene(name, camera="own"):
    """(spheres, camera): the scene `name` seen through its own camera, through the cover-glass scene's ("cover") or through
    another look-at camera ("other")."""
    import myraytracer_amd as mrt
    glass, glass_cam = mrt.scene_cover(1, True)
    if name == "default":
        sc, cam = mrt.scene_default(), None
    else:
        sc, cam = mrt.scene_cover(1, name == "cover-glass")
    if camera == "cover":
        cam = glass_cam
    if camera == "other":                        # from the other side and from above: other tiles see the glass and the sky
        cam = mrt.Camera(1, (-4.0, 9.0, -11.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0, 0.0, 10.0)
    return sc, cam


@functools.lru_cache(maxsize=None)
def _oracle_trips(scene, camera, w, h, spp, frame, rng_mode=0):
    """(h, w) u32: the oracle's world_hit calls of every pixel (= bounce-loop trips, ray_depth > 0) in a frame of spp samples
    with frame `frame`'s shuffle (tests/test_tile_order_host.py holds them against the counters of 1 x 1 rectangles)."""
    from oracle import pyoracle as O
    sc, cam = _scene(scene, camera)
    trips = np.zeros((h, w), np.uint32)
    O.render_frame(w, h, spp, DEPTH, O.pack_world(to_oracle_spheres(O, sc)), to_oracle_camera(O, cam), O.fill_seeds(SEED, w, h),
                   O.frame_shuffle(SEED, frame), rng_mode=rng_mode, trips=trips)
    trips.setflags(write=False)
    return trips


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _narrow_shape(more_tiles_than_waves=True):
    """With one persistent wave per CU (mrt_debug_set_schedule(pilot, 1)) a launch has as many waves as the chip has CUs: the
    smallest image of 22 tile columns with more tiles than that (176 x 96 = 264 tiles on 256 CUs; + 3, so that a list can be
    longer than the launch and still not the whole image) -- or a strip of exactly as many tiles as waves."""
    if not more_tiles_than_waves:
        return 8 * _cus(), 8
    return 176, 8 * ((_cus() + 3) // 22 + 1)


def _narrow(mrt, w, h, spp=SPP, slots=None, pilot_spp=PILOT_SPP, **kw):
    ctx = _Ctx(mrt, w, h, spp, schedule=(pilot_spp, 1), **kw)
    if slots is not None:
        ctx.st.debug_set_frames_in_flight(slots)
    return ctx


def _frame(st):
    st.redraw()
    return st.debug_read_tile_schedule()


# ---- a. the sort kernels on synthetic costs

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_whole_frame_sort_on_every_input_family(mrt, n):
    """n crosses the wave (64) and workgroup (256) boundaries of the hist / scatter launches and, at 4097, holds more entries
    than there are buckets; an image 8 n wide and 8 high has n tiles."""
    with _Ctx(mrt, 8 * n, 8, 1, scene="default") as st:
        for name, cost in cost_families(n).items():
            order = st.debug_sort_tiles(cost)
            assert order_violations(cost, order) == [], f"{name}, n = {n}"
        _, order, info = st.debug_read_tile_schedule()
        assert info["kind"] == "none" and len(order) == 0                # (the staging left no frame's order behind)


def test_list_sort_on_every_input_family(mrt):
    n = 1000
    rng = np.random.default_rng(7)
    with _Ctx(mrt, 8 * n, 8, 1, scene="default") as st:
        for name, cost in cost_families(n).items():
            by_cost = np.argsort(cost, kind="stable")
            lists = {"one": np.array([n // 2]), "permuted": rng.permutation(n), "every-third": np.arange(1, n, 3),
                     "ascending-cost": by_cost[::2], "descending-cost": by_cost[::-2], "short-permuted": rng.permutation(n)[:257]}
            for lname, members in lists.items():
                order = st.debug_sort_tiles(cost, members)
                assert order_violations(cost, order, members) == [], f"{name}, list {lname}"
        # the listed tiles all in ONE bucket (in list order nothing tells them apart), every unlisted tile heavier: an unlisted
        # cost that leaked into the histogram or the scan would move the listed ones past the end or onto each other
        members = rng.permutation(n)[:300]
        cost = np.full(n, 50000, np.uint32)
        cost[members] = 1000
        order = st.debug_sort_tiles(cost, members)
        check_order(cost, order, members)
        # ... and lighter ones; then listed tiles in two buckets between them
        cost = np.full(n, 3, np.uint32)
        cost[members] = rng.choice([1000, 2000], len(members)).astype(np.uint32)
        check_order(cost, st.debug_sort_tiles(cost, members), members)


def test_sort_diagnostic_refusals_and_a_real_frame_afterwards(mrt):
    """No scene: MRT_ERR_NO_SCENE, as the frame calls; sizes beyond the context's tiles, a list entry that is no tile: refused.
    The caller's costs never order a real frame: the next one runs a pilot of its own (or, too short for one, index order)."""
    w, h = _narrow_shape()
    n = (w // 8) * (h // 8)
    st = mrt.State(mrt.Args(w, h, SPP, DEPTH, 1.0), seed=SEED)
    try:
        for call in (lambda: st.debug_sort_tiles(np.arange(4)), st.debug_read_tile_schedule):
            with pytest.raises(mrt.MrtError) as e:
                call()
            assert e.value.status == MRT_ERR_NO_SCENE
        assert st.debug_check_context() is None
    finally:
        st.close()
    with _narrow(mrt, w, h, slots=1) as st:
        for bad in (lambda: st.debug_sort_tiles(np.arange(n + 1)), lambda: st.debug_sort_tiles(np.arange(8), [8]),
                    lambda: st.debug_sort_tiles(np.arange(8), np.arange(9)), lambda: st.debug_sort_tiles(np.zeros(0))):
            with pytest.raises(mrt.MrtError) as e:
                bad()
            assert e.value.status == MRT_ERR_INVALID_ARG
        _frame(st)
        cost1, order1, info1 = _frame(st)
        assert (info1["kind"], info1["pilot"]) == ("sorted", False)
        junk = np.arange(n, dtype=np.uint32)                             # ascending: the last tile first
        junk_order = st.debug_sort_tiles(junk)
        check_order(junk, junk_order)
        _, order, info = _frame(st)
        assert (info["kind"], info["entries"], info["pilot"]) == ("sorted", n, True)
        pilot = tile_max(_oracle_trips("cover-glass", "own", w, h, PILOT_SPP, 2), w, h)
        check_order(pilot, order)
        assert order_violations(pilot, junk_order) != []                 # (the caller's costs would not have passed)


# ---- b. costs from real frames

W, H = 43, 21                      # 6 x 3 tiles, ragged right and top


def _check_costs(st, trips, what):
    px = st.debug_read_pixel_costs()
    cost, _, _ = st.debug_read_tile_schedule()
    assert px.shape == (H, W) and cost.shape == (18,)
    assert np.array_equal(cost, tile_max(px, W, H)), what
    if trips is not None:
        assert np.array_equal(px, trips), what                           # per pixel, the oracle's world_hit calls
        assert np.array_equal(cost, tile_max(trips, W, H)), what


@pytest.mark.parametrize("route", ["stream", "counter-16", "counter-192", "tracked"])
def test_tile_cost_is_the_heaviest_pixel_of_the_tile(mrt, route):
    spp = 192 if route == "counter-192" else SPP                         # three blocks of 64: summed per pixel, then the maximum
    mode = 1 if route.startswith("counter") else 0
    with _Ctx(mrt, W, H, spp) as st:
        if mode:
            st.set_rng_mode(1)
        if route == "tracked":
            st.set_noise_tracking(True)                                  # finalize_tracked_kernel
        for frame in range(2):
            st.redraw()
            _check_costs(st, _oracle_trips("cover-glass", "own", W, H, spp, frame, mode), f"{route}, frame {frame}")
        assert int(_oracle_trips("cover-glass", "own", W, H, spp, 1, mode).max()) > spp      # (not all sky)


@pytest.mark.parametrize("form", [2, 3])
def test_a_batchs_tile_costs_are_its_last_frames(mrt, form):
    with _Ctx(mrt, W, H) as st:
        st.debug_set_frame_batching(form)
        st.render(3)
        assert len(st.kernel_ms_history(8)) == 1                         # one launch
        _check_costs(st, _oracle_trips("cover-glass", "own", W, H, SPP, 2), f"batch form {form}")
        assert not np.array_equal(_oracle_trips("cover-glass", "own", W, H, SPP, 2), _oracle_trips("cover-glass", "own", W, H, SPP, 0))


@pytest.mark.parametrize("rank", [0, 1])
def test_a_shards_tile_costs_are_those_of_its_own_bands(mrt, rank):
    """43 x 52: 7 bands, the top one 4 rows high, dealt to 3 ranks of 3 local bands each.  Rank 0 owns the partial top band
    (its third); rank 1's third band is padding beyond the image, whose tiles must cost 0."""
    w, h, world = 43, 52, 3
    full = _oracle_trips("cover-glass", "own", w, h, SPP, 0)
    with _Ctx(mrt, w, h, shard=(rank, world)) as st:
        st.redraw()
        px = st.debug_read_pixel_costs()
        cost, order, info = st.debug_read_tile_schedule()
    assert px.shape == (24, w) and cost.shape == (18,) and info["entries"] == 18
    expect = np.zeros((24, w), np.uint32)
    for lrow in range(24):
        y = mrt.shard_global_row(lrow, rank, world)
        if y < h:
            expect[lrow] = full[y]
            assert np.array_equal(px[lrow], full[y]), f"rank {rank}: local row {lrow} = global row {y}"
    assert np.array_equal(cost, tile_max(expect, w, 24))
    if rank == 0:
        assert np.array_equal(cost[12:], tile_max(full[48:52], w, 4)) and cost[12:].min() > 0
    else:
        assert not cost[12:].any() and cost[:12].min() > 0


def test_a_subset_frame_costs_its_listed_tiles_and_leaves_the_others(mrt):
    listed = np.array([16, 0, 5, 11, 7], np.uint32)
    with _Ctx(mrt, W, H) as st:
        st.debug_set_frames_in_flight(1)
        st.redraw()
        before, _, _ = st.debug_read_tile_schedule()
        assert np.array_equal(before, tile_max(_oracle_trips("cover-glass", "own", W, H, SPP, 0), W, H))
        st.render_tiles(listed, 1)
        px = st.debug_read_pixel_costs()
        after, order, info = st.debug_read_tile_schedule()
    assert (info["kind"], info["entries"], info["pilot"]) == ("list", 5, False) and np.array_equal(order, listed)
    new = tile_max(_oracle_trips("cover-glass", "own", W, H, SPP, 1), W, H)
    unlisted = np.setdiff1d(np.arange(18), listed)
    assert np.array_equal(after[listed], tile_max(px, W, H)[listed]) and np.array_equal(after[listed], new[listed])
    assert np.array_equal(after[unlisted], before[unlisted])
    assert not np.array_equal(new[listed], before[listed])               # (the subset frame did change what it touched)


# ---- c. which costs order which frame

def test_one_frame_in_flight_orders_by_the_previous_frames_costs(mrt):
    w, h = _narrow_shape()
    n = (w // 8) * (h // 8)
    with _narrow(mrt, w, h, slots=1) as st:
        cost, order, info = _frame(st)
        assert (info["kind"], info["entries"], info["pilot"]) == ("sorted", n, True), "the smallest shape with more tiles than waves"
        check_order(tile_max(_oracle_trips("cover-glass", "own", w, h, PILOT_SPP, 0), w, h), order)
        assert st.debug_last_launch()[1] is not None
        for k in range(1, 4):
            prev = cost
            assert np.array_equal(prev, tile_max(_oracle_trips("cover-glass", "own", w, h, SPP, k - 1), w, h))
            cost, order, info = _frame(st)
            assert (info["kind"], info["entries"], info["pilot"], info["slot"]) == ("sorted", n, False, 0)
            check_order(prev, order)
            assert order_violations(cost, order) != []                   # (by the frame before, not by its own costs)


def test_two_frames_in_flight_order_by_the_same_slots_frame_two_earlier(mrt):
    w, h = _narrow_shape()
    n = (w // 8) * (h // 8)
    with _narrow(mrt, w, h) as st:
        seen = []
        for k in range(6):
            cost, order, info = _frame(st)
            assert (info["kind"], info["entries"], info["slot"]) == ("sorted", n, k % 2)
            assert info["pilot"] == (k < 2)                              # each slot's first frame
            if k < 2:
                check_order(tile_max(_oracle_trips("cover-glass", "own", w, h, PILOT_SPP, k), w, h), order)
            else:
                check_order(seen[k - 2], order)
                assert order_violations(seen[k - 1], order) != []        # (not by the other slot's, one frame earlier)
            assert np.array_equal(cost, tile_max(_oracle_trips("cover-glass", "own", w, h, SPP, k), w, h))
            seen.append(cost)


@pytest.mark.parametrize("change", ["world", "camera"])
def test_a_new_scene_or_camera_gets_a_fresh_pilot(mrt, change):
    w, h = _narrow_shape()
    with _narrow(mrt, w, h, slots=1) as st:
        _frame(st)
        _, old_order, info = _frame(st)
        assert (info["kind"], info["pilot"]) == ("sorted", False)
        if change == "world":                                            # the scene alone: the camera stays, and set_camera
            st.set_world(_scene("default")[0])                           # (which invalidates the estimate by itself) is not called
            new = ("default", "cover")
        else:
            st.set_camera(_scene("cover-glass", "other")[1])
            new = ("cover-glass", "other")
        assert st.frames_done == 2
        cost, order, info = _frame(st)
        assert (info["kind"], info["pilot"]) == ("sorted", True)
        pilot = tile_max(_oracle_trips(*new, w, h, PILOT_SPP, 2), w, h)
        check_order(pilot, order)
        assert order_violations(pilot, old_order) != []                  # the stale estimate's order would not have passed
        assert np.array_equal(cost, tile_max(_oracle_trips(*new, w, h, SPP, 2), w, h))
        prev = cost
        _, order, info = _frame(st)
        assert (info["kind"], info["pilot"]) == ("sorted", False)
        check_order(prev, order)


@pytest.mark.parametrize("case", ["sort-off", "no-more-tiles-than-waves", "short-chains", "too-short-for-a-pilot"])
def test_frames_that_are_not_sorted_run_in_index_order(mrt, case):
    w, h = _narrow_shape(case != "no-more-tiles-than-waves")
    n = (w // 8) * (h // 8)
    spp = {"short-chains": 3, "too-short-for-a-pilot": 8 * PILOT_SPP - 1}.get(case, SPP)
    with _narrow(mrt, w, h, spp, slots=1) as st:
        if case == "sort-off":
            st.debug_set_tile_sort(False)
        frames = 1 if case == "too-short-for-a-pilot" else 3
        for k in range(frames):
            cost, order, info = _frame(st)
            assert (info["kind"], info["entries"], info["pilot"]) == ("index", n, False), f"frame {k}"
            assert np.array_equal(order, np.arange(n))
            assert st.debug_last_launch()[1] is None
        if case == "too-short-for-a-pilot":                              # ... but its costs order the slot's next frame
            assert np.array_equal(cost, tile_max(_oracle_trips("cover-glass", "own", w, h, spp, 0), w, h))
            _, order, info = _frame(st)
            assert (info["kind"], info["pilot"]) == ("sorted", False)
            check_order(cost, order)


def test_one_tile_more_than_waves_is_where_the_sort_starts(mrt):
    """A strip of exactly as many tiles as waves is the last unsorted shape (the index-order test above); one tile more is
    the smallest image whose frames are sorted."""
    n = _cus() + 1
    w, h = 8 * n, 8
    with _narrow(mrt, w, h, slots=1) as st:
        cost, order, info = _frame(st)
        assert (info["kind"], info["entries"], info["pilot"]) == ("sorted", n, True)
        check_order(tile_max(_oracle_trips("cover-glass", "own", w, h, PILOT_SPP, 0), w, h), order)
        _, order, info = _frame(st)
        assert (info["kind"], info["pilot"]) == ("sorted", False)
        check_order(cost, order)


def test_a_subset_frames_list_is_sorted_by_the_slots_costs(mrt):
    w, h = _narrow_shape()
    n = (w // 8) * (h // 8)
    rng = np.random.default_rng(11)
    long_list = rng.permutation(n)[:_cus() + 1].astype(np.uint32)        # one tile longer than the launch is wide
    short_list = rng.permutation(n)[:_cus()].astype(np.uint32)           # ... and exactly as long: no sort
    assert n > len(long_list) > _cus() >= len(short_list)
    with _narrow(mrt, w, h, slots=1) as st:
        before, _, _ = _frame(st)
        st.render_tiles(long_list, 1)
        after, order, info = st.debug_read_tile_schedule()
        assert (info["kind"], info["entries"], info["pilot"]) == ("sorted-list", _cus() + 1, False)
        check_order(before, order, long_list)
        assert order_violations(before, long_list, long_list) != []      # (the list as given would not have passed)
        unlisted = np.setdiff1d(np.arange(n), long_list)
        assert np.array_equal(after[unlisted], before[unlisted])
        assert np.array_equal(after[long_list], tile_max(_oracle_trips("cover-glass", "own", w, h, SPP, 1), w, h)[long_list])
        st.render_tiles(short_list, 1)
        _, order, info = st.debug_read_tile_schedule()
        assert (info["kind"], info["entries"]) == ("list", _cus()) and np.array_equal(order, short_list)


# ---- d. the utilisation counter

@pytest.mark.parametrize("w,h", [(W, H), (8, 8)])
def test_lane_slots_counts_whole_waves_and_covers_the_work(mrt, w, h):
    """lane_slots (64 per bounce-loop trip of a wave) feeds the launch-width controller.  No upper bound: it depends on the
    schedule."""
    with _Ctx(mrt, w, h) as st:
        st.redraw()
        c, px = st.read_counters(), st.debug_read_pixel_costs()
    assert c["lane_slots"] % 64 == 0 and c["lane_slots"] >= c["world_hit_calls"] == int(px.sum()) > 0
    assert c["world_hit_calls"] == int(_oracle_trips("cover-glass", "own", w, h, SPP, 0).sum())
    if (w, h) == (8, 8):                                                  # one tile, one wave: it runs as long as its longest pixel
        assert c["lane_slots"] >= 64 * int(px.max())
