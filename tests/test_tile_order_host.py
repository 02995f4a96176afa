"""tests/tile_order_ref.py judges the GPU's queue orders (tests/test_gpu_tile_order.py); here it is itself put to the test,
without a GPU: a correct numpy sort of every input family passes all three checks, and the orders a subtly wrong sort kernel
would produce are rejected.  No deliberately broken kernel ever runs on a GPU: this is how the GPU tests are known to be able
to fail."""
import numpy as np
import pytest

from tile_order_ref import (N_KEYS, U32_MAX, bucket_edges, check_order, cost_families, cost_of_key, edge_values, key_of,
                            order_violations, tile_max)

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097)
SHARP = ("edges", "log-uniform")          # the families every mutant must be caught on


def sorted_order(cost, members=None, key=key_of):
    """A correct queue: the members by decreasing key (a stable sort, one of the many valid tie orders)."""
    members = np.arange(len(cost)) if members is None else np.asarray(members)
    return members[np.argsort(-key(np.asarray(cost)[members]), kind="stable")]


def three_launch_sort(cost, lane_off_by_one=None):
    """The sort as three steps -- histogram over 1,024 buckets, an exclusive scan from the heaviest bucket down that 64 lanes
    share at 16 buckets each, scatter -- so that a scan fault can be modelled: lane_off_by_one = L makes every lane from L on
    start from the prefix of the lane before it (one lane's 16 buckets are not counted)."""
    keys = key_of(cost)
    hist = np.bincount(keys, minlength=1024)[::-1]                       # heaviest bucket first
    lane_sum = hist.reshape(64, 16).sum(axis=1)
    lane_start = np.concatenate([[0], np.cumsum(lane_sum)[:-1]])
    if lane_off_by_one is not None:
        lane_start[lane_off_by_one:] = np.concatenate([[0], lane_start])[lane_off_by_one:64]
    within = np.cumsum(hist.reshape(64, 16), axis=1) - hist.reshape(64, 16)
    start = (lane_start[:, None] + within).ravel()[::-1]                  # start[key]
    order = np.zeros(len(cost), np.int64)
    nxt = start.copy()
    for i, k in enumerate(keys):
        if nxt[k] < len(order):
            order[nxt[k]] = i
        nxt[k] += 1
    return order


def test_the_key_is_the_documented_one():
    assert [int(k) for k in key_of(np.array([0, 1, 31, 32, 33, 63, 64, 65, 2 ** 31, U32_MAX], np.uint32))] == \
        [0, 1, 31, 32, 33, 63, 64, 64, 27 * 32, 27 * 32 + 31]
    for e in range(5, 32):
        for m in range(32):
            lo, hi = bucket_edges(e, m)
            k = (e - 4) * 32 + m
            assert [int(x) for x in key_of(np.array([lo, hi], np.uint64))] == [k, k] and cost_of_key(k) == lo
            assert int(key_of(np.array([lo - 1], np.uint64))[0]) == k - 1
    assert int(key_of(np.array([U32_MAX], np.uint64))[0]) == N_KEYS - 1
    v = np.sort(np.random.default_rng(1).integers(0, 2 ** 32, 100000, dtype=np.uint64))
    assert (np.diff(key_of(v)) >= 0).all()                               # monotone


def test_the_input_families_are_what_they_claim():
    ev = edge_values()
    assert {0, 1, 30, 31, 32, 33, 63, 64, 65, 2 ** 31, U32_MAX} <= set(int(x) for x in ev)
    assert len(set(int(k) for k in key_of(ev))) >= 27 * 4
    f = cost_families(1000)
    assert set(f) == {"edges", "log-uniform", "below-40", "all-equal", "distinct-per-wave", "ascending", "descending", "alternating"}
    assert all(v.dtype == np.uint32 and len(v) == 1000 for v in f.values())
    assert len(set(key_of(f["all-equal"]))) == 1 and f["below-40"].max() < 40 and len(set(f["alternating"])) == 2
    for w in range(0, 1000, 64):
        k = key_of(f["distinct-per-wave"][w:w + 64])
        assert len(set(int(x) for x in k)) == len(k)
    assert (np.diff(f["ascending"].astype(np.int64)) >= 0).all() and (np.diff(f["descending"].astype(np.int64)) <= 0).all()
    assert int(key_of(f["log-uniform"]).max()) > 800 and int(key_of(f["log-uniform"]).min()) < 100


@pytest.mark.parametrize("n", SIZES)
def test_a_correct_sort_passes_on_every_input(n):
    for name, cost in cost_families(n).items():
        assert order_violations(cost, sorted_order(cost)) == [], name
        assert order_violations(cost, three_launch_sort(cost)) == [], name
        check_order(cost, sorted_order(cost)[::-1] if len(set(key_of(cost))) == 1 else sorted_order(cost))   # ties: any order
        if n >= 3:                                                       # as a subset frame's list
            rng = np.random.default_rng(n)
            for members in (rng.permutation(n), np.arange(0, n, 3), np.array([n // 2])):
                assert order_violations(cost, sorted_order(cost, members), members) == [], name


@pytest.mark.parametrize("n", (257, 1000, 4097))
@pytest.mark.parametrize("family", SHARP + ("below-40",))
def test_a_reversed_order_and_exchanged_neighbour_buckets_fail_the_key_and_the_bound(n, family):
    cost = cost_families(n)[family]
    good = sorted_order(cost)
    assert order_violations(cost, good[::-1]) == ["key", "bound"]
    assert order_violations(cost, sorted_order(cost, key=lambda c: key_of(c) ^ 1)) == ["key", "bound"]


@pytest.mark.parametrize("n", (257, 1000, 4097))
@pytest.mark.parametrize("family", SHARP)
def test_every_other_mutant_order_is_rejected(n, family):
    cost = cost_families(n)[family]
    good = sorted_order(cost)
    dup = good.copy()
    dup[n // 3] = dup[2 * n // 3]                                        # one entry written over another
    assert "permutation" in order_violations(cost, dup)
    lost = good.copy()
    lost[n // 2] = n                                                     # an id that is no tile
    assert "permutation" in order_violations(cost, lost)
    # the scan off by one lane's 16 buckets, at the first lane that has entries before it and entries of its own
    lane_sum = np.bincount(key_of(cost), minlength=1024)[::-1].reshape(64, 16).sum(axis=1)
    lanes = [l for l in range(1, 64) if lane_sum[l - 1] and lane_sum[l:].sum()]
    assert lanes
    assert order_violations(cost, three_launch_sort(cost, lane_off_by_one=lanes[0])) != []
    assert "permutation" in order_violations(cost, three_launch_sort(cost, lane_off_by_one=lanes[len(lanes) // 2]))
    # a list sorted by the cost at the list POSITION instead of the listed tile's
    members = np.random.default_rng(n).permutation(n)
    by_position = members[np.argsort(-key_of(cost[np.arange(n)]), kind="stable")]
    assert set(order_violations(cost, by_position, members)) >= {"key", "bound"}
    part = np.arange(2, n, 3)
    by_position = part[np.argsort(-key_of(cost[np.arange(len(part))]), kind="stable")]
    assert "key" in order_violations(cost, by_position, part)
    # the unlisted tiles' costs leaking in: the list in the whole frame's order is fine, an order holding an unlisted tile is not
    assert order_violations(cost, good[np.isin(good, part)], part) == []
    leak = good[:len(part)]
    assert "permutation" in order_violations(cost, leak, part)


def test_the_bound_alone_catches_what_the_key_would_if_the_buckets_were_others():
    """An order sorted by a coarser key (4 mantissa bits) is not the documented one, and the implementation-independent bound
    says so by itself on the bucket edges; an order sorted by a FINER key (the exact cost) passes everything."""
    cost = cost_families(1000)["edges"]
    coarse = sorted_order(cost, key=lambda c: key_of(c) >> 1)
    assert "bound" in order_violations(cost, coarse)
    assert order_violations(cost, sorted_order(cost, key=lambda c: np.asarray(c).astype(np.int64))) == []


def test_tile_max_on_ragged_edges():
    rng = np.random.default_rng(3)
    w, h = 43, 21
    p = rng.integers(1, 1000, (h, w)).astype(np.uint32)
    t = tile_max(p, w, h)
    assert t.shape == (3 * 6,)
    for ty in range(3):
        for tx in range(6):
            assert t[ty * 6 + tx] == p[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].max()
    assert tile_max(p.ravel(), w, h).tolist() == t.tolist()
    one = np.zeros((8, 8), np.uint32)
    one[7, 7] = 5
    assert tile_max(one, 8, 8).tolist() == [5]
    assert tile_max(np.zeros((16, 9), np.uint32), 9, 16).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("rng_mode,spp", [(0, 16), (1, 16), (1, 192)])
def test_the_oracles_per_pixel_trips_are_its_counters_of_one_pixel_rectangles(mrt, oracle, rng_mode, spp):
    """render_frame's per-pixel trips output (what the GPU's per-pixel and per-tile costs are compared with) against the world_hit_calls of a
    1 x 1 render_frame rectangle per pixel, on the GPU tests' 43 x 21 cover-glass frame."""
    from common import to_oracle_camera, to_oracle_spheres
    w, h, depth, seed = 43, 21, 8, 5
    sc, cam = mrt.scene_cover(1, True)
    packed, ocam = oracle.pack_world(to_oracle_spheres(oracle, sc)), to_oracle_camera(oracle, cam)
    seeds, shuffle = oracle.fill_seeds(seed, w, h), oracle.frame_shuffle(seed, 1)
    trips, total = np.zeros((h, w), np.uint32), oracle.Counters()
    plain = oracle.render_frame(w, h, spp, depth, packed, ocam, seeds, shuffle, rng_mode=rng_mode)
    image = oracle.render_frame(w, h, spp, depth, packed, ocam, seeds, shuffle, rng_mode=rng_mode, counters=total, trips=trips)
    assert np.array_equal(image.view(np.uint32), plain.view(np.uint32))
    assert int(trips.sum()) == total.world_hit_calls and trips.min() >= spp and trips.max() > spp
    for y in range(h):
        for x in range(0, w, 1 if spp == 16 else 6):
            one = oracle.Counters()
            oracle.render_frame(w, h, spp, depth, packed, ocam, seeds, shuffle, rows=(y, y + 1), cols=(x, x + 1), nthreads=1,
                                counters=one, rng_mode=rng_mode)
            assert trips[y, x] == one.world_hit_calls, (x, y)
