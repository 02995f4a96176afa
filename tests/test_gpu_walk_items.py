"""The small-scene walk derives its (owner, cluster) items cooperatively from the sweep masks (kernels.hip, "Small scenes";
the derivation is restated in tests/test_walk_items_host.py): the shapes at which that can go wrong, through
mrt_debug_world_hit -- the render kernel instantiated to take its rays from an array, 64 consecutive rays = the lanes of one
wave, in order.  Per case the winners equal the oracle's world_hit bit for bit and the (ray, sphere) pairs that reached the
root tests contain every sphere with discriminant >= 0 not behind the origin and only spheres with discriminant >= 0
(test_gpu_superset._check).

The scenes put clusters where a ray's item count is known: groups of four small spheres 10 units apart, or a straight row of
1,000 spheres = 250 clusters that one ray threads.  Neither is taken on trust: the builder's clusters are read back on the host
(mrt_debug_build_hierarchy: every group one cluster, and which mask word -- 32 top records -- it landed in), and the number of
items the walk really ran comes from the launch's own member-test counter (mrt_debug_world_hit_stats: 4 per cluster item;
these scenes have no direct spheres), so a case that no longer produces its item count, or its pattern of words, fails."""
import numpy as np
import pytest

from common import mismatch_report, oracle_render, to_oracle_spheres
from test_gpu_superset import _check, _random_scene, _rays_for
from test_hierarchy_host import build

pytestmark = pytest.mark.gpu
SWEEPS = pytest.mark.parametrize("sweep", [1, 2], ids=["valu-sweep", "matrix-core-sweep"])


def _groups_at(mrt, centre):
    """groups of four spheres of radius 0.05 around the given centres: group g = spheres 4 g .. 4 g + 3"""
    centre = np.asarray(centre, np.float32)
    sc = np.zeros(4 * len(centre), mrt.SPHERE_DTYPE)
    off = np.array([[0.1, 0, 0], [-0.1, 0, 0], [0, 0, 0.1], [0, 0, -0.1]], np.float32)
    sc["center"] = (centre[:, None, :] + off[None]).reshape(-1, 3)
    sc["radius"] = 0.05
    sc["material_ty"] = 1
    sc["albedo"] = 0.5
    return sc


def _groups(mrt, nx, nz):
    """nx x nz groups around (10 i, 0, 10 k); group k nx + i"""
    return _groups_at(mrt, [[10.0 * i, 0.0, 10.0 * k] for k in range(nz) for i in range(nx)])


def _records(mrt, sc):
    """group -> top record (= cluster) of a groups scene, from the host's build: every group is exactly one cluster, nothing is
    tested directly, one level"""
    h = build(mrt, sc)
    assert h["levels"] == 1 and h["n_direct"] == 0
    never = np.isinf(h["nodes"][:h["n_members"], 3]).reshape(-1, 4)
    rec = {}
    for c, (m, nv) in enumerate(zip(h["midx"].reshape(-1, 4), never)):
        if nv.all():
            continue
        assert not nv.any() and len(set((m // 4).tolist())) == 1, f"cluster {c} holds spheres {m.tolist()}: not one group"
        rec[int(m[0]) // 4] = c
    assert len(rec) == len(sc) // 4
    return rec


def _items(mrt, oracle, sc, rays, sweep, what):
    """_check's comparisons, then the number of cluster items the walk ran for these rays (whole waves: no padding rays)"""
    assert len(rays) % 64 == 0 and build(mrt, sc)["n_direct"] == 0
    variant, pairs, _ = _check(mrt, oracle, sc, rays, sweep=sweep, what=what)
    assert variant == sweep
    with mrt.State(mrt.Args(16, 16), seed=1) as st:
        st.set_world(sc)
        st.debug_set_sweep(sweep)
        st.debug_world_hit(rays, len(sc))
        traced, member_tests = st.debug_world_hit_stats()
    assert traced == len(rays) and member_tests % 4 == 0
    return member_tests // 4, pairs


def _lane_rays(kinds):
    """one ray per lane j over the groups scene: 'none' points away from everything, 'one' drops through one sphere of group (j, 0), 'two' runs
    along z through the groups (j, 0) and (j, 1); axis-parallel directions, so exactly unit length"""
    rays = np.zeros((len(kinds), 6), np.float32)
    for j, kind in enumerate(kinds):
        x = 10.0 * (j % 64)
        rays[j] = dict(none=(x + 5.0, 50.0, 0.0, 0, 1, 0), one=(x + 0.1, 5.0, 0.0, 0, -1, 0), two=(x, 0.0, -5.0, 0, 0, 1))[kind]
    return rays


BOUNDARY = {
    "total-0": ["none"] * 64,
    "total-1": ["none"] * 17 + ["one"] + ["none"] * 46,
    "total-63": ["one"] * 63 + ["none"],
    "total-64": ["one"] * 64,
    "total-65-last-lane-straddles": ["one"] * 63 + ["two"],
    "total-128": ["two"] * 64,
    "straddle-then-a-new-owner": ["two"] * 31 + ["one", "two"] + ["none"] * 17 + ["one"] + ["none"] * 13,
}


@SWEEPS
@pytest.mark.parametrize("name", list(BOUNDARY))
def test_item_counts_around_a_round(mrt, oracle, name, sweep):
    """total_rem = 0, 1, 63, 64, 65, 128 by how many of a wave's 64 rays aim at isolated clusters, and intervals that straddle
    the 64/65 boundary: the carry into position 0 of the second round"""
    sc, kinds = _groups(mrt, 64, 2), BOUNDARY[name]
    _records(mrt, sc)
    rays = _lane_rays(kinds)
    items, pairs = _items(mrt, oracle, sc, rays, sweep, name)
    # the wave's total_rem: one item per group a lane's ray threads, no neighbouring bound admitted
    assert items == sum(dict(none=0, one=1, two=2)[k] for k in kinds)
    # 'one' passes one sphere; 'two' the two spheres on its axis in each of its two groups
    assert pairs == sum(dict(none=0, one=1, two=4)[k] for k in kinds)


def _row(mrt, n=1000):
    sc = np.zeros(n, mrt.SPHERE_DTYPE)
    sc["center"][:, 0] = 0.5 * np.arange(n, dtype=np.float32)
    sc["radius"] = 0.1
    sc["material_ty"] = 1
    sc["albedo"] = 0.5
    return sc


@SWEEPS
@pytest.mark.parametrize("along", [(20,), (20, 45), (0, 63)], ids=["one-owner-250", "two-owners-500", "first-and-last-lane"])
def test_one_lane_holds_many_items(mrt, oracle, along, sweep):
    """A row of 250 clusters (8 full mask words) and rays along it: an owner with more than 64 items, spanning rounds and -- with
    two such owners -- windows of the table, between lanes that own nothing; every word full: ranks 0 .. 31 within a word"""
    sc = _row(mrt)
    rays = np.zeros((64, 6), np.float32)
    rays[:] = (0.0, 40.0, 7.0, 0, 1, 0)
    rays[:, 0] = 3.0 + 5.0 * np.arange(64)
    for lane in along:
        rays[lane] = (-5.0 - lane, 0.0, 0.0, 1, 0, 0)
    assert len(build(mrt, sc)["top"]) == 256
    items, pairs = _items(mrt, oracle, sc, rays, sweep, f"row, lanes {along}")
    assert items == 250 * len(along) and pairs == 1000 * len(along)


@SWEEPS
def test_rays_across_the_row_and_columns_of_groups(mrt, oracle, sweep):
    """Few items per lane: rays across the row (at most a cluster or two each, every part of the row); rays along the columns of
    a 32 x 8 grid of groups -- the 8 clusters of a column lie in ONE mask word, the lane's other seven words are empty -- and
    along its rows: 4 clusters in each of the 8 words"""
    row = _row(mrt)
    rays = np.zeros((128, 6), np.float32)
    rays[:] = (0, 3.0, 0, 0, -1, 0)
    rays[:, 0] = np.linspace(0.0, 499.5, 128).astype(np.float32)
    _check(mrt, oracle, row, rays, sweep=sweep, what="across the row")
    grid = _groups(mrt, 32, 8)
    rec = _records(mrt, grid)
    for i in range(32):
        assert len({rec[k * 32 + i] // 32 for k in range(8)}) == 1, f"column {i} is spread over several mask words"
    for k in range(8):
        assert np.bincount([rec[k * 32 + i] // 32 for i in range(32)], minlength=8).tolist() == [4] * 8
    cols = np.zeros((64, 6), np.float32)
    cols[:32] = (0, 0, -5.0, 0, 0, 1)
    cols[:32, 0] = 10.0 * np.arange(32)
    cols[32:] = (-5.0, 0, 0, 1, 0, 0)                      # along the rows of the grid: 32 clusters each
    cols[32:, 2] = 10.0 * (np.arange(32) % 8)
    items, pairs = _items(mrt, oracle, grid, cols, sweep, "grid")
    assert items == 32 * 8 + 32 * 32
    # (two spheres per group on the ray's axis; in f32 the discriminant of a few of the farthest rounds below 0)
    assert 32 * 8 * 2 + 32 * 28 * 2 < pairs <= 32 * 8 * 2 + 32 * 32 * 2


@SWEEPS
def test_one_bit_in_each_mask_word(mrt, oracle, sweep):
    """8 slabs of 4 x 8 groups, 70 units apart along x: the builder gives every slab a mask word of its own, so a ray along x
    holds exactly one candidate in each of the block's 8 words (word selection with rank 0 .. 7, every bit rank 0); the lanes in
    between own nothing"""
    sc = _groups_at(mrt, [[70.0 * i, 10.0 * j, 10.0 * k] for i in range(8) for j in range(4) for k in range(8)])
    rec = _records(mrt, sc)
    for j in range(4):
        for k in range(8):
            assert sorted(rec[i * 32 + j * 8 + k] // 32 for i in range(8)) == list(range(8)), "a slab shares a mask word"
    rays = np.zeros((64, 6), np.float32)
    rays[:] = (35.0, 200.0, 5.0, 0, 1, 0)
    for n, (j, k) in enumerate((j, k) for j in range(4) for k in range(8)):
        rays[2 * n] = (-5.0, 10.0 * j, 10.0 * k, 1, 0, 0)
    items, pairs = _items(mrt, oracle, sc, rays, sweep, "slabs")
    # (two spheres per group on the ray's axis; in f32 the discriminant of some of the farthest rounds below 0)
    assert items == 32 * 8 and 32 * 8 < pairs <= 32 * 8 * 2


@SWEEPS
def test_lanes_on_the_literal_path_between_usable_lanes(mrt, oracle, sweep):
    """Odd lanes carry a direction of length 1.5: they take the index-ordered loop and own no items (their count is zeroed,
    whatever their masks hold); the even lanes' items and every lane's winner are the reference's"""
    sc = _groups(mrt, 64, 2)
    rays = _lane_rays(["two"] * 64)
    rays[1::2, 3:] *= 1.5
    ref_hit, ref_t, ref_set, required = oracle.world_hit_batch(oracle.pack_world(to_oracle_spheres(oracle, sc)), rays)
    with mrt.State(mrt.Args(16, 16), seed=1) as st:
        st.set_world(sc)
        st.debug_set_sweep(sweep)
        hit, t, cand = st.debug_world_hit(rays, len(sc))
        traced, member_tests = st.debug_world_hit_stats()
    assert (traced, member_tests) == (64, 4 * 2 * 32)          # the 32 usable lanes' two items each and nothing of the others
    assert (ref_hit >= 0).all()
    assert np.array_equal(hit, ref_hit)
    assert np.array_equal(t.view(np.uint32), ref_t.view(np.uint32))
    assert not cand[1::2].any()
    assert not (required[0::2] & ~cand[0::2]).any() and not (cand[0::2] & ~ref_set[0::2]).any()


@SWEEPS
@pytest.mark.parametrize("n", [124, 500])
def test_random_small_scenes(mrt, oracle, n, sweep):
    """124 and 500 spheres (plus a ground sphere): 1 and 4 mask words, 256 random, grazing and on-surface rays"""
    rng = np.random.default_rng(n)
    sc = _random_scene(mrt, rng, n)
    rays = _rays_for(rng, sc, 96, 96, 64)[:256]
    _check(mrt, oracle, sc, rays, sweep=sweep, what=f"{n} spheres")


def test_a_frame_with_the_camera_lists_in_force(mrt, oracle):
    """The cover scene at 64x64, 4 spp with the lists asked for (the draw-counting small-scene instantiation with the lists):
    three frames -- the lists are in force from the second -- equal the oracle's bits and its three counters; the member tests
    (not an oracle quantity) equal the total recorded from the walk that stored its items, whatever order the rounds take them in"""
    sc, cam = mrt.scene_cover(1, True)
    cnt = oracle.Counters()
    ref = oracle_render(oracle, sc, cam, 64, 64, 4, 50, 3, frames=3, counters=cnt)
    runs = []
    for _ in range(2):
        with mrt.State(mrt.Args(64, 64, 4, 50, 1.0), seed=3) as st:
            st.debug_set_camera_masks(2)
            st.set_world(sc)
            st.set_camera(cam)
            for _ in range(3):
                st.redraw()
            st.sync()
            runs.append((st.read_framebuffer(), st.read_counters(), st.debug_read_camera_masks(table=False)))
    fb, got, info = runs[0]
    assert info["in_force"] and info["lists"]
    assert np.array_equal(fb.view(np.uint32), ref.view(np.uint32)), mismatch_report(fb, ref)
    assert (got["samples"], got["world_hit_calls"], got["rng_draws"]) == (cnt.samples, cnt.world_hit_calls, cnt.rng_draws)
    # (recorded from the commit before the cooperative derivation, whose walk took the same items from a queue: the same sweep
    # masks give the same items, so a derivation that dropped or repeated one would move this total even where the image held)
    assert got["member_tests"] == runs[1][1]["member_tests"] == 1274128
