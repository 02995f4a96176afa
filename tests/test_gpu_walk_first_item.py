"""The small-scene walk's round 0 -- every owner tests its first candidate in the lane -- and the cooperative rounds on the
reduced counts (kernels.hip, "Small scenes"; the numbering is restated in tests/test_walk_first_item_host.py), through
mrt_debug_world_hit as tests/test_gpu_walk_items.py drives it: 64 consecutive rays = the lanes of one wave, in order; per case
the winners equal the oracle's world_hit bit for bit, the (ray, sphere) pairs that reached the root tests lie between the
required and the admissible set (test_gpu_superset._check), and the number of cluster items the walk ran -- round 0's plus the
cooperative rounds', from the launch's member-test counter -- is the number the rays were built to carry.

The scenes are full nx x nz grids of groups of four small spheres, 10 units apart (one group = one cluster and no padding
record, both checked on the host build): 32, 64, 128 or 256 top records = 1, 2, 4 or 8 mask words per lane.  A ray along z
through column i carries nz candidates, a ray along x through row k carries nx, a ray dropped on one group one, a ray pointing
away none; a lane's share of the cooperative rounds is its count less one."""
import numpy as np
import pytest

from common import mismatch_report, oracle_render, to_oracle_spheres
from test_gpu_superset import _check
from test_gpu_walk_items import _groups, _records, _row
from test_hierarchy_host import build

pytestmark = pytest.mark.gpu
SWEEPS = pytest.mark.parametrize("sweep", [1, 2], ids=["valu-sweep", "matrix-core-sweep"])
_SCENES = {}


def _grid(mrt, nx, nz):
    """(spheres, group -> top record) of the grid: group k nx + i around (10 i, 0, 10 k)"""
    if (nx, nz) not in _SCENES:
        sc = _groups(mrt, nx, nz)
        rec = _records(mrt, sc)
        assert len(build(mrt, sc)["top"]) == nx * nz           # no padding records: nx nz / 32 full mask words
        _SCENES[nx, nz] = (sc, rec)
    return _SCENES[nx, nz]


def _rays(kinds):
    """('col', i): along z through column i; ('row', k): along x through row k; ('drop', i, k): down through one sphere of group
    (i, k); ('none', j): away from everything.  Axis-parallel directions, so exactly unit length"""
    rays = np.zeros((len(kinds), 6), np.float32)
    for j, kind in enumerate(kinds):
        if kind[0] == "col":
            rays[j] = (10.0 * kind[1], 0.0, -5.0, 0, 0, 1)
        elif kind[0] == "row":
            rays[j] = (-5.0, 0.0, 10.0 * kind[1], 1, 0, 0)
        elif kind[0] == "drop":
            rays[j] = (10.0 * kind[1] + 0.1, 5.0, 10.0 * kind[2], 0, -1, 0)
        else:
            rays[j] = (10.0 * kind[1] + 5.0, 50.0, 5.0, 0, 1, 0)
    return rays


def _count(kind, nx, nz):
    return dict(col=nz, row=nx, drop=1, none=0)[kind[0]]


def _run(mrt, oracle, nx, nz, kinds, sweep, what, reduced=None):
    """_check's comparisons for the wave's 64 rays, then the cluster items the walk ran"""
    sc, _ = _grid(mrt, nx, nz)
    assert len(kinds) == 64
    if reduced is not None:
        assert sum(max(_count(k, nx, nz) - 1, 0) for k in kinds) == reduced
    rays = _rays(kinds)
    variant, pairs, _ = _check(mrt, oracle, sc, rays, sweep=sweep, what=what)
    assert variant == sweep
    with mrt.State(mrt.Args(16, 16), seed=1) as st:
        st.set_world(sc)
        st.debug_set_sweep(sweep)
        st.debug_world_hit(rays, len(sc))
        traced, member_tests = st.debug_world_hit_stats()
    assert traced == 64 and member_tests % 4 == 0
    want = sum(_count(k, nx, nz) for k in kinds)
    assert member_tests // 4 == want, f"{what}: {member_tests // 4} cluster items, the rays carry {want}"
    return pairs


def _mix(nx, nz, rows, cols, drops=0):
    """`rows` row rays, `cols` column rays and `drops` dropped rays, interleaved over the wave's lanes; the rest point away"""
    kinds = [("row", r % nz) for r in range(rows)] + [("col", c % nx) for c in range(cols)] + [("drop", (3 * q) % nx, q % nz) for q in range(drops)]
    assert len(kinds) <= 64
    kinds += [("none", j) for j in range(64 - len(kinds))]
    order = np.random.default_rng(len(kinds) + rows + 7 * cols).permutation(64)
    return [kinds[p] for p in order]


@SWEEPS
@pytest.mark.parametrize("nx,nz", [(32, 1), (32, 2), (32, 4), (32, 8)], ids=["32", "64", "128", "256"])
def test_one_candidate_each_runs_no_cooperative_round(mrt, oracle, nx, nz, sweep):
    """64 lanes dropped on one group each: round 0 is the whole walk"""
    kinds = [("drop", (5 * j) % nx, j % nz) for j in range(64)]
    pairs = _run(mrt, oracle, nx, nz, kinds, sweep, f"one each, {nx * nz} records", reduced=0)
    assert pairs == 64                                         # the sphere the ray drops through


@SWEEPS
@pytest.mark.parametrize("nx", [16, 32, 64, 128], ids=["32", "64", "128", "256"])
def test_two_candidates_each_run_one_full_cooperative_round(mrt, oracle, nx, sweep):
    kinds = [("col", (j * 7) % nx) for j in range(64)]
    _run(mrt, oracle, nx, 2, kinds, sweep, f"two each, {2 * nx} records", reduced=64)


# reduced total -> (nx, nz, row rays, column rays, dropped rays): 63 / 64 / 65 around one cooperative round
ROUND = {63: (64, 2, 0, 63, 1), 64: (64, 2, 0, 64, 0), 65: (32, 4, 2, 1, 40)}
# 255 / 256 / 257 around the table's window, in 4 words (columns of 4, rows of 32) and in 8 words (columns of 8, rows of 32)
WINDOW = {(255, 128): (32, 4, 3, 54, 7), (256, 128): (32, 4, 4, 44, 16), (257, 128): (32, 4, 5, 34, 20),
          (255, 256): (32, 8, 1, 32, 31), (256, 256): (32, 8, 6, 10, 40), (257, 256): (32, 8, 4, 19, 30)}


@SWEEPS
@pytest.mark.parametrize("reduced", sorted(ROUND))
def test_reduced_totals_around_a_round(mrt, oracle, reduced, sweep):
    nx, nz, rows, cols, drops = ROUND[reduced]
    _run(mrt, oracle, nx, nz, _mix(nx, nz, rows, cols, drops), sweep, f"reduced total {reduced}", reduced=reduced)


@SWEEPS
@pytest.mark.parametrize("reduced,total", sorted(WINDOW))
def test_reduced_totals_around_the_table_window(mrt, oracle, reduced, total, sweep):
    nx, nz, rows, cols, drops = WINDOW[reduced, total]
    assert nx * nz == total
    _run(mrt, oracle, nx, nz, _mix(nx, nz, rows, cols, drops), sweep, f"reduced total {reduced}, {total} records", reduced=reduced)


@SWEEPS
@pytest.mark.parametrize("total", [32, 64])
def test_one_lane_with_every_cluster_among_lanes_with_none_or_one(mrt, oracle, total, sweep):
    """One column holds the whole scene; lane 41 threads it, the others drop on one of its groups or point away"""
    kinds = [("drop", 0, (7 * j) % total) if j % 3 else ("none", j) for j in range(64)]
    kinds[41] = ("col", 0)
    _run(mrt, oracle, 1, total, kinds, sweep, f"one lane holds all {total}", reduced=total - 1)


@SWEEPS
def test_one_lane_with_every_cluster_of_eight_words(mrt, oracle, sweep):
    """The row of 250 clusters (8 mask words): lane 9 threads it -- one item in the lane, 249 through the cooperative rounds --
    between lanes without a candidate and lanes dropped on one sphere of the row (its cluster, perhaps a neighbouring bound)"""
    sc = _row(mrt)
    rays = np.zeros((64, 6), np.float32)
    rays[:] = (0.0, 40.0, 7.0, 0, 1, 0)
    rays[:, 0] = 3.0 + 5.0 * np.arange(64)
    drops = [j for j in range(1, 64, 4) if j != 9]
    for j in drops:
        rays[j] = (0.5 * (15 * j), 3.0, 0.0, 0, -1, 0)
    rays[9] = (-5.0, 0.0, 0.0, 1, 0, 0)
    _check(mrt, oracle, sc, rays, sweep=sweep, what="row")
    with mrt.State(mrt.Args(16, 16), seed=1) as st:
        st.set_world(sc)
        st.debug_set_sweep(sweep)
        st.debug_world_hit(rays, len(sc))
        traced, member_tests = st.debug_world_hit_stats()
    assert traced == 64 and member_tests % 4 == 0
    assert 250 + len(drops) <= member_tests // 4 <= 250 + 3 * len(drops)


@SWEEPS
@pytest.mark.parametrize("nx,nz", [(32, 2), (64, 4)], ids=["64", "256"])
def test_usable_and_unusable_lanes_interleaved(mrt, oracle, nx, nz, sweep):
    """Odd lanes carry a direction of length 1.5: they take the index-ordered loop, own no items -- neither in round 0 nor in
    the cooperative rounds, whatever their mask words hold -- and still get the reference's winner"""
    sc, _ = _grid(mrt, nx, nz)
    rays = _rays([("col", (5 * j) % nx) for j in range(64)])
    rays[1::2, 3:] *= 1.5
    ref_hit, ref_t, ref_set, required = oracle.world_hit_batch(oracle.pack_world(to_oracle_spheres(oracle, sc)), rays)
    with mrt.State(mrt.Args(16, 16), seed=1) as st:
        st.set_world(sc)
        st.debug_set_sweep(sweep)
        assert st.debug_sweep_variant() == sweep
        hit, t, cand = st.debug_world_hit(rays, len(sc))
        traced, member_tests = st.debug_world_hit_stats()
    assert (traced, member_tests) == (64, 4 * nz * 32)
    assert (ref_hit >= 0).all()
    assert np.array_equal(hit, ref_hit)
    assert np.array_equal(t.view(np.uint32), ref_t.view(np.uint32))
    assert not cand[1::2].any()
    assert not (required[0::2] & ~cand[0::2]).any() and not (cand[0::2] & ~ref_set[0::2]).any()


@SWEEPS
@pytest.mark.parametrize("nx,nz", [(32, 1), (32, 2), (32, 4), (32, 8)], ids=["32", "64", "128", "256"])
def test_the_only_candidate_is_the_last_record_of_the_last_word(mrt, oracle, nx, nz, sweep):
    """Lane 37 drops on the group that the builder made the scene's last top record -- bit 0 of the top word -- and nobody else
    holds anything: round 0 alone, one item"""
    _, rec = _grid(mrt, nx, nz)
    last = [g for g, r in rec.items() if r == nx * nz - 1]
    assert len(last) == 1
    kinds = [("none", j) for j in range(64)]
    kinds[37] = ("drop", last[0] % nx, last[0] // nx)
    pairs = _run(mrt, oracle, nx, nz, kinds, sweep, f"last record of {nx * nz}", reduced=0)
    assert pairs == 1


_FRAME = {}


def _cover_reference(mrt, oracle):
    """the cover scene at 64x64, 2 spp, depth 50, three frames: computed once, shared by the two launch forms"""
    if not _FRAME:
        sc, cam = mrt.scene_cover(1, True)
        cnt = oracle.Counters()
        _FRAME["ref"] = (sc, cam, oracle_render(oracle, sc, cam, 64, 64, 2, 50, 3, frames=3, counters=cnt), cnt)
    return _FRAME["ref"]


# member tests of the three frames, recorded from the commit before round 0 (the cooperative derivation alone): the same sweep
# masks give the same items, so a walk that dropped or repeated one would move the total even where the image held
MEMBER_TESTS = {2: 637223, 3: 682811}


@pytest.mark.parametrize("mode,lists", [(2, True), (3, False)], ids=["lists-sc3", "masks-sc0"])
def test_a_frame_with_the_lists_and_one_with_the_masks(mrt, oracle, mode, lists):
    """The draw-counting small-scene instantiations, with the camera-ray lists (SC = 3) and with the masks (SC = 0): three frames
    -- the tables are in force from the second -- equal the oracle's bits and its three counters, and the member tests equal the
    total recorded before round 0 existed"""
    sc, cam, ref, cnt = _cover_reference(mrt, oracle)
    with mrt.State(mrt.Args(64, 64, 2, 50, 1.0), seed=3) as st:
        st.debug_set_camera_masks(mode)
        st.set_world(sc)
        st.set_camera(cam)
        for _ in range(3):
            st.redraw()
        st.sync()
        fb, got, info = st.read_framebuffer(), st.read_counters(), st.debug_read_camera_masks(table=False)
        main, _ = st.debug_last_launch()
    print(f"mode {mode}: member_tests {got['member_tests']}, last launch {main}, {info}")
    assert info["in_force"] and info["lists"] == lists
    assert main & 8 and bool(main & 64) == lists
    assert np.array_equal(fb.view(np.uint32), ref.view(np.uint32)), mismatch_report(fb, ref)
    assert (got["samples"], got["world_hit_calls"], got["rng_draws"]) == (cnt.samples, cnt.world_hit_calls, cnt.rng_draws)
    assert got["member_tests"] == MEMBER_TESTS[mode]
