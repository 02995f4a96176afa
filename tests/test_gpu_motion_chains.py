"""Chains of updates, regroups, camera changes, frames and temporal steps on a real context against the host model
(tests/motion_chains.py): every call returns the model's status, and every check of every in-suite chain finds the model's
framebuffer, counters, guides, temporal history and image bit for bit, a hierarchy that passes tests/refit_ref.py for the model's
spheres, the member_index tests/regroup_ref.py gives, candidate sets under both sweeps that hold what the oracle requires and
nothing with a negative discriminant, camera masks that cover the current camera's rays, camera-ray sphere lists that are
tests/camera_list_ref.py's for the geometry and camera as they are, and a sound context; and every render launch of the small
layout got the table -- none, the masks, the lists -- that motion_chains.CameraTables predicts from the calls alone.

tests/test_motion_chains_host.py shows on the CPU what the chains cover, that the reference meets the conditions these tests rest
on (hit and sky pixels, rays that hit, history found, fifty scene sizes of drift, radii of a thousandth), and that the runner
reports seeded defects."""
import pytest

import motion_chains as MC

pytestmark = pytest.mark.gpu

STATS = {}                      # case -> the runner's statistics of its in-suite run


def _guarded(f, *a, **kw):
    """A stalled wait or a HIP error is no comparison failure: nothing more runs on the GPU in this session.  Every call the
    runner makes on a context, its read-backs and diagnostics and the context's creation included, raises ChainStopped for them."""
    try:
        return f(*a, **kw)
    except MC.ChainStopped as e:
        pytest.exit(f"motion chains stopped: {e}", returncode=3)


def _state(p):
    return _guarded(MC.new_state, p)


def _run_case(oracle, case):
    p, _ = MC.chain(case)
    stats = {}
    with _state(p) as st:
        _guarded(MC.run, case, st, MC.new_model(oracle, p), oracle, stats)
    STATS[case] = stats
    return stats


def _summary(stats):
    layouts = sorted({k[0] for k in stats if isinstance(k, tuple) and k[0]})
    per = {l: {k[1]: v for k, v in stats.items() if isinstance(k, tuple) and k[0] == l} for l in layouts}
    launches, lists = stats.get("mask launches", []), stats.get("list launches", [])
    return (f"{per}; largest drift {stats['largest drift']:.1f} scene sizes, smallest clustered radius {stats['smallest radius']:.3g}; "
            f"{sum(f for _, f, _ in launches)} of {len(launches)} small-layout launches ran with a table, {sum(f for _, f, _ in lists)} with the lists")


@pytest.mark.parametrize("case", MC.SUITE_CASES)
def test_chain_matches_the_model(oracle, case):
    print(f"chain {case}: " + _summary(_run_case(oracle, case)))


def test_two_chains_side_by_side(oracle):
    """Two contexts on one device through two different chains, op by op in turn, each against its own model: masks with frames
    in flight beside a temporal chain that changes its scene; and a list chain beside a mask chain -- the lists next to the masks
    on one device, each context building its own tables."""
    for one, other in ((1, 7), (12, 1)):
        _side_by_side(oracle, one, other)


def _side_by_side(oracle, one, other):
    (pa, ops_a), (pb, ops_b) = MC.chain(one), MC.chain(other)
    with _state(pa) as a, _state(pb) as b:
        ra = MC.Run(f"chain {one} beside chain {other}", pa, a, MC.new_model(oracle, pa), oracle)
        rb = MC.Run(f"chain {other} beside chain {one}", pb, b, MC.new_model(oracle, pb), oracle)
        for i in range(max(len(ops_a), len(ops_b))):
            if i < len(ops_a):
                _guarded(ra.step, ops_a[i])
            if i < len(ops_b):
                _guarded(rb.step, ops_b[i])


def test_masks_were_in_force_across_generations(oracle):
    """Read from mrt_debug_read_camera_masks' "the most recent launch ran with them" behind every render of the small-layout
    chains: in at least three of them the masks were in force under two or more generations, with 4 or more frames in flight at
    one of them -- otherwise the interleavings of builds and frames in flight were not exercised."""
    small = [case for case in MC.SUITE_CASES[:12] if MC.chain(case)[0]["layout"] == "small"]     # (the numbers below were set for these)
    good, seen = [], {}
    for case in small:
        stats = STATS.get(case) or _run_case(oracle, case)
        in_force = [(gen, fif) for gen, on, fif in stats.get("mask launches", []) if on]
        seen[case] = (len({gen for gen, _ in in_force}), max([fif for _, fif in in_force], default=0))
        if seen[case][0] >= 2 and seen[case][1] >= 4:
            good.append(case)
    print(f"(generations with masks in force, most frames in flight among them) per small-layout chain: {seen}")
    assert len(good) >= 3, seen
    assert sum(STATS[case].get(("small", "mask tables checked"), 0) for case in small) >= 3, "no check ever met a table built for its generation"


def test_lists_were_in_force_across_generations(oracle):
    """The twin for the list chains 12 .. 15, from "the most recent launch ran with the lists": in at least three of them the
    lists were in force under two or more generations, with 4 or more frames in flight at one of them, and at least three checks
    met a list table built for their generation and held it to tests/camera_list_ref.py.  (That the calls alone can meet this:
    tests/test_motion_chains_host.py::test_the_calls_alone_put_the_lists_in_force_across_generations.)"""
    cases = [case for case in MC.SUITE_CASES if "lists" in MC.chain(case)[0]["flavour"]]
    assert cases == [12, 13, 14, 15]
    good, seen = [], {}
    for case in cases:
        stats = STATS.get(case) or _run_case(oracle, case)
        in_force = [(gen, fif) for gen, on, fif in stats.get("list launches", []) if on]
        seen[case] = (len({gen for gen, _ in in_force}), max([fif for _, fif in in_force], default=0))
        if seen[case][0] >= 2 and seen[case][1] >= 4:
            good.append(case)
    checked = {case: STATS[case].get(("small", "list tables checked"), 0) for case in cases}
    print(f"(generations with the lists in force, most frames in flight among them) per list chain: {seen}; list tables checked: {checked}")
    assert len(good) >= 3, seen
    assert sum(checked.values()) >= 3, "no check ever met a list table built for its generation"


def test_the_comparison_is_live_on_a_real_context(oracle):
    """The other way round from tests/test_motion_chains_host.py: with a defective model as the reference, the runner must report
    the real context as different, for every defect, in two chains.  (Nothing here makes the library misbehave: the defect is in
    the Python model.  Only what a model can say is compared.)"""
    from test_motion_chains_host import DEFECTS
    order = sorted(MC.SUITE_CASES, key=lambda c: ("temporal" not in MC.chain(c)[0]["flavour"], c))      # (most defects need a history)
    for defect in DEFECTS:
        caught = 0
        for case in order:
            p, _ = MC.chain(case)
            with _state(p) as st:
                try:
                    _guarded(MC.run, case, st, MC.new_model(oracle, p, defect), oracle, device_checks=False)
                except MC.ChainMismatch:
                    caught += 1
            if caught >= 2:
                break
        assert caught >= 2, defect.__name__
