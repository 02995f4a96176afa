"""The adaptive chains (tests/adaptive_chains.py) on a real context against the host model: every call returns the model's status;
every selection, allocation, read and present compares where it stands; and every check finds the model's framebuffer, counters,
n_t, S, newest report and tile map, guides, denoised image, temporal history (the response's H2 included) and image bit for bit (a report's doubles at
state_sequences.REPORT_REL), next to everything motion_chains.Run.check_device holds a context to.  Every render launch of the
small layout, subset launches included, got the camera table that motion_chains.CameraTables predicts from the calls alone.

tests/test_adaptive_chains_host.py shows on the CPU that the chains contain the twelve situations, that the reference meets the
conditions these tests rest on, and that the runner reports the seeded defects."""
import time

import pytest

import adaptive_chains as AC
import motion_chains as MC

pytestmark = pytest.mark.gpu

STATS = {}                      # name -> the runner's statistics of its in-suite run


def _guarded(f, *a, **kw):
    """a stalled wait or a HIP error is no comparison failure: nothing more runs on the GPU in this session"""
    try:
        return f(*a, **kw)
    except MC.ChainStopped as e:
        pytest.exit(f"adaptive chains stopped: {e}", returncode=3)


def _run_case(oracle, name):
    p, ops = AC.params_and_ops(name)            # (a written chain by its name, a random one by its case number)
    stats = {}
    t0 = time.perf_counter()
    with _guarded(MC.new_state, p) as st:
        _guarded(AC.run, name, st, AC.new_model(oracle, name), oracle, stats)
    stats["seconds"] = time.perf_counter() - t0
    STATS[name] = stats
    return stats


def _count(stats, what):
    return sum(v for k, v in stats.items() if isinstance(k, tuple) and k[1] == what)


@pytest.mark.parametrize("name", AC.NAMES)
def test_chain_matches_the_model(oracle, name):
    stats = _run_case(oracle, name)
    ops = AC.CHAINS[name][1]
    assert _count(stats, "checks") == sum(op == ("check",) for op in ops)
    print(_statistics("adaptive chain", name, ops, stats))
    if name == "regroups":
        assert _count(stats, "auto regroups") >= 1, "the policy's gate never opened"


def _statistics(what, name, ops, stats):
    return (f"{what} {name}: {len(ops)} ops, {_count(stats, 'checks')} checks ({stats['diverged checks']} diverged, {stats.get('h2 checks', 0)} of H2), "
            f"{_count(stats, 'regroups')} regroups, {_count(stats, 'auto regroups')} by the policy, {stats['seconds']:.2f} s")


@pytest.mark.parametrize("case", AC.SUITE_CASES)
def test_random_chain_matches_the_model(oracle, case):
    """a random chain (python tests/adaptive_chains.py CASE prints it): every call returns the model's status, every check finds
    what the written chains' checks find, the fast history H2 of the temporal response included"""
    stats = _run_case(oracle, case)
    p, ops = AC.chain(case)
    assert _count(stats, "checks") == sum(op == ("check",) for op in ops)
    print(_statistics(f"random adaptive chain ({p['layout']}, {p['max_w']}, {p['size']}, {p['flavour']})", case, ops, stats))


def test_two_chains_side_by_side(oracle):
    """two contexts on one device through two different chains, op by op in turn, each against its own model: forced tables with
    frames in flight beside a temporal chain on the wider image; reports and budgets beside the large layout; a random chain with
    the response on beside a random chain of a large layout"""
    for one, other in (("tables", "temporal-075"), ("reports", "large"), (13, 18)):
        (pa, ops_a), (pb, ops_b) = AC.params_and_ops(one), AC.params_and_ops(other)
        with _guarded(MC.new_state, pa) as a, _guarded(MC.new_state, pb) as b:
            ra = AC.new_run(one, a, AC.new_model(oracle, one), oracle)
            rb = AC.new_run(other, b, AC.new_model(oracle, other), oracle)
            for i in range(max(len(ops_a), len(ops_b))):
                if i < len(ops_a):
                    _guarded(ra.step, ops_a[i])
                if i < len(ops_b):
                    _guarded(rb.step, ops_b[i])


def test_subset_launches_ran_with_masks_and_with_lists_across_generations(oracle):
    """from mrt_debug_read_camera_masks' "the most recent launch ran with them" behind every subset launch of the chain that forces
    the tables: the masks were in force under three or more generations, then the lists under three or more, with 4 or more frames
    in flight (that the calls alone can meet this: tests/test_adaptive_chains_host.py)"""
    stats = STATS.get("tables") or _run_case(oracle, "tables")
    masks = {gen for (gen, on, fif), (_, lists, _) in zip(stats["subset mask launches"], stats["subset list launches"]) if on and not lists and fif >= 4}
    lists = {gen for gen, on, fif in stats["subset list launches"] if on and fif >= 4}
    print(f"generations under which subset launches ran with the masks: {sorted(masks)}, with the lists: {sorted(lists)}")
    assert len(masks) >= 3 and len(lists) >= 3      # (the switch begins no generation: the two may share the one it was made under)
    assert _count(stats, "mask tables checked") >= 1 and _count(stats, "list tables checked") >= 1


def test_the_comparison_is_live_on_a_real_context(oracle):
    """the other way round from tests/test_adaptive_chains_host.py: with a defective model as the reference the runner must report
    the real context as different, for every defect, in a chain that catches it on the host.  (Nothing here makes the library
    misbehave: the defect is in the Python model.  Only what a model can say is compared.)"""
    from test_adaptive_chains_host import CAUGHT_BY, DEFECTS, RESPONSE_DEFECTS, SUITE_CAUGHT_BY
    for defect in DEFECTS:
        if defect in RESPONSE_DEFECTS:          # (the response's: the shortest random chain that catches it on the host)
            name = min(SUITE_CAUGHT_BY[defect.__name__], key=lambda c: (len(AC.chain(c)[1]), c))
        else:
            name = next(n for n in CAUGHT_BY[defect.__name__] if n != "denoise-long")       # (the shortest runs)
        with _guarded(MC.new_state, AC.params_and_ops(name)[0]) as st:
            with pytest.raises(MC.ChainMismatch):
                _guarded(AC.run, name, st, AC.new_model(oracle, name, defect), oracle, device_checks=False)
