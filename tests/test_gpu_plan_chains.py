"""The plan chains (tests/plan_chains.py) on a real context against the host model: every call returns the model's status; every
plan read and every plan rendered compares where it stands -- k or k', tile_frames, tiles, frames, used_seq, both variances as
bits --; every check finds what the adaptive chains' checks find, and every plan the ring still holds.

tests/test_plan_chains_host.py shows on the CPU that the chains contain the situations they exist for and that the runner reports
the seeded defects of a stand-in."""
import time

import pytest

import motion_chains as MC
import plan_chains as PC

pytestmark = pytest.mark.gpu


def _guarded(f, *a, **kw):
    """a stalled wait or a HIP error is no comparison failure: nothing more runs on the GPU in this session"""
    try:
        return f(*a, **kw)
    except MC.ChainStopped as e:
        pytest.exit(f"plan chains stopped: {e}", returncode=3)


def _run_case(oracle, name):
    p, ops = PC.params_and_ops(name)
    stats = {}
    t0 = time.perf_counter()
    with _guarded(MC.new_state, p) as st:
        run = _guarded(PC.run, name, st, PC.new_model(oracle, name), oracle, stats)
    checks = sum(v for k, v in stats.items() if isinstance(k, tuple) and k[1] == "checks")
    assert checks == sum(op == ("check",) for op in ops)
    m = run.model
    partial = sum(bool((k != left).any() and left.any()) for k, left in m.targets)
    print(f"plan chain {name} ({p['layout']}, {p['max_w']}, {p['size']}): {len(ops)} ops, {checks} checks, {stats.get('plans checked', 0)} plans "
          f"compared at checks, {len(m.targets)} plans rendered ({partial} with a partial k'), {time.perf_counter() - t0:.2f} s")
    return run


@pytest.mark.parametrize("name", PC.NAMES)
def test_chain_matches_the_model(oracle, name):
    _run_case(oracle, name)


@pytest.mark.parametrize("case", PC.SUITE_CASES)
def test_random_chain_matches_the_model(oracle, case):
    """a random chain (python tests/plan_chains.py CASE prints it)"""
    _run_case(oracle, case)


def test_the_comparison_is_live_on_a_real_context(oracle):
    """the other way round from tests/test_plan_chains_host.py: with a defective model as the reference the runner must report the
    real context as different, for every defect, in the first written chain that catches it on the host.  (Nothing here makes the
    library misbehave: the defect is in the Python model.)"""
    from test_plan_chains_host import CAUGHT_BY, DEFECTS
    for defect in DEFECTS:
        name = CAUGHT_BY[defect.__name__]["written"][0]
        with _guarded(MC.new_state, PC.params_and_ops(name)[0]) as st:
            with pytest.raises(MC.ChainMismatch):
                _guarded(PC.run, name, st, PC.new_model(oracle, name, defect), oracle, device_checks=False)
