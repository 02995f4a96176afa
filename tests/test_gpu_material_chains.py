"""The material chains (tests/material_chains.py) on a real context against the host model: every call returns the model's
status, and every check finds the model's framebuffer, counters, guides, temporal history and image bit for bit, a hierarchy that
still passes tests/refit_ref.py, the reference's member_index, sound candidate sets under both sweeps, camera tables that cover
the current camera's rays and a sound context; every render launch of the small layout got the camera table that the calls
predict when a material edit counts as no new generation.

tests/test_material_chains_host.py shows on the CPU what the chains cover, that the flag restarts some pixels and leaves others,
and that the runner reports seeded defects."""
import pytest

import material_chains as XC
import motion_chains as MC

pytestmark = pytest.mark.gpu


def _guarded(f, *a, **kw):
    """a stalled wait or a HIP error is no comparison failure: nothing more runs on the GPU in this session"""
    try:
        return f(*a, **kw)
    except MC.ChainStopped as e:
        pytest.exit(f"material chains stopped: {e}", returncode=3)


@pytest.mark.parametrize("name", XC.NAMES)
def test_chain_matches_the_model(oracle, name):
    p, ops = XC.CHAINS[name]
    stats = {}
    with _guarded(MC.new_state, p) as st:
        run = _guarded(XC.run, name, st, XC.new_model(oracle, name), oracle, stats)
    layout = p["layout"]
    assert stats[(layout, "checks")] == sum(op[0] == "check" for op in ops)
    print(f"material chain {name}: {len(ops)} ops, {stats[(layout, 'checks')]} checks, {stats.get((layout, 'regroups'), 0)} regroups")
    if name == "small-masks":
        # tables were in force across edits: launches ran with a table under a generation that an edit did not end
        launches = stats["mask launches"]
        assert sum(on for _, on, _ in launches) >= 4, launches
        assert stats.get((layout, "mask tables checked"), 0) >= 1
    if "temporal" in name:
        assert sum(f for first, f, n in run.model.found if not first) > 0


def test_the_comparison_is_live_on_a_real_context(oracle):
    """with a defective model as the reference the runner must report the real context as different (the defect is in the
    Python model; only what a model can say is compared)"""
    from test_material_chains_host import FlagIgnored, GuidesNotStaleAfterMaterials, OffByOneRange
    for defect, name in ((FlagIgnored, "small-temporal"), (GuidesNotStaleAfterMaterials, "small-temporal"), (OffByOneRange, "small-masks")):
        with _guarded(MC.new_state, XC.CHAINS[name][0]) as st:
            with pytest.raises(MC.ChainMismatch):
                _guarded(XC.run, name, st, XC.new_model(oracle, name, defect), oracle, device_checks=False)
