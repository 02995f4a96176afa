"""Random call sequences on a real context against the host model (tests/state_sequences.py, tests/state_model.py): every op of
every in-suite case, and of two contexts driven side by side, returns what the model returns -- framebuffer, S, n_t, frames_done,
the next Locals, seeds, guides, the denoised image, presented bytes and their numbering, reports, tile maps, render_adaptive's
selection, counters and the status of every call.  Scheduling is never compared.

Counters are compared in every sequence, subset frames included: the model renders a subset frame's tiles as rectangles through
the oracle, and a pixel's samples, world_hit calls and draws do not depend on the rectangle it is rendered in
(tests/test_state_model.py checks that two complementary tile lists count what one whole frame counts)."""
import pytest

import state_sequences as SS

pytestmark = pytest.mark.gpu

SMALL = 8                       # debug_last_launch: the render kernel's small-scene instantiation
FRAME_OPS = ("redraw", "render", "render_tiles", "render_adaptive")
LAYOUTS = {}                    # case -> per accumulation, the layouts its render launches used


def _state(p):
    st = SS.new_state(p)
    st.set_wait_timeout(60.0)   # (a stalled wait fails the case with the wait's name long before the suite's own limit)
    return st


def _layout_recorder(case):
    runs = LAYOUTS.setdefault(case, [set()])
    seen = {"frames": 0}

    def after(i, op, status, st):
        if op[0] == "reset" and status == 0:
            runs.append(set())
            seen["frames"] = 0
        elif op[0] in FRAME_OPS and status == 0 and st.frames_done > seen["frames"]:
            seen["frames"] = st.frames_done
            runs[-1].add(bool(st.debug_last_launch()[0] & SMALL))
    return after


def _guarded(f, *a, **kw):
    """A stalled wait or a HIP error is no comparison failure: nothing more runs on the GPU in this session."""
    try:
        f(*a, **kw)
    except SS.SequenceStopped as e:
        pytest.exit(f"state sequences stopped: {e}", returncode=3)


def _run_case(oracle, case):
    p, _ = SS.sequence(case)
    LAYOUTS.pop(case, None)
    with _state(p) as st:
        _guarded(SS.run, case, st, SS.new_model(oracle, p), after=_layout_recorder(case))


@pytest.mark.parametrize("case", SS.SUITE_CASES)
def test_sequence_matches_the_model(oracle, case):
    _run_case(oracle, case)


def test_both_scene_layouts_ran_inside_one_accumulation(oracle):
    """The one thing read from the launch diagnostics: over the in-suite cases some accumulation (no reset in between) launched
    both the small-scene and the large-scene instantiation of the render kernel."""
    for case in SS.SUITE_CASES:
        if case not in LAYOUTS:
            _run_case(oracle, case)
    both = [case for case, runs in LAYOUTS.items() if any(r == {True, False} for r in runs)]
    assert len(both) >= 2, LAYOUTS


def test_two_contexts_side_by_side(oracle):
    """Two contexts on one device through two different cases, op by op in turn, each against its own model."""
    (pa, ops_a), (pb, ops_b) = SS.sequence(3), SS.sequence(6)
    with _state(pa) as a, _state(pb) as b:
        ma, mb = SS.new_model(oracle, pa), SS.new_model(oracle, pb)
        for i in range(max(len(ops_a), len(ops_b))):
            if i < len(ops_a):
                _guarded(SS.run_ops, f"case 3 beside case 6, from op {i}", ops_a[i:i + 1], a, ma)
            if i < len(ops_b):
                _guarded(SS.run_ops, f"case 6 beside case 3, from op {i}", ops_b[i:i + 1], b, mb)


def test_the_comparison_is_live_on_a_real_context(oracle):
    """The other way round from tests/test_state_model.py: with a defective model as the reference, the runner must report the
    real context as different -- for every one of the eight defects, somewhere in the in-suite cases.  (Nothing here makes the
    library misbehave: the defect is in the Python model.)"""
    from test_state_model import DEFECTS
    for defect in DEFECTS:
        caught = 0
        for case in SS.SUITE_CASES:
            p, _ = SS.sequence(case)
            with _state(p) as st:
                try:
                    _guarded(SS.run, case, st, SS.new_model(oracle, p, defect))
                except SS.SequenceMismatch:
                    caught += 1
            if caught >= 2:
                break
        assert caught >= 2, defect.__name__
