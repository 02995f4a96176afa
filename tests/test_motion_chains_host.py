"""Host tests of the motion chains (tests/motion_chains.py): the generator is deterministic and covers its vocabulary and the three
call patterns the chains exist for; the reference alone meets the conditions without which the GPU tests would pass vacuously;
and the runner, driven with the model in the implementation's place, reports every seeded defect of that stand-in."""
import hashlib
import json
import os

import numpy as np
import pytest

import motion_chains as MC
from motion_chains import H, W

FILLERS = ("render", "temporal_step", "set_camera")       # ops that may stand between the ops of a pattern


def _matches(ops, pattern, fillers=FILLERS):
    """the pattern's predicates match consecutive ops of `ops`, fillers between them skipped"""
    for start in range(len(ops)):
        i, k = start, 0
        while i < len(ops) and k < len(pattern):
            if pattern[k](ops[i]):
                i, k = i + 1, k + 1
            elif k and ops[i][0] in fillers:
                i += 1
            else:
                break
        if k == len(pattern):
            return True
    return False


is_op = lambda name, kind=None: (lambda op: op[0] == name and (kind is None or op[1] == kind))


def test_a_case_number_reproduces_its_chain():
    for case in MC.SUITE_CASES:
        assert MC.chain(case) == MC.chain(case)
    assert MC.chain(0)[1] != MC.chain(1)[1]


def test_the_generator_still_draws_the_recorded_chains():
    """tests/golden/motion_chain_digests.json: sha256 of repr(chain(case)), cases 0 .. 11 recorded before the list flavours were
    added to the generator (they must not change by one op: the suite's statistics were set for them), 12 .. 15 when they were final"""
    with open(os.path.join(os.path.dirname(__file__), "golden", "motion_chain_digests.json")) as f:
        want = json.load(f)
    assert sorted(want, key=int) == [str(c) for c in MC.SUITE_CASES]
    got = {str(c): hashlib.sha256(repr(MC.chain(c)).encode()).hexdigest() for c in MC.SUITE_CASES}
    assert got == want, [c for c in got if got[c] != want[c]]


LIST_CASES = (12, 13, 14, 15)


def test_the_list_chains_switch_between_no_table_the_masks_and_the_lists():
    modes = set()
    for case in LIST_CASES:
        p, ops = MC.chain(case)
        assert "lists" in p["flavour"] and p["layout"] == "small"
        assert ops[1] == ("set_camera_masks", 2) and ("set_frame_batching", 0) in ops[:4]
        assert {op[0] for op in ops} <= set(MC.VOCABULARY)
        switch = [op[1] for op in ops if op[0] == "set_camera_masks"]
        assert all(type(v) is int and v in (0, 2, 3) for v in switch) and switch[-1] == 2, (case, switch)
        modes |= set(switch)
    assert modes == {0, 2, 3}
    for case in (0, 1, 2, 3):                   # the mask chains: off and the library's rule
        assert {op[1] for op in MC.chain(case)[1] if op[0] == "set_camera_masks"} <= {False, True}


def _predicted(stats):
    """(generations with the lists in force, most frames in flight among them) from the decision model's own predictions"""
    on = [(gen, fif) for gen, in_force, lists, fif in stats.get("predicted launches", []) if in_force and lists]
    return len({gen for gen, _ in on}), max([fif for _, fif in on], default=0)


def test_the_calls_alone_put_the_lists_in_force_across_generations(reference_runs):
    """what tests/test_gpu_motion_chains.py::test_lists_were_in_force_across_generations asks of the device, asked of
    CameraTables with no device: the condition can be met by the calls alone"""
    seen = {case: _predicted(reference_runs[case][6]) for case in LIST_CASES}
    assert sum(gens >= 2 and fif >= 4 for gens, fif in seen.values()) >= 3, seen
    for case in (0, 1, 2, 3):                   # (the mask chains never ask for the lists: mode 1 leaves `lists` open)
        assert all(lists is None or not in_force for _, in_force, lists, _ in reference_runs[case][6]["predicted launches"])


def test_the_in_suite_cases_cover_the_vocabulary_and_the_patterns():
    ops_in, kinds_in, refusals = {}, {}, set()
    patterns = dict.fromkeys(("regroup, partial update, check", "update, regroup, update, regroup", "another sphere count, temporal on"), 0)
    blocks, in_flight, sweeps, mask_switch = set(), set(), set(), set()
    for case in MC.SUITE_CASES:
        p, ops = MC.chain(case)
        # (chain 8 is the long one: fifty-two drifts of one scene size each)
        assert len(ops) <= (130 if p["flavour"] == "long drift" else 40) and ops[-1] == ("check",) and ops[0] == ("set_world", p["layout"])
        if p["flavour"] == "long drift":
            drifts = [op for op in ops if op[0] == "update" and op[1] == "drift"]
            assert len(drifts) >= 50 and all(op[3] == 1 for op in drifts)
        assert p["max_w"] == (0.0 if any(op[0] == "set_temporal" for op in ops) else 1.0)
        assert sum(op[0] == "refused" for op in ops) == 1
        for op in ops:
            ops_in.setdefault(op[0], set()).add(case)
            if op[0] == "update":
                kinds_in.setdefault(op[1], set()).add(case)
            if op[0] == "refused":
                refusals.add(op[1])
            if op[0] == "set_regroup_block":
                blocks.add(op[1])
            if op[0] == "set_frames_in_flight":
                in_flight.add(op[1])
            if op[0] == "set_sweep":
                sweeps.add(op[1])
            if op[0] == "set_camera_masks":
                mask_switch.add(op[1])
        # a check follows every regroup before the grouping changes again (straight behind it in seg_two_regroups; behind the
        # updates and frames queued on purpose behind the regroup elsewhere: tests/motion_chains.py, "Checks"), and every third update
        owed = updates = 0
        for op in ops:
            if op[0] == "check":
                owed = updates = 0
            elif op[0] in ("regroup", "set_world"):
                assert not owed, (case, "a regroup without a check")
                owed = op[0] == "regroup"
            elif op[0] == "update":
                updates += 1
                assert updates <= 3, case
        patterns["regroup, partial update, check"] += _matches(ops, [is_op("regroup"), is_op("update", "partial"), is_op("check")])
        patterns["update, regroup, update, regroup"] += _matches(ops, [is_op("update"), is_op("regroup"), is_op("update"), is_op("regroup")],
                                                                 FILLERS + ("check",))
        temporal, n, counts = False, None, set()
        for op in ops:
            if op[0] == "set_temporal":
                temporal = op[1]
            if op[0] == "set_world":
                m = len(MC.layout_scene(op[1]))
                if temporal and n is not None and m != n:
                    counts.add((n, m))
                n = m
        patterns["another sphere count, temporal on"] += bool(counts)
    for name in MC.VOCABULARY:
        assert len(ops_in.get(name, ())) >= 2, name
    for kind in MC.UPDATE_KINDS:
        assert len(kinds_in.get(kind, ())) >= 2, kind
    assert all(v >= 3 for v in patterns.values()), patterns
    assert refusals == set(MC.REFUSALS)
    assert blocks == {0, 4} and in_flight == {0, 1, 4, 8} and sweeps == {0, 1, 2} and mask_switch == {False, True, 2, 3}
    layouts = {MC.chain(c)[0]["layout"] for c in MC.SUITE_CASES}
    assert layouts == {"small", "large-quad", "large-lin", "deep-4200"}
    # the partial updates: a range that ends at the last sphere, one of exactly one sphere, one anywhere
    assert {op[2] % 3 for c in MC.SUITE_CASES for op in MC.chain(c)[1] if op[0] == "update" and op[1] == "partial"} == {0, 1, 2}


@pytest.fixture(scope="module")
def reference_runs(oracle):
    """every in-suite case run with the model in both places: per case (params, ops, per check: (guide hits, ray hit share, pairs per
    ray), the model, the shadow, the shadow's figures behind every op, the runner's statistics)"""
    out = {}
    for case in MC.SUITE_CASES:
        checks, trace = [], []

        def after(i, op, run):
            sh, m = run.sh, run.model
            trace.append((float(np.abs(sh.xyzr()).max()), max(abs(v) for v in sh.cam[0])))
            if op[0] == "check":
                g = m.debug_read_guides()
                rays, _, _ = MC.check_rays(m.spheres, m.cam_raw)
                hit, _, _, required = MC.reference_hits(oracle, m.spheres, rays)
                unit = np.abs((rays[:, 3:].astype(np.float64) ** 2).sum(1) - 1.0) < 5e-6
                checks.append((int((g["index"] >= 0).sum()), float((hit >= 0).mean()), float(required.sum()) / len(rays), bool(unit.all())))
        p, ops = MC.chain(case)
        run = MC.run(case, MC.new_model(oracle, p), MC.new_model(oracle, p), oracle, after=after)
        out[case] = (p, ops, checks, run.model, run.sh, trace, run.stats)
    return out


def test_the_reference_meets_the_conditions_the_gpu_tests_rest_on(reference_runs):
    drift_cases = shrink_cases = temporal_cases = 0
    for case, (p, ops, checks, model, sh, trace, _) in reference_runs.items():
        assert len(checks) == sum(op[0] == "check" for op in ops)
        for k, (guide_hits, hit_share, pairs, unit) in enumerate(checks):
            assert 0 < guide_hits < W * H, (case, k, "the guides need hit pixels and sky pixels")
            assert hit_share >= 0.25 and pairs > 1.0, (case, k, hit_share, pairs)
            assert unit, (case, k, "a ray that |d.d - 1| would drop")
        assert max(t[0] for t in trace) <= MC.LIMIT and max(t[1] for t in trace) <= MC.LIMIT, case
        if "temporal" in p["flavour"]:
            later = [(f, n) for first, f, n in model.found if not first]
            assert len(later) >= 4 and sum(f for f, _ in later) >= 0.25 * sum(n for _, n in later), (case, model.found)
            assert sum(first for first, _, _ in model.found) >= 2, (case, "the history was never dropped and begun again")
            temporal_cases += 1
        if "drift" in p["flavour"]:
            assert sh.drifted() >= 50.0, (case, sh.drifted())
            drift_cases += 1
        if "shrink" in p["flavour"]:
            assert sh.smallest_clustered_radius() <= 1e-3 * sh.rmin0, (case, sh.smallest_clustered_radius(), sh.rmin0)
            third = (sh.n - 1) // 3
            assert np.abs(sh.sc["radius"][:third]).max() <= 1.001e-3 * 0.5, case      # three shrinks in a row, not one sphere alone
            shrink_cases += 1
    assert drift_cases >= 2 and shrink_cases >= 2 and temporal_cases >= 4
    print({c: len(r[1]) for c, r in reference_runs.items()})


# ------------------------------------------------------------------ the runner detects defects of the stand-in

class GuidesNotStaleAfterUpdate(MC.Model):
    """mrt_update_spheres forgets to mark the guides stale: the next read and the next step use the old first hits"""
    def _after_update(self):
        pass


class UpdateDropsHistory(MC.Model):
    """mrt_update_spheres drops the temporal history, as mrt_set_world does"""
    def _after_update(self):
        super()._after_update()
        self._drop_history()


class HistoryKeptAcrossSetWorld(MC.Model):
    """mrt_set_world keeps the history although the sphere indices mean something else now"""
    def _after_set_world(self):
        pass


class FrameTakesTheNextGeometry(MC.Model):
    """an update overtakes the frame queued before it: that frame renders the geometry of the call after it"""
    def _after_update(self):
        super()._after_update()
        if self.frames:
            _, cam_raw, key = self.frames[-1]
            self.frames[-1] = (self.spheres, cam_raw, (MC._key(self.spheres), key[1]))
            del self.done[len(self.frames) - 1:]


class ResetClearsHistory(MC.Model):
    """mrt_reset drops the temporal history"""
    def _after_reset(self):
        self._drop_history()


class RefusedUpdateApplied(MC.Model):
    """a refused mrt_update_spheres has written the spheres of its range that exist"""
    def _refused_update(self, first, arr):
        count = min(len(arr), len(self.spheres) - first)
        self._write(first, np.nan_to_num(np.clip(arr[:count], -1.0e7, 1.0e7), nan=1.0))
        self._after_update()


class PreviousCameraNotSnapshotted(MC.Model):
    """mrt_temporal_step keeps the previous camera of the first step since the history was dropped"""
    def temporal_step(self):
        keep = None if self.cleared else self.prev_cam
        super().temporal_step()
        if keep is not None:
            self.prev_cam = keep


class RegroupMarksNothingButDropsTheSnapshot(MC.Model):
    """mrt_regroup_spheres re-creates "previous" from the spheres as they are: the next step sees no motion"""
    def regroup_spheres(self):
        super().regroup_spheres()
        self.prev_xyzr = self.xyzr()


DEFECTS = [GuidesNotStaleAfterUpdate, UpdateDropsHistory, HistoryKeptAcrossSetWorld, FrameTakesTheNextGeometry, ResetClearsHistory,
           RefusedUpdateApplied, PreviousCameraNotSnapshotted, RegroupMarksNothingButDropsTheSnapshot]


def test_the_correct_model_passes_its_own_runner(reference_runs):
    assert len(reference_runs) == len(MC.SUITE_CASES)


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda c: c.__name__)
def test_the_runner_catches_a_defective_stand_in(oracle, defect):
    caught = []
    for case in MC.SUITE_CASES:
        p, _ = MC.chain(case)
        try:
            MC.run(case, MC.new_model(oracle, p, defect), MC.new_model(oracle, p), oracle)
        except MC.ChainMismatch:
            caught.append(case)
        if len(caught) >= 2:
            break
    assert len(caught) >= 2, (defect.__name__, caught)


# ------------------------------------------------------------------ ... and a defective decision model

class FollowsTheRule(MC.Model):
    """A stand-in for the implementation that reports which table its last launch got, by the true rule (its own CameraTables,
    driven by the calls it receives: every render of these chains is a launch per frame)"""

    def __init__(self, O, max_w):
        self.cam_tables, self.cam_last, self.cam_slots = MC.CameraTables(), (False, False), 2
        super().__init__(O, max_w)

    def _small(self):
        return len(self.spheres) == len(MC.layout_scene("small"))

    def set_world(self, spheres):
        super().set_world(spheres)
        self.cam_tables.call("set_world")

    def update_spheres(self, first, xyzr):
        super().update_spheres(first, xyzr)     # (a refused one raises before this)
        if len(xyzr):
            self.cam_tables.call("update_spheres")

    def regroup_spheres(self):
        super().regroup_spheres()
        self.cam_tables.call("regroup_spheres")

    def set_camera(self, cam):
        super().set_camera(cam)
        if cam is not None:
            self.cam_tables.call("set_camera")

    def debug_set_camera_masks(self, on):
        self.cam_tables.mode = int(on)

    def debug_set_frames_in_flight(self, slots):
        self.cam_slots = slots or 2

    def render(self, frames=1):
        super().render(frames)
        for _ in range(frames):
            self.cam_last = self.cam_tables.launch(self._small(), self.cam_slots, MC.SPP)

    def debug_read_camera_masks(self, table=True):
        in_force, lists = self.cam_last
        return dict(in_force=in_force, lists=bool(lists), built=False, masks=None)


class CameraChangeLeavesTheTable(MC.CameraTables):
    """a camera change does not make the table stale"""
    def stale_after(self, call):
        return call != "set_camera" and super().stale_after(call)


class EverySlotBuiltOnceAnyIs(MC.CameraTables):
    """every slot counts as built once any slot is: the slots' records are not read against the generation"""
    def slot_has_built(self, slot):
        return bool(self.slot_gen)


def test_the_correct_decision_model_agrees_with_the_stand_in(oracle):
    for case in (1, 12):
        p, _ = MC.chain(case)
        run = MC.run(case, MC.new_model(oracle, p, FollowsTheRule), MC.new_model(oracle, p), oracle)
        assert len(run.stats["list launches"]) == len(run.stats["predicted launches"]) >= 8


@pytest.mark.parametrize("defect", [CameraChangeLeavesTheTable, EverySlotBuiltOnceAnyIs], ids=lambda c: c.__name__)
def test_the_runner_catches_a_defective_decision_model(oracle, defect):
    caught = []
    for case in (0, 1, 2, 3) + LIST_CASES:
        p, _ = MC.chain(case)
        try:
            MC.run(case, MC.new_model(oracle, p, FollowsTheRule), MC.new_model(oracle, p), oracle, tables=defect)
        except MC.ChainMismatch as e:
            assert "the calls say" in str(e), e
            caught.append(case)
        if len(caught) >= 2:
            break
    assert len(caught) >= 2, (defect.__name__, caught)


@pytest.mark.parametrize("status", [MC.HIP, MC.STALLED])
def test_a_hip_error_or_a_stalled_wait_from_a_read_back_stops_the_chain(oracle, mrt, status):
    """not only the ops' own calls: the runner's read-backs and diagnostics on a real context raise ChainStopped too (which the
    GPU tests turn into pytest.exit), here from the first one a chain makes -- the hierarchy read behind mrt_set_world"""
    class Faulted(MC.Model):
        _ctx = 1                                # (what the runner takes for a real context)

        def debug_read_hierarchy(self):
            raise mrt.MrtError(status, "mrt_debug_read_hierarchy", "injected")

    p, _ = MC.chain(0)
    with pytest.raises(MC.ChainStopped):
        MC.run(0, MC.new_model(oracle, p, Faulted), MC.new_model(oracle, p), oracle)
