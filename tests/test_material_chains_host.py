"""Host tests of the material chains (tests/material_chains.py), as tests/test_motion_chains_host.py is for the motion chains:
the chains cover what they exist for; run model against model they meet the conditions without which the GPU tests would pass
vacuously (pixels that restart under the flag, pixels that keep their history beside them); and the runner reports every seeded
defect of a stand-in's update_materials."""
import numpy as np
import pytest

import material_chains as XC
import motion_chains as MC


def test_the_chains_cover_the_edits_the_flag_and_both_layouts():
    kinds, flagged, layouts = set(), 0, set()
    for name in XC.NAMES:
        p, ops = XC.CHAINS[name]
        layouts.add(p["layout"])
        assert 25 <= len(ops) <= 40 and ops[0] == ("set_world", p["layout"]) and ops[-1] == ("check",), (name, len(ops))
        assert p["max_w"] == (0.0 if any(op[0] == "set_temporal" for op in ops) else 1.0)
        mats = [op for op in ops if op[0] == "materials"]
        assert len(mats) >= 5 and {op[0] for op in ops} & {"update", "regroup", "set_camera", "reset"} == {"update", "regroup", "set_camera", "reset"}, name
        kinds |= {op[1] for op in mats}
        flagged += sum(op[3] for op in mats)
        assert {op[0] for op in ops} <= set(MC.VOCABULARY) | {"materials", "refused_materials"}
    assert kinds == set(XC.MATERIAL_KINDS) and flagged >= 6 and layouts == {"small", "large-quad"}
    assert sum(any(op[0] == "refused_materials" for op in XC.CHAINS[n][1]) for n in XC.NAMES) >= 2
    # an edit straight behind a regroup and one straight behind a geometry update, no frame between
    joined = [op[0] for n in XC.NAMES for op in XC.CHAINS[n][1]]
    pairs = set(zip(joined, joined[1:]))
    assert {("regroup", "materials"), ("update", "materials"), ("materials", "update"), ("materials", "check")} <= pairs


@pytest.fixture(scope="module")
def reference_runs(oracle):
    out = {}
    for name in XC.NAMES:
        restarts = []

        def after(i, op, run):
            m = run.model
            if op[0] == "materials" and op[3]:
                assert np.isnan(m.prev_xyzr[:, 3]).any()
                restarts.append(len(m.found))
            if op[0] == "temporal_step":
                assert not np.isnan(m.prev_xyzr).any()
        run = XC.run(name, XC.new_model(oracle, name), XC.new_model(oracle, name), oracle, after=after)
        out[name] = (run, restarts)
    return out


def test_the_correct_model_passes_its_own_runner(reference_runs):
    assert set(reference_runs) == set(XC.NAMES)
    for name, (run, _) in reference_runs.items():
        assert run.stats[(XC.CHAINS[name][0]["layout"], "checks")] >= 3
        types = run.model.spheres["material_ty"]
        assert (types == 7).any() and {1, 2, 3} <= set(types.tolist()), name


def test_the_flag_restarts_some_pixels_and_leaves_others(reference_runs):
    """at the step behind a flagged edit some pixels find no history and others do -- except right behind a dropped history"""
    seen = 0
    for name, (run, restarts) in reference_runs.items():
        found = run.model.found
        for k in restarts:
            first, f, n = found[k]
            if first:
                continue
            assert 0 < f <= n, (name, k, found)         # (a one-sphere edit may show in no pixel)
            seen += f < n
    assert seen >= 4


class GuidesNotStaleAfterMaterials(XC.Model):
    """mrt_update_materials forgets to mark the guides stale: the albedo guide is the old materials'"""
    def _after_materials(self, first, count, restart_history):
        keep = self.guides_stale
        super()._after_materials(first, count, restart_history)
        self.guides_stale = keep


class FlagIgnored(XC.Model):
    """MRT_MATERIALS_RESTART_HISTORY does nothing"""
    def _after_materials(self, first, count, restart_history):
        super()._after_materials(first, count, False)


class AlwaysRestarts(XC.Model):
    """every edit restarts the history of its spheres, flag or not"""
    def _after_materials(self, first, count, restart_history):
        super()._after_materials(first, count, True)


class EditDropsTheWholeHistory(XC.Model):
    """a material edit drops the temporal history, as mrt_set_world does"""
    def _after_materials(self, first, count, restart_history):
        super()._after_materials(first, count, restart_history)
        self._drop_history()


class PreviousNotRestored(XC.Model):
    """the NaN stays in "previous": the spheres of a flagged edit never find history again"""
    def temporal_step(self):
        nan = None if self.prev_xyzr is None else np.isnan(self.prev_xyzr[:, 3])
        super().temporal_step()
        if nan is not None and nan.any():
            self.prev_xyzr = self.prev_xyzr.copy()
            self.prev_xyzr[nan, 3] = np.nan


class FrameTakesTheNextMaterials(XC.Model):
    """an edit overtakes the frame queued before it"""
    def _after_materials(self, first, count, restart_history):
        super()._after_materials(first, count, restart_history)
        if self.frames:
            _, cam_raw, key = self.frames[-1]
            self.frames[-1] = (self.spheres, cam_raw, (MC._key(self.spheres), key[1]))
            del self.done[len(self.frames) - 1:]


class RefusedEditApplied(XC.Model):
    """a refused mrt_update_materials has written the spheres of its range that exist"""
    def update_materials(self, first, materials, restart_history=False):
        try:
            super().update_materials(first, materials, restart_history)
        except MC.Refused:
            count = len(self.spheres) - first
            new = np.array(materials[:count], copy=True)
            new["albedo"] = 0.123
            super().update_materials(first, new, restart_history)
            raise


class OffByOneRange(XC.Model):
    """the scatter writes one sphere too few"""
    def update_materials(self, first, materials, restart_history=False):
        if first + len(materials) <= len(self.spheres) and len(materials) > 1:
            materials = materials[:-1]
        super().update_materials(first, materials, restart_history)


DEFECTS = [GuidesNotStaleAfterMaterials, FlagIgnored, AlwaysRestarts, EditDropsTheWholeHistory, PreviousNotRestored,
           FrameTakesTheNextMaterials, RefusedEditApplied, OffByOneRange]


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda c: c.__name__)
def test_the_runner_catches_a_defective_stand_in(oracle, defect):
    caught = []
    for name in XC.NAMES:
        try:
            XC.run(name, XC.new_model(oracle, name, defect), XC.new_model(oracle, name), oracle)
        except MC.ChainMismatch:
            caught.append(name)
    assert caught, defect.__name__
