"""Host tests of the adaptive chains (tests/adaptive_chains.py), as tests/test_motion_chains_host.py is for the motion chains: the
chains are legal and contain the twelve situations they exist for, read from their ops; the model reproduces the single-step
references (tests/state_model.py without an edit, motion_chains.Model without a subset frame, the summed-S map in its other
summation order); run model against model the chains meet the conditions without which the GPU tests would pass vacuously
(selections that are neither empty nor everything, allocations with unequal and with equal counts, diverged checks, denoises over
distinct n_t); and the runner reports every seeded defect of a stand-in, with the chains that catch it."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_chains as AC
import budget_ref
import material_chains as XC
import motion_chains as MC
import myraytracer_amd as M
import state_model

EDITS = ("update", "materials", "regroup", "set_camera", "set_world")
SUBSETS = ("subset", "adaptive", "budget")


def _ops(name):
    return AC.CHAINS[name][1]


def _diverged(ops, i):
    """a subset frame among ops[:i] since the last reset (the written-out subsets: every one lists fewer tiles than the image has)"""
    seen = False
    for op in ops[:i]:
        seen = (seen or op[0] == "subset") and op[0] != "reset"
    return seen


# ------------------------------------------------------------------ legality and coverage

def test_shape_vocabulary_and_checks():
    names, sizes, queued = set(), [], 0
    assert 12 <= len(AC.NAMES) <= 17
    for name in AC.NAMES:
        p, ops = AC.CHAINS[name]
        assert len(ops) <= 40 and ops[0] == ("set_world", p["layout"]) and ops[-1] == ("check",), (name, len(ops))
        assert p["size"] in (AC.SMALL_IMAGE, AC.WIDE_IMAGE)
        sizes.append(p["size"])
        names |= {op[0] for op in ops}
        assert {op[0] for op in ops} <= set(MC.VOCABULARY) | set(AC.VOCABULARY), name
        edits = 0
        for op in ops[1:]:                      # a check after every third scene edit
            edits = 0 if op[0] == "check" else edits + (op[0] in EDITS)
            assert edits <= 3, (name, op)
        assert ("set_frames_in_flight", 0) not in ops
        queued += ("set_frame_batching", 0) in ops and any(op in ops for op in (("set_frames_in_flight", 4), ("set_frames_in_flight", 8)))
        first_subset = min(i for i, op in enumerate(ops) if op[0] == "subset")
        assert all(i < first_subset for i, op in enumerate(ops) if op == ("set_frame_batching", 0)), name     # (the situations queue behind it)
    assert set(AC.VOCABULARY) <= names
    assert sizes.count(AC.WIDE_IMAGE) >= 2 and sizes.count(AC.SMALL_IMAGE) >= 2
    assert 2 * queued >= len(AC.NAMES), queued
    assert {op[1] for n in AC.NAMES for op in _ops(n) if op[0] == "refuse"} == set(AC.REFUSALS)
    assert {AC.CHAINS[n][0]["layout"] for n in AC.NAMES} == {"small", "large-quad"}


def _windows(ops, pattern):
    """the indices at which the ops' names run through `pattern`"""
    names = [op[0] for op in ops]
    return [i for i in range(len(ops) - len(pattern) + 1) if names[i:i + len(pattern)] == list(pattern)]


def _situations(chains):
    """the twelve situations read from the ops of `chains` (name or case -> (params, ops)): which chains hold each, and the
    kinds, modes and weights that the conditions on them name"""
    found = {k: [] for k in range(1, 13)}
    kinds_1, kinds_3, denoise_6, long_6 = set(), set(), set(), []
    for n, (p, ops) in chains.items():
        n = str(n)
        # 1: subset, update, subset, update, render(2), ..., check, behind the divergence
        for i in _windows(ops, ("subset", "update", "subset", "update", "render")):
            if ops[i + 4][1] >= 2 and _diverged(ops, i + 1):
                found[1].append(n)
        kinds_1 |= {op[1] for i, op in enumerate(ops) if op[0] == "update" and _diverged(ops, i)}
        # 2: a regroup and the policy with ratio 1 at every update, subset frames on both sides
        names = [op[0] for op in ops]
        for i, op in enumerate(ops):
            sides = "subset" in names[max(i - 3, 0):i] and "subset" in names[i + 1:i + 4]
            if op[0] == "regroup" and sides and any(o == ("auto_regroup", True, 1.0, 1) for o in ops) and p["layout"] == "small":
                found[2].append(n)
            # 3: every kind of material edit between subset frames
            if op[0] == "materials" and sides and _diverged(ops, i):
                kinds_3.add(op[1])
        if any(ops[i][3] for i in _windows(ops, ("materials", "temporal_step"))):
            found[3].append(n)
        # 4: a camera and a scene of another sphere count on a diverged accumulation, frames and a report behind them, no reset
        cam = [i for i, op in enumerate(ops) if op[0] == "set_camera" and _diverged(ops, i)]
        world = [i for i, op in enumerate(ops) if op[0] == "set_world" and op[1] != p["layout"] and _diverged(ops, i)]
        if cam and world and not any(op[0] == "reset" for op in ops) and any(op[0] == "query" for op in ops[world[0]:]):
            found[4].append(n)
        # 5: steps behind subset frames, both orders of update and subset, the image read and presented
        if (any(op[0] == "set_temporal" for op in ops) and _windows(ops, ("subset", "temporal_step")) and
                _windows(ops, ("update", "subset", "temporal_step")) and _windows(ops, ("subset", "update", "temporal_step")) and
                ("read_temporal",) in ops and ("present", "temporal") in ops):
            found[5].append((n, p["max_w"]))
        # 6: the per-tile denoise by mode and blend; behind an update and a material edit; behind the long runs; presented
        mode, mix, on = 0, False, False
        for i, op in enumerate(ops):
            if op[0] == "denoise_variance":
                mode = op[1]
            if op[0] == "denoise_mix":
                mix = op[1]
            if op[0] == "denoise_adaptive":
                on = op[1]
            if op[0] == "read_denoised" and on and _diverged(ops, i):
                denoise_6.add((mode, mix))
        if _windows(ops, ("update", "read_denoised")) and _windows(ops, ("materials", "read_denoised")) and ("present", "denoised") in ops:
            found[6].append(n)
        runs = [i for i, op in enumerate(ops) if op[0] == "subset" and op[2] > AC.K_TABLE_FIRST and len(op[1]) == 1]
        if len(runs) >= 2 and len({ops[i][1] for i in runs}) == 1 and all(ops[i + 1] == ("read_denoised",) for i in runs):
            long_6.append(n)
        # 7: reports of both kinds on both sides of an edit; a selection and an allocation from a report older than an edit; the ring
        seq, edit_seq, kinds_before, kinds_after, old = 0, None, set(), set(), set()
        for i, op in enumerate(ops):
            if op[0] == "query":
                seq += 1
                (kinds_before if edit_seq is None else kinds_after).add(op[3])
            if op[0] in ("update", "materials") and seq and edit_seq is None:
                edit_seq = seq
            if op[0] in ("adaptive", "budget") and edit_seq is not None and op[-1] <= edit_seq:
                old.add(op[0])
        # (the refusal names the first of the nine: report 8 back from the newest, the one a ring of 9 would still hold)
        nine = any(ops[i + 9] == ("refuse", "old-report", sum(o[0] == "query" for o in ops[:i + 1]))
                   for i in _windows(ops, ("query",) * 9) if i + 9 < len(ops))
        if kinds_before == kinds_after == {"max_rel", "sum_s"} and old == {"adaptive", "budget"}:
            found[7].append(n)
        if nine:
            found[7].append(n + " (nine)")
        # 8: the masks forced, then the lists: subset launches under generations of all three kinds
        gens = {2: set(), 3: set()}
        mode, last = None, None
        for op in ops:
            if op[0] == "set_camera_masks":
                mode, last = op[1], None
            if op[0] in ("update", "regroup", "set_camera"):
                last = op[0]
            if op[0] == "subset" and mode in gens and last:
                gens[mode].add(last)
        if all(v == {"update", "regroup", "set_camera"} for v in gens.values()) and ("set_frame_batching", 0) in ops:
            found[8].append(n)
        # 9: a reset of a diverged, moving chain; a denoise with the setting off accepted; divergence again
        for i, op in enumerate(ops):
            if op[0] == "reset" and _diverged(ops, i) and any(o[0] == "update" for o in ops[:i]):
                rest = ops[i + 1:]
                d = [j for j, o in enumerate(rest) if o == ("read_denoised",)]
                s = [j for j, o in enumerate(rest) if o[0] == "subset"]
                if d and s and d[0] < s[0] and not any(o[0] == "denoise_adaptive" for o in ops[:i + 1 + d[0]]):
                    found[9].append(n)
        # 10: spp between subset frames; counter mode at 64 by tiles, 65 refused
        if (any(ops[i + 1][1] != MC.SPP for i in _windows(ops, ("subset", "spp", "subset"))) and
                any(ops[i] == ("rng_mode", 1) and ops[i + 1] == ("spp", 64) for i in _windows(ops, ("rng_mode", "spp", "subset"))) and
                any(ops[i] == ("spp", 65) and ops[i + 1] == ("refuse", "counter-65") for i in _windows(ops, ("spp", "refuse", "check")))):
            found[10].append(n)
        # 11: batched whole frames behind an update, after the divergence, in both forms
        forms = {ops[i][1] for i in _windows(ops, ("set_frame_batching", "update", "render")) if ops[i + 2][1] >= 2 and _diverged(ops, i)}
        if forms == {2, 3}:
            found[11].append(n)
        # 12: the large layout through 1, 2, 5 and 6
        if (p["layout"] == "large-quad" and _windows(ops, ("subset", "update", "subset")) and "regroup" in names and
                ("auto_regroup", True, 1.0, 1) in ops and _windows(ops, ("subset", "temporal_step")) and "read_denoised" in names):
            found[12].append(n)
    return found, kinds_1, kinds_3, denoise_6, long_6


def test_every_situation_is_present():
    found, kinds_1, kinds_3, denoise_6, long_6 = _situations({n: AC.CHAINS[n] for n in AC.NAMES})
    assert kinds_1 >= {"jitter", "scatter", "partial", "shrink", "ground"} and kinds_3 == set(XC.MATERIAL_KINDS), (kinds_1, kinds_3)
    assert denoise_6 == {(m, x) for m in (0, 1, 2) for x in (False, True)}, denoise_6
    assert long_6 and {w for _, w in found[5]} == {0.0, 0.75}, (long_6, found[5])
    assert any("(nine)" in n for n in found[7]) and any("(nine)" not in n for n in found[7]), found[7]
    assert all(found.values()), found


def test_every_chain_is_legal(oracle):
    """the model accepts every call but the ones a chain draws as refusals, and refuses those for the one reason drawn"""
    status = {"denoise-off": MC.STATE, "adaptive-on-sums": MC.STATE, "budget-on-max-rel": MC.STATE, "old-report": MC.STATE,
              "duplicate-tile": MC.INVALID_ARG, "counter-65": MC.INVALID_ARG, "present-temporal-dropped": MC.STATE,
              **dict.fromkeys(AC.RESPONSE_REFUSALS, MC.INVALID_ARG)}
    assert status == AC.REFUSAL_STATUS
    for name in AC.NAMES:
        m, sh = AC.new_model(oracle, name), AC.Shadow()
        for op in _ops(name):
            before = m.temporal_response()
            for call, args in sh.calls(op):
                got, _ = MC._call(m, call, args)
                assert got == (status[op[1]] if op[0] == "refuse" else MC.OK), (name, op, call, got)
            if op[0] == "refuse":               # one reason at a time: the state allows the call, only the reason drawn does not
                if op[1] in AC.RESPONSE_REFUSALS:
                    assert m.temporal_response() == before == (sh.response[0], dict(zip(("fast_history", "clamp_sigma", "antilag"), sh.response[1:])))
                if op[1] == "present-temporal-dropped":
                    assert m.temporal_on and m.spheres is not None and not m.stepped
                if op[1] in ("adaptive-on-sums", "budget-on-max-rel"):
                    assert m._oldest() <= op[2] <= m.noise_seq
                if op[1] == "old-report":
                    assert m.reports.get(op[2]) is None and op[2] < m._oldest() and m.tracking
                if op[1] == "denoise-off":
                    assert m.tracking and m.acc.diverged and not m.denoise_adaptive_on
                if op[1] == "counter-65":
                    assert (m.rng_mode, m.spp) == (1, 65)


# ------------------------------------------------------------------ the reference runs and their conditions

@pytest.fixture(scope="module")
def reference_runs(oracle):
    out = {}
    for name in AC.NAMES:
        seen = {"checks": [], "maps": []}

        def after(i, op, run, seen=seen):
            m = run.model
            if op[0] == "check":
                seen["checks"].append(bool(m.acc.diverged))
            if op[0] == "query" and op[3] == "sum_s":
                seen["maps"].append((m.reports[m.noise_seq]["map"].copy(), m.acc.S.copy(), m.acc.fb.copy()))
        out[name] = (AC.run(name, AC.new_model(oracle, name), AC.new_model(oracle, name), oracle, after=after), seen)
    return out


def test_the_reference_meets_the_conditions(reference_runs):
    partial, unequal, equal = 0, 0, 0
    for name, (run, seen) in reference_runs.items():
        m = run.model
        checks = sum(v for k, v in run.stats.items() if isinstance(k, tuple) and k[1] == "checks")      # (per layout: a chain may change its scene)
        assert checks == len(seen["checks"]) == sum(op == ("check",) for op in _ops(name))
        assert 2 * sum(seen["checks"]) >= len(seen["checks"]), (name, seen["checks"])
        assert run.stats["diverged checks"] == sum(seen["checks"])
        partial += sum(0 < n < tiles for n, tiles in m.selections)
        unequal += sum(len(set(k.tolist())) > 1 for k in m.allocations)
        equal += sum(len(set(k.tolist())) == 1 and k[0] > 0 for k in m.allocations)
        for counts in m.denoises:               # (every per-tile denoise: a read, a present, a check's)
            assert len(set(counts.tolist())) >= 2 and counts.max() >= 2, (name, counts)
    print(f"selections neither empty nor everything: {partial}; allocations with unequal counts: {unequal}, with equal counts: {equal}")
    assert partial >= 6 and unequal >= 6 and equal >= 1
    # the device's table of K(n) (ensure_k_table: made for the largest n_t + 1, 4096 entries at first, doubled until it fits): both
    # kinds of consumer meet the first table, then consumers that need 8192 entries, then consumers that need 16384, in that
    # order -- so that a table queued work has read is replaced twice
    first = AC.K_TABLE_FIRST
    needs = [(kind, first if n + 1 <= first else 2 * first if n + 1 <= 2 * first else 4 * first) for kind, n in
             reference_runs["denoise-long"][0].model.k_consumers]
    sizes = [size for _, size in needs]
    assert sizes == sorted(sizes) and set(sizes) == {first, 2 * first, 4 * first}, needs
    assert {kind for kind, size in needs if size == first} == {"denoise", "query"}, needs
    assert all({kind for kind, size in needs if size == s} >= {"denoise"} for s in (2 * first, 4 * first)), needs
    assert max(n for _, n in reference_runs["denoise-long"][0].model.k_consumers) + 1 <= 4 * first


def test_the_calls_alone_put_both_tables_in_force_under_subset_launches(reference_runs):
    """motion_chains.CameraTables' prediction for the chain that forces the tables: subset launches with the masks under three or
    more generations, then with the lists under three or more, 4 or more frames in flight (the GPU test asserts it of the device)"""
    launches = reference_runs["tables"][0].stats["subset predicted launches"]
    masks = {gen for gen, on, lists, fif in launches if on and lists is False and fif >= 4}
    lists = {gen for gen, on, lists, fif in launches if on and lists is True and fif >= 4}
    assert len(masks) >= 3 and len(lists) >= 3, launches
    for name, (run, _) in reference_runs.items():       # the prediction goes on to the end wherever every launch is one frame
        assert run.tables_lost == (("set_frame_batching", 0) not in _ops(name)), name


def test_the_summed_s_map_in_the_other_order(reference_runs):
    """on the chains' own S -- a few binades, nothing to cancel -- the tile sums taken row-major, one after the other, round to the
    same floats: the model's map is no artefact of the order budget_ref.tile_sums adds in (the fixture that tells the orders apart
    is tests/test_budget_host.py's)"""
    n = ragged = 0
    for name, (_, seen) in reference_runs.items():
        for tmap, S, fb in seen["maps"]:
            assert np.array_equal(tmap.ravel().view(np.uint32), budget_ref.tile_sums_row_major(S, fb).view(np.uint32)), name
            ragged += bool((tmap[:, -1] > 0).all() and (tmap[-1] > 0).all())      # the ragged column and band hold something
            n += 1
    assert n >= 8 and ragged >= 8


# ------------------------------------------------------------------ the model against the single-step references

def test_without_an_edit_the_model_is_state_model(oracle):
    w, h = AC.WIDE_IMAGE
    a = AC.Model(oracle, 0.75, w, h)
    b = state_model.Model(oracle, M._lib.load(), M.Args(w, h, MC.SPP, MC.DEPTH, 0.75), MC.SEED)
    sh = AC.Shadow()
    for name, args in sh.calls(("set_world", "small")):
        if name != "debug_set_hierarchy":
            getattr(a, name)(*args)
            getattr(b, name)(*args)
    for m in (a, b):
        m.set_noise_tracking(True)
    steps = [("render", 2), ("render_tiles", (0, 7, 17), 1), ("noise_query", 0.3, 0.02), ("render", 1), ("render_tiles", (5, 11), 2),
             ("noise_query", 0.2, 0.02), ("render_adaptive", 2, 2), ("render_adaptive", 1, 1), ("render", 2), ("noise_query", 0.1, 0.05)]
    for name, *args in steps:
        ra, rb = getattr(a, name)(*args), getattr(b, name)(*args)
        assert ra == rb, (name, ra, rb)
        for f in ("read_framebuffer", "read_noise", "tile_frames"):
            assert MC._same(getattr(a, f)(), getattr(b, f)()), (name, args, f)
        assert a.read_counters() == b.read_counters() and a.frames_done == b.frames_done
        if name == "noise_query":
            assert a.noise_result() == b.noise_result() and MC._same(a.read_noise_tiles(), b.read_noise_tiles())
    assert a.acc.diverged and len(set(a.acc.n.tolist())) >= 3


def test_without_a_subset_frame_the_model_is_the_motion_model(oracle):
    for max_w in (1.0, 0.75, 0.0):
        a, b = AC.Model(oracle, max_w), XC.Model(oracle, max_w)
        sh = AC.Shadow()
        ops = [("set_world", "small"), ("render", 2), ("update", "jitter", 5), ("render", 1), ("set_camera", 0.2, 12.0, 2.0), ("render", 2),
               ("materials", "types", 6, False), ("render", 1), ("reset",), ("update", "partial", 7), ("render", 2)]
        for op in ops:
            for name, args in sh.calls(op):
                getattr(a, name)(*args)
                getattr(b, name)(*args)
            assert MC._same(a.read_framebuffer(), b.read_framebuffer()), (max_w, op)
            assert a.read_counters() == b.read_counters() and a.frames_done == b.frames_done
        assert not a.acc.diverged and (a.tile_frames() == a.frames_done).all()


# ------------------------------------------------------------------ seeded defects

class _Remembers(AC.Model):
    """keeps what the last update, camera change and material edit replaced"""
    old_spheres = old_cam = old_materials = None

    def _write(self, first, arr):
        self.old_spheres = self.spheres
        super()._write(first, arr)

    def set_camera(self, cam):
        if getattr(self, "cam_raw", None) is not None:
            self.old_cam = (self.cam_raw, self.cam_key)
        super().set_camera(cam)

    def update_materials(self, first, materials, restart_history=False):
        self.old_materials = self.spheres
        super().update_materials(first, materials, restart_history)


class SubsetTakesTheSceneBeforeTheUpdate(_Remembers):
    """a subset frame is rendered with the spheres from before the last mrt_update_spheres"""
    def _frame_inputs(self, tiles):
        s, c, k = super()._frame_inputs(tiles)
        if tiles is not None and self.old_spheres is not None and len(self.old_spheres) == len(s):
            old = self.old_spheres.copy()
            for f in M.MATERIAL_DTYPE.names:
                old[f] = s[f]
            s = old
        return s, c, k


class SubsetTakesTheCameraBeforeTheChange(_Remembers):
    """... with the camera from before the last mrt_set_camera"""
    def _frame_inputs(self, tiles):
        s, c, k = super()._frame_inputs(tiles)
        return (s,) + (self.old_cam if tiles is not None and self.old_cam is not None else (c, k))


class SubsetTakesTheMaterialsBeforeTheEdit(_Remembers):
    """... with the materials from before the last mrt_update_materials"""
    def _frame_inputs(self, tiles):
        s, c, k = super()._frame_inputs(tiles)
        if tiles is not None and self.old_materials is not None and len(self.old_materials) == len(s):
            s = s.copy()
            for f in M.MATERIAL_DTYPE.names:
                s[f] = self.old_materials[f]
        return s, c, k


class LastFrameOfABatchNotCounted(AC.Model):
    """the n_t of the listed tiles misses the last frame of a batch"""
    def _counted(self, tiles, frames):
        if frames >= 2:
            self.acc.n[np.asarray(tiles)] -= 1


class WholeFrameAtTheUniformWeight(AC.Model):
    """a whole frame after the divergence is blended at frames_done's weight in every tile"""
    def _blend(self, mean, tiles):
        if tiles is None and self.acc.diverged:
            keep = self.acc.n.copy()
            self.acc.n[:] = self.acc.frames_done
            super()._blend(mean, tiles)
            self.acc.n[:] = keep + 1
        else:
            super()._blend(mean, tiles)


class _ForgetsTheGuides(AC.Model):
    """an update does not mark the guides stale for one consumer; every other consumer finds them stale"""
    consumer, owed = None, False

    def _after_update(self):
        keep = self.guides_stale
        super()._after_update()
        self.guides_stale, self.owed = keep, True

    def _guides_for(self, consumer):
        forgets = consumer == self.consumer and (consumer != "step" or self.acc.diverged)
        if self.owed and not forgets:
            self.guides_stale, self.owed = True, False
        return super()._guides_for(consumer)


class TileDenoiseKeepsStaleGuides(_ForgetsTheGuides):
    """... when the next consumer is the per-tile denoise"""
    consumer = "denoise-tiles"


class StepOnADivergedAccumulationKeepsStaleGuides(_ForgetsTheGuides):
    """... when the next consumer is a temporal step on a diverged accumulation"""
    consumer = "step"


class DenoiseTakesKOfFramesDone(AC.Model):
    """the per-tile denoise takes K(frames_done) for every tile"""
    def _denoise_counts(self):
        return np.full_like(self.acc.tile_frames(), self.acc.frames_done)


class SumMapSkipsTheRaggedColumn(AC.Model):
    """the summed-S map leaves the ragged last column of tiles at 0"""
    def _sum_map(self):
        m = super()._sum_map()
        if self.w % 8:
            m[:, -1] = 0
        return m


class BudgetTakesTheNewestReport(AC.Model):
    """mrt_render_budget allocates from the newest summed-S report instead of the one named"""
    def _budget_report(self, seq):
        return self.reports[max(s for s, r in self.reports.items() if r["kind"] == "sum_s")]


class ResetLeavesTheDivergence(AC.Model):
    """mrt_reset zeroes the counts but leaves the accumulation marked as diverged"""
    def reset(self):
        was = self.acc.diverged
        super().reset()
        self.acc.diverged = was


class ResponseSurvivesEnableChange(AC.Model):
    """a call that changes the response's `enabled` keeps the history"""
    def _response_enabled_changed(self):
        pass


class FastHistoryNotZeroedAfterDrop(AC.Model):
    """a dropped history leaves the H2 the next step reads as it was"""
    def _h2_after_drop(self):
        return self.h2 if self.h2 is not None else super()._h2_after_drop()


class AntilagRoundsTheLength(AC.Model):
    """4c stores N'' rounded to an integer"""
    def _stored_length(self, h0):
        h0 = h0.copy()
        h0[..., 3] = np.rint(h0[..., 3])
        return h0


class ClampCountsOtherSpheres(AC.Model):
    """4b counts a window tap whatever sphere its H1' names"""
    def _clamp_indices(self, h1):
        h1 = h1.copy()
        h1[..., 3] = 0.0
        return h1


RESPONSE_DEFECTS = [ResponseSurvivesEnableChange, FastHistoryNotZeroedAfterDrop, AntilagRoundsTheLength, ClampCountsOtherSpheres]
DEFECTS = RESPONSE_DEFECTS + [SubsetTakesTheSceneBeforeTheUpdate, SubsetTakesTheCameraBeforeTheChange, SubsetTakesTheMaterialsBeforeTheEdit,
           LastFrameOfABatchNotCounted, WholeFrameAtTheUniformWeight, TileDenoiseKeepsStaleGuides,
           StepOnADivergedAccumulationKeepsStaleGuides, DenoiseTakesKOfFramesDone, SumMapSkipsTheRaggedColumn, BudgetTakesTheNewestReport,
           ResetLeavesTheDivergence]
# the chains that report each defect (run with the defective stand-in as the implementation); the test holds the list to what it finds
_ALL = ("edits", "regroups", "materials", "two-pictures", "temporal-0", "temporal-075", "denoise", "denoise-long", "reports", "ring", "tables",
        "reset", "spp-rng", "batched", "large")
CAUGHT_BY = {
    "SubsetTakesTheSceneBeforeTheUpdate": [n for n in _ALL if n not in ("materials", "two-pictures", "denoise-long")],
    "SubsetTakesTheCameraBeforeTheChange": list(_ALL),      # (every chain sets a camera behind its scene: "before" is the pinhole)
    "SubsetTakesTheMaterialsBeforeTheEdit": ["materials", "temporal-075", "denoise", "reports"],
    "LastFrameOfABatchNotCounted": ["two-pictures", "temporal-075", "denoise-long", "reports", "ring", "batched", "large"],
    "WholeFrameAtTheUniformWeight": ["edits", "regroups", "materials", "two-pictures", "temporal-075", "reports", "tables", "spp-rng", "batched"],
    "TileDenoiseKeepsStaleGuides": ["denoise", "denoise-long", "reset"],
    "StepOnADivergedAccumulationKeepsStaleGuides": ["temporal-0", "temporal-075", "large"],
    "DenoiseTakesKOfFramesDone": ["denoise", "denoise-long", "reset", "large"],
    "SumMapSkipsTheRaggedColumn": ["edits", "regroups", "two-pictures", "denoise-long", "reports", "ring", "batched"],
    "BudgetTakesTheNewestReport": ["reports"],
    "ResetLeavesTheDivergence": ["reset"],
}

# ... and the two written chains with the response on, behind the fifteen the lists above were recorded on
for _defect, _more in {"SubsetTakesTheSceneBeforeTheUpdate": ["response-0", "response-large"],
                       "SubsetTakesTheCameraBeforeTheChange": ["response-0", "response-large"],
                       "SubsetTakesTheMaterialsBeforeTheEdit": ["response-0"], "LastFrameOfABatchNotCounted": ["response-large"],
                       "WholeFrameAtTheUniformWeight": ["response-large"],
                       "StepOnADivergedAccumulationKeepsStaleGuides": ["response-0", "response-large"],
                       "DenoiseTakesKOfFramesDone": ["response-large"]}.items():
    CAUGHT_BY[_defect] = CAUGHT_BY[_defect] + _more
CAUGHT_BY.update({"ResponseSurvivesEnableChange": ["response-0"], "FastHistoryNotZeroedAfterDrop": ["response-0"],
                  "AntilagRoundsTheLength": ["response-0", "response-large"], "ClampCountsOtherSpheres": ["response-0", "response-large"]})
# The random chains (AC.SUITE_CASES) that report each defect.  The response's: every case that does, of the cases that set the
# response at all (no other can); the others': the first case that does, in the suite's order
SUITE_CAUGHT_BY = {"ResponseSurvivesEnableChange": [2, 7, 8, 13, 19, 20], "FastHistoryNotZeroedAfterDrop": [2, 7, 8, 13, 19, 20],
                   "AntilagRoundsTheLength": [1, 14, 20], "ClampCountsOtherSpheres": [1, 2, 7, 8, 13, 14, 19, 20]}
SUITE_FIRST_CATCH = {"SubsetTakesTheSceneBeforeTheUpdate": 0, "SubsetTakesTheCameraBeforeTheChange": 0,
                     "SubsetTakesTheMaterialsBeforeTheEdit": 3, "LastFrameOfABatchNotCounted": 0, "WholeFrameAtTheUniformWeight": 0,
                     "TileDenoiseKeepsStaleGuides": 3, "StepOnADivergedAccumulationKeepsStaleGuides": 1, "DenoiseTakesKOfFramesDone": 2,
                     "SumMapSkipsTheRaggedColumn": 0, "BudgetTakesTheNewestReport": 0, "ResetLeavesTheDivergence": 6}


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda c: c.__name__)
def test_the_runner_catches_a_defective_stand_in(oracle, defect):
    caught = []
    for name in AC.NAMES:
        try:
            AC.run(name, AC.new_model(oracle, name, defect), AC.new_model(oracle, name), oracle)
        except MC.ChainMismatch:
            caught.append(name)
    print(f"{defect.__name__}: caught by {caught}")
    assert caught, defect.__name__
    assert caught == CAUGHT_BY[defect.__name__], (defect.__name__, caught)


# ------------------------------------------------------------------ the random chains (adaptive_chains.chain, SUITE_CASES)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adaptive_chain_cases.json")
# the situations of the written chains that no random chain holds, and why (at most two, none of the response's)
NOT_REACHED = {"6, the long runs": "a run of 4100 subset frames stays in the written chain denoise-long",
               "7, nine queries in a row": "with the refusal behind them they are ten ops, and the generator checks at least every 8"}


def _suite():
    return {c: AC.chain(c) for c in AC.SUITE_CASES}


def _response_windows(ops):
    """(steps with the response on right behind a subset frame, changes of `enabled` with a step before and a step after)"""
    on, behind, changes, stepped, pending = False, 0, 0, False, 0
    for i, op in enumerate(ops):
        if op[0] == "temporal_response":
            pending += stepped and op[1] != on
            on = op[1]
        if op[0] == "temporal_step":
            behind += on and ops[i - 1][0] == "subset"
            changes, pending, stepped = changes + pending, 0, True
    return behind, changes


def test_a_case_number_reproduces_its_chain():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert set(golden["cases"]) == {str(c) for c in AC.SUITE_CASES}
    for c, (p, ops) in _suite().items():
        assert AC.chain(c) == (p, ops)
        assert hashlib.sha256(repr(ops).encode()).hexdigest() == golden["cases"][str(c)], f"the generator changed case {c}"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join("tests", "adaptive_chains.py"), "7"], cwd=root, capture_output=True, text=True, check=True).stdout
    p, ops = AC.chain(7)
    assert out.splitlines() == [f"case 7: {p}"] + [f"{i:3d} {op!r}" for i, op in enumerate(ops)]


def test_the_plan_and_the_suite_cover_what_they_promise():
    assert len(AC.PLAN) >= 12 and {f for *_, f in AC.PLAN} == set(AC.FLAVOURS)
    for layout in ("small", "large-quad", "large-lin"):
        assert sum(l == layout for l, *_ in AC.PLAN) >= 3
    suite = _suite()
    names, refusals = dict.fromkeys(AC.UNION_VOCABULARY, 0), set()
    for c, (p, ops) in suite.items():
        assert (p["layout"], p["max_w"], p["size"], p["flavour"]) == AC.PLAN[c % len(AC.PLAN)]
        assert len(ops) <= 40 and ops[0] == ("set_world", p["layout"]) and ops[-1] == ("check",), (c, len(ops))
        assert {op[0] for op in ops} <= set(AC.UNION_VOCABULARY), c
        checks = [-1] + [i for i, op in enumerate(ops) if op == ("check",)]
        assert max(np.diff(checks)) <= 8, (c, checks)
        assert all(op[2] < AC.K_TABLE_FIRST for op in ops if op[0] == "subset"), c
        edits = 0
        for op in ops[1:]:                      # a check after every third update
            edits = 0 if op[0] == "check" else edits + (op[0] == "update")
            assert edits <= 3, (c, op)
        for n in {op[0] for op in ops}:
            names[n] += 1
        refusals |= {op[1] for op in ops if op[0] in ("refuse", "refused")} | {op[0] for op in ops if op[0] == "refused_materials"}
    assert all(v >= 3 for v in names.values()), {n: v for n, v in names.items() if v < 3}
    assert refusals == set(AC.REFUSALS) | set(MC.REFUSALS) | {"refused_materials"}
    for layout in ("small", "large-quad", "large-lin"):
        assert sum(p["layout"] == layout for p, _ in suite.values()) >= 3
    for max_w in (1.0, 0.75, 0.0):
        assert sum(p["max_w"] == max_w for p, _ in suite.values()) >= 3
    windows = {c: _response_windows(ops) for c, (_, ops) in suite.items()}
    assert sum(b > 0 for b, _ in windows.values()) >= 4 and sum(ch > 0 for _, ch in windows.values()) >= 2, windows
    # the written chains' situations, read from the random chains' ops by the same reader
    found, kinds_1, kinds_3, denoise_6, long_6 = _situations(suite)
    assert kinds_1 >= {"jitter", "scatter", "partial", "shrink", "ground"} and kinds_3 == set(XC.MATERIAL_KINDS), (kinds_1, kinds_3)
    assert denoise_6 == {(m, x) for m in (0, 1, 2) for x in (False, True)}, denoise_6
    assert {w for _, w in found[5]} == {0.0, 0.75}, found[5]
    assert all(found.values()) and any("(nine)" not in n for n in found[7]), found
    assert len(NOT_REACHED) <= 2 and not long_6 and not any("(nine)" in n for n in found[7])       # (the two listed: indeed not there)


@pytest.fixture(scope="module")
def suite_runs(oracle):
    """every random chain model against model, and on the way every call's status on a model of its own: OK but for the
    refusals drawn, and those refuse for the reason drawn"""
    out = {}
    for c, (p, ops) in _suite().items():
        m, sh = AC.new_model(oracle, c), AC.Shadow()
        for op in ops:
            before = m.temporal_response()
            for call, args in sh.calls(op):
                got, _ = MC._call(m, call, args)
                want = AC.REFUSAL_STATUS[op[1]] if op[0] == "refuse" else MC.OK if op[0] not in ("refused", "refused_materials") else None
                assert got == want or (want is None and got != MC.OK), (c, op, call, got)
            if op[0] == "refuse":               # one reason at a time
                if op[1] in ("adaptive-on-sums", "budget-on-max-rel"):
                    assert m._oldest() <= op[2] <= m.noise_seq
                if op[1] == "old-report":
                    assert 0 < op[2] < m._oldest() and m.tracking
                if op[1] == "denoise-off":
                    assert m.tracking and m.acc.diverged and not m.denoise_adaptive_on
                if op[1] == "counter-65":
                    assert (m.rng_mode, m.spp) == (1, 65)
                if op[1] in AC.RESPONSE_REFUSALS:
                    assert m.temporal_response() == before
                if op[1] == "present-temporal-dropped":
                    assert m.temporal_on and m.spheres is not None and not m.stepped
        seen = []

        def after(i, op, run, seen=seen):
            if op[0] == "check":
                seen.append(bool(run.model.acc.diverged))
        out[c] = (AC.run(c, AC.new_model(oracle, c), AC.new_model(oracle, c), oracle, after=after), seen)
    return out


def test_every_random_chain_is_legal_and_meets_the_conditions(suite_runs):
    diverged = moved = fractional = h2 = h2_dropped = 0
    for c, (run, seen) in suite_runs.items():
        assert len(seen) == sum(op == ("check",) for op in AC.chain(c)[1])
        diverged += any(seen)
        moved += sum(a > 0 for a, _ in run.model.response_steps)
        fractional += sum(b > 0 for _, b in run.model.response_steps)
        h2 += run.stats.get("h2 checks", 0)
        h2_dropped += run.stats.get("h2 checks of a dropped history", 0)
    print(f"cases with a diverged check: {diverged} of {len(suite_runs)}; steps whose clamp moved a pixel: {moved}, that stored a fractional "
          f"length: {fractional}; checks of H2: {h2}, of a dropped history's: {h2_dropped}")
    assert 2 * diverged >= len(suite_runs)
    assert moved >= 8 and fractional >= 4 and h2 >= 8 and h2_dropped >= 2


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda c: c.__name__)
def test_a_random_chain_catches_every_defect(oracle, defect):
    name = defect.__name__
    caught = []
    if defect in RESPONSE_DEFECTS:
        for c in AC.SUITE_CASES:
            if any(op[0] == "temporal_response" for op in AC.chain(c)[1]):
                try:
                    AC.run(c, AC.new_model(oracle, c, defect), AC.new_model(oracle, c), oracle)
                except MC.ChainMismatch:
                    caught.append(c)
        assert caught and caught == SUITE_CAUGHT_BY[name], (name, caught)
    else:
        for c in AC.SUITE_CASES:
            try:
                AC.run(c, AC.new_model(oracle, c, defect), AC.new_model(oracle, c), oracle)
            except MC.ChainMismatch:
                caught.append(c)
                break
        assert caught == [SUITE_FIRST_CATCH[name]], (name, caught)


# sha256 over (h0, h1, the temporal image) at every check with a history, per written chain that steps with the response never
# enabled: recorded from the model as it was before it knew the response (the parent commit's tests/motion_chains.py)
TEMPORAL_BEFORE_THE_RESPONSE = {
    "materials": (3, "bdfe641f0b6c920be1547778ff8dbee5ad12bcf563c2af60f54afcc44c6ab995"),
    "temporal-0": (3, "e131179e52b6a046b4e2cd913cd4c38e765b0eee778f9936e8b88385c373d666"),
    "temporal-075": (3, "40fa753e8171325dd42722fa21a146d0ebc458ff048d4ed877955e7660195f23"),
    "large": (3, "ccb2213094abc3a2f1188abcbf22a379ef819957aa33a1f7e1514dbb76ec5c3f"),
}


def test_with_the_response_never_enabled_the_temporal_outputs_are_what_they_were(oracle):
    for name in AC.NAMES:
        if any(op[0] == "temporal_response" for op in _ops(name)):
            continue
        h, n = hashlib.sha256(), [0]

        def after(i, op, run, h=h, n=n):
            m = run.model
            assert m.h2 is None and not m.response_steps and m.temporal_response() == (False, {"fast_history": 4, "clamp_sigma": 2.0, "antilag": 1.0})
            if op[0] == "check" and m.temporal_on and m.stepped:
                for a in (m.h0, m.h1, m.read_temporal()):
                    h.update(a.tobytes())
                n[0] += 1
        AC.run(name, AC.new_model(oracle, name), AC.new_model(oracle, name), oracle, after=after)
        assert (n[0], h.hexdigest()) == TEMPORAL_BEFORE_THE_RESPONSE.get(name, (0, hashlib.sha256().hexdigest())), name
