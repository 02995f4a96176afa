"""Host tests of the plan chains (tests/plan_chains.py), as tests/test_adaptive_chains_host.py is for the adaptive chains: every
written and every random chain is legal on the model; the situations the chains exist for are present, read from their ops; run
model against model they meet the conditions without which the GPU test would pass vacuously (plans rendered with a partial k',
plans already met); a case number reproduces its chain; and the runner reports every seeded defect of a stand-in."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_chains as AC
import budget_plan_ref as ref
import motion_chains as MC
import plan_chains as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY = tuple(PC.NAMES) + tuple(PC.SUITE_CASES)
KEPT_ACROSS = ("update", "materials", "regroup", "set_camera", "set_world")
FRAMES = ("subset", "adaptive", "render")


def _status(op):
    if op[0] != "refuse":
        return MC.OK
    return MC.STATE if op[1] in PC.REFUSALS else AC.REFUSAL_STATUS[op[1]]


def test_shape_and_vocabulary():
    assert len(PC.NAMES) >= 10 and len(PC.SUITE_CASES) == 12
    names = set()
    for n in EVERY:
        p, ops = PC.params_and_ops(n)
        assert len(ops) <= 40 and ops[0] == ("set_world", p["layout"]) and ops[-1] == ("check",), (n, len(ops))
        assert p["size"] in (PC.SMALL_IMAGE, PC.WIDE_IMAGE) and {op[0] for op in ops} <= set(PC.UNION_VOCABULARY), n
        names |= {op[0] for op in ops}
        edits = 0
        for op in ops[1:]:                      # a check after every third scene edit, as the adaptive chains have it
            edits = 0 if op[0] == "check" else edits + (op[0] in KEPT_ACROSS)
            assert edits <= 3, (n, op)
    assert set(PC.VOCABULARY) <= names
    suite = [PC.chain(c)[0] for c in PC.SUITE_CASES]
    assert {p["size"] for p in suite} == {PC.SMALL_IMAGE, PC.WIDE_IMAGE} and {p["max_w"] for p in suite} == {1.0, 0.75, 0.0}
    for c in PC.SUITE_CASES:                    # the generator's own rule: a check at least every 8 ops
        checks = [-1] + [i for i, op in enumerate(PC.chain(c)[1]) if op == ("check",)]
        assert max(np.diff(checks)) <= 8, (c, checks)
    assert {op[1] for n in PC.NAMES for op in PC.CHAINS[n][1] if op[0] == "refuse"} == set(PC.REFUSALS)
    for name in AC.NAMES:                       # adaptive_chains' own chains are what they were: its vocabulary, no plan
        assert not {op[0] for op in AC.CHAINS[name][1]} & set(PC.VOCABULARY)


def test_every_chain_is_legal(oracle):
    """the model accepts every call but the refusals drawn, and refuses those with the status the header states"""
    for n in EVERY:
        m, sh = PC.new_model(oracle, n), PC.Shadow()
        for op in PC.params_and_ops(n)[1]:
            for call, args in sh.calls(op):
                got, _ = MC._call(m, call, args)
                assert got == _status(op), (n, op, call, got)
            if op[0] == "refuse" and op[1] in ("plan-not-held", "planned-not-held"):     # one reason at a time
                assert m.tracking and op[2] in m.plans and not m._held(op[2]), (n, op)
            if op[0] == "refuse" and op[1] in ("plan-on-max-rel", "plan-on-sums"):
                assert m._held(op[2]) and op[2] not in m.plans and m.kinds[op[2]] == {"plan-on-max-rel": "max_rel", "plan-on-sums": "sum_s"}[op[1]]


def _seqs(ops):
    """{report seq: the index of the query that made it}, and the kind of each"""
    at, kinds, seq = {}, {}, 0
    for i, op in enumerate(ops):
        if op[0] in ("plan", "query"):
            seq += 1
            at[seq], kinds[seq] = i, "plan" if op[0] == "plan" else op[3]
    return at, kinds


def _situations(chains):
    found = {k: [] for k in ("queued-subset", "queued-adaptive", "queued-whole", "twice", "lag-1", "newest-first", "ninth", "max-rel-neighbour",
                             "uniform", "diverged", "diverges-between", "budget-0", "budget-2^40", "in-flight-4", "in-flight-8", "reset",
                             "tracking") + tuple("across-" + k for k in KEPT_ACROSS)}
    for n, (p, ops) in chains.items():
        at, kinds = _seqs(ops)
        last_reset = lambda i: max([j for j in range(i) if ops[j][0] == "reset"], default=0)
        subset_since_reset = lambda i: any(o[0] == "subset" for o in ops[last_reset(i):i])
        selected_since_reset = lambda i: any(o[0] in ("subset", "adaptive", "budget", "planned") for o in ops[last_reset(i):i])
        in_flight = 0
        lag = 0
        for i, op in enumerate(ops):
            if op[0] == "set_frames_in_flight":
                in_flight = op[1]
            if op[0] == "plan":
                if op[3] == 0:
                    found["budget-0"].append(n)
                if op[3] == 1 << 40:
                    found["budget-2^40"].append(n)
                found["diverged" if subset_since_reset(i) else "uniform" if not selected_since_reset(i) else "diverged"].append(n)
            if op[0] in ("planned", "read_plan") and op[1] in at:
                between = ops[at[op[1]] + 1:i]
                for k in KEPT_ACROSS:
                    if any(o[0] == k for o in between):
                        found["across-" + k].append(n)
            if op[0] == "planned":
                between = ops[at[op[1]] + 1:i]
                for kind, key in (("subset", "queued-subset"), ("adaptive", "queued-adaptive"), ("render", "queued-whole")):
                    if any(o[0] == kind for o in between):
                        found[key].append(n)
                if not selected_since_reset(at[op[1]]) and any(o[0] == "subset" for o in between):
                    found["diverges-between"].append(n)
                if i and ops[i - 1] == op:
                    found["twice"].append(n)
                if i and ops[i - 1][0] == "planned" and ops[i - 1][1] > op[1]:
                    found["newest-first"].append(n)
                lag = lag + 1 if i and ops[i - 1][0] == "plan" and at.get(op[1] + 1) == i - 1 else 0
                if lag >= 2:
                    found["lag-1"].append(n)
                if in_flight in (4, 8) and not any(o == ("check",) for o in ops[at[op[1]]:i]) and any(o[0] in FRAMES for o in between):
                    found[f"in-flight-{in_flight}"].append(n)
            if op[0] == "refuse" and op[1] in ("plan-not-held", "planned-not-held"):
                between = ops[at[op[2]] + 1:i]
                if sum(o[0] in ("plan", "query") for o in between) >= PC.NOISE_RING and op[2] == 1 and kinds[1] == "plan":
                    found["ninth"].append(n)
                if any(o[0] == "reset" for o in between):
                    found["reset"].append(n)
                if ("tracking", False) in between and ("tracking", True) in between:
                    found["tracking"].append(n)
            if op[0] == "refuse" and op[1] == "plan-on-max-rel":
                held = [s for s in kinds if s > len(kinds) - PC.NOISE_RING]
                if kinds[op[2]] == "max_rel" and any(kinds[s] == "plan" for s in held):
                    found["max-rel-neighbour"].append(n)
    return found


def test_every_situation_is_present():
    found = _situations({n: PC.CHAINS[n] for n in PC.NAMES})
    assert all(found.values()), {k: v for k, v in found.items() if not v}
    suite = _situations({c: PC.chain(c) for c in PC.SUITE_CASES})
    for k in ("queued-subset", "queued-whole", "twice", "lag-1", "newest-first", "ninth", "reset", "uniform", "diverged", "budget-0",
              "budget-2^40", "across-update", "across-materials", "across-regroup", "across-set_camera"):
        assert suite[k], k


@pytest.fixture(scope="module")
def reference_runs(oracle):
    return {n: PC.run(n, PC.new_model(oracle, n), PC.new_model(oracle, n), oracle) for n in EVERY}


def test_the_reference_meets_the_conditions(reference_runs):
    """the target rule shows: plans rendered with 0 < k' != k in each of the three chains that queue frames in between, plans
    already met (k' = 0 behind a k that was not), plans with unequal counts; the checks compare plans; budget 2^40 on a uniform
    accumulation renders whole frames"""
    partial = {n: sum(bool((k != left).any() and left.any()) for k, left in r.model.targets) for n, r in reference_runs.items()}
    met = {n: sum(bool(k.any() and not left.any()) for k, left in r.model.targets) for n, r in reference_runs.items()}
    for n in ("queued-subset", "queued-adaptive", "queued-whole", "in-flight", "newest-first"):
        assert partial[n] >= 1, (n, partial)
    assert met["queued-subset"] >= 2 and met["queued-adaptive"] >= 1
    assert sum(partial[c] > 0 for c in PC.SUITE_CASES) >= 4 and sum(met[c] > 0 for c in PC.SUITE_CASES) >= 4
    unequal = sum(len(set(k.tolist())) > 1 for r in reference_runs.values() for k, _ in r.model.targets)
    assert unequal >= 20
    assert sum(r.stats.get("plans checked", 0) for r in reference_runs.values()) >= 100
    whole = [k for k, _ in reference_runs["budgets"].model.targets if k.any() and len(set(k.tolist())) == 1]
    assert whole and whole[0][0] == 2
    assert not reference_runs["divergence"].model.targets[0][0].min() == 0          # mandatory frames: every tile gets one


def test_a_case_number_reproduces_its_chain():
    for c in PC.SUITE_CASES:
        assert PC.chain(c) == PC.chain(c)
    out = subprocess.run([sys.executable, os.path.join("tests", "plan_chains.py"), "3", "8"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    want = []
    for c in (3, 8):
        p, ops = PC.chain(c)
        want += [f"case {c}: {p}"] + [f"{i:3d} {op!r}" for i, op in enumerate(ops)]
    assert out.splitlines() == want
    assert len({repr(PC.chain(c)[1]) for c in PC.SUITE_CASES}) == len(PC.SUITE_CASES)


# ------------------------------------------------------------------ seeded defects

class TargetIgnoresFramesSinceTheQuery(PC.Model):
    """k' = k: the frames queued since the query do not count towards the plan"""
    def _left(self, n_q, k):
        return np.asarray(k, np.uint32).copy()


class AllocatesFromTheCountsNow(PC.Model):
    """the allocation is made from n_now in place of n_q"""
    def _plan_counts(self, seq):
        return self.acc.n.copy()


class PlanSurvivesAReset(PC.Model):
    """mrt_reset (and tracking switched off and on) leaves the plans readable"""
    def _held(self, seq):
        return max(self.noise_seq - PC.NOISE_RING + 1, 1) <= seq <= self.noise_seq


class RingOfNine(PC.Model):
    """the ring holds nine plans"""
    def _held(self, seq):
        return max(self.noise_first, self.noise_seq - PC.NOISE_RING, 1) <= seq <= self.noise_seq


class VarAfterOfWhatIsLeft(PC.Model):
    """mrt_render_planned reports var_after for k' instead of the plan's"""
    def _reported_after(self, seq, res, left):
        p = self.plans[seq]
        return ref.blocked_sums(p["map"].ravel(), p["n_q"], left, self.max_w)[1]


DEFECTS = [TargetIgnoresFramesSinceTheQuery, AllocatesFromTheCountsNow, PlanSurvivesAReset, RingOfNine, VarAfterOfWhatIsLeft]
# the written chains that report each defect (the defective stand-in as the implementation); the test holds the list to what it finds
_QUEUED = ["queued-subset", "queued-adaptive", "queued-whole", "lag-1", "newest-first", "ring", "divergence", "in-flight"]
CAUGHT_BY = {
    "TargetIgnoresFramesSinceTheQuery": {"written": _QUEUED, "random": [0, 1, 3, 4, 6, 7, 9, 10, 11]},
    "AllocatesFromTheCountsNow": {"written": ["queued-subset", "queued-adaptive", "queued-whole", "lag-1", "newest-first", "ring", "edits", "reset",
                                              "divergence", "budgets", "in-flight"], "random": [0, 1, 3, 4, 6, 7, 9, 10, 11]},
    "PlanSurvivesAReset": {"written": ["reset"], "random": [1, 2, 3, 5, 7, 9, 11]},
    "RingOfNine": {"written": ["ring"], "random": [2, 3, 4, 6, 8, 10]},
    "VarAfterOfWhatIsLeft": {"written": _QUEUED, "random": [0, 1, 3, 4, 6, 7, 9, 10]},
}


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda c: c.__name__)
def test_the_runner_catches_a_defective_stand_in(oracle, defect):
    caught = {"written": [], "random": []}
    for n in EVERY:
        try:
            PC.run(n, PC.new_model(oracle, n, defect), PC.new_model(oracle, n), oracle)
        except MC.ChainMismatch:
            caught["random" if isinstance(n, int) else "written"].append(n)
    print(f"{defect.__name__}: caught by {caught}")
    assert caught["written"] and caught["random"], (defect.__name__, caught)
    assert caught == CAUGHT_BY[defect.__name__], (defect.__name__, caught)
