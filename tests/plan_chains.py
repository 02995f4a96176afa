"""Chains that put the device's budget plan (mrt_noise_query_budget, mrt_read_budget_plan, mrt_render_planned) next to scene
edits, resets and frames in flight, checked against a host model.  They sit on adaptive_chains' runner through its hooks -- a
Shadow, a Model, a compare and an extra_check of their own -- the way adaptive_chains sits on motion_chains; adaptive_chains'
chains and case numbers are untouched.  On top of its ops:

  ("plan", threshold, floor, budget, max_frames)   mrt_noise_query_budget
  ("read_plan", seq)                               mrt_read_budget_plan(seq): always a named report
  ("planned", seq)                                 mrt_render_planned(seq)
  ("refuse", kind, seq)                            REFUSALS: a plan the header refuses, MRT_ERR_STATE each

The model is adaptive_chains.Model plus, per report: whether it carries a plan, n_q (the model's n_t at the query) and
budget_plan_ref.plan on the model's own summed-S map; ("planned", seq) is budget_plan_ref.target against the model's n_t now,
rendered as the levels L_j through the model's render_tiles, as adaptive_chains.Model renders mrt_render_budget's.  It follows
the header and reads nothing back.  At max_framebuffer_weight 0 K is +inf for every n: no difference of two K is > 0, so a plan
holds mandatory frames only, and both variance sums are +inf, or NaN where a tile's s is 0.

Compared where a call stands: the status; k (mrt_read_budget_plan) or k' (mrt_render_planned), tile_frames, tiles, frames,
used_seq, the plan's tile_frames, and both variances as 64-bit patterns (a NaN equals a NaN: its sign and payload are the
platform's).  A check compares what adaptive_chains' compares, and every plan the ring still holds.

Eleven chains are written out (CHAINS); chain(case) draws further ones from a seed: `python tests/plan_chains.py CASE` prints one."""
import os
import sys

import numpy as np

if __name__ == "__main__":                      # (python tests/plan_chains.py CASE: the package lies one directory up)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import adaptive_chains as AC
import budget_plan_ref as ref
import budget_ref
import material_chains as XC
import motion_chains as MC

OK, INVALID_ARG, NO_SCENE, STATE = MC.OK, MC.INVALID_ARG, MC.NO_SCENE, MC.STATE
NOISE_RING = AC.NOISE_RING
SMALL_IMAGE, WIDE_IMAGE = AC.SMALL_IMAGE, AC.WIDE_IMAGE
# a plan that is not held (older than the ring, discarded by mrt_reset or by tracking switched off and on), read and rendered;
# a report of the ring that holds a max-rel map, and one that holds a summed-S map without a plan
REFUSALS = ("plan-not-held", "planned-not-held", "plan-on-max-rel", "plan-on-sums")
VOCABULARY = ("plan", "read_plan", "planned")
UNION_VOCABULARY = AC.UNION_VOCABULARY + VOCABULARY


class Shadow(AC.Shadow):
    def calls(self, op):
        name, a = op[0], op[1:]
        if name == "plan":
            return [("noise_query", (a[0], a[1], "sum_s", a[2], a[3]))]
        if name == "read_plan":
            return [("budget_plan", a)]
        if name == "planned":
            return [("render_planned", a)]
        if name == "refuse" and a[0] in REFUSALS:
            return [("render_planned" if a[0] == "planned-not-held" else "budget_plan", a[1:])]
        return super().calls(op)


# ------------------------------------------------------------------ the model

class Model(AC.Model):
    """adaptive_chains.Model with the plans.  What the seeded defects of tests/test_plan_chains_host.py override: _plan_counts,
    _left, _held, _reported_after."""

    def __init__(self, O, max_w, w=MC.W, h=MC.H):
        super().__init__(O, max_w, w, h)
        self.kinds, self.plans = {}, {}         # seq -> the report's map kind; seq -> {map, n_q, budget, max_frames}
        self.targets = []                       # (k, k') of every mrt_render_planned: statistics for the host tests' conditions

    # ---- what the seeded defects change
    def _plan_counts(self, seq):
        """the n the allocation of report `seq` was made from"""
        return self.plans[seq]["n_q"]

    def _left(self, n_q, k):
        return ref.target(n_q, k, self.acc.n)

    def _held(self, seq):
        return self._oldest() <= seq <= self.noise_seq

    def _reported_after(self, seq, res, left):
        return res["var_after"]

    # ----
    def noise_query(self, threshold=0.02, floor=0.01, tile_map="max_rel", budget=None, max_frames=8):
        if budget is None:
            super().noise_query(threshold, floor, tile_map)
            self.kinds[self.noise_seq] = tile_map
            return
        if not self.tracking:
            raise MC.Refused(STATE, "noise_query_budget")
        if not 1 <= max_frames <= 32:
            raise MC.Refused(INVALID_ARG, "noise_query_budget")
        super().noise_query(threshold, floor, "sum_s")
        seq = self.noise_seq
        self.kinds[seq] = "sum_s"
        self.plans[seq] = dict(map=self.reports[seq]["map"].copy(), n_q=self.acc.n.copy(), budget=int(budget), max_frames=int(max_frames))

    def _plan(self, where, seq):
        if not self.tracking:
            raise MC.Refused(STATE, where)
        assert seq != 0, "the chains always name a report: 0 depends on what has finished"
        if not self._held(seq) or self.kinds[seq] != "sum_s" or seq not in self.plans:
            raise MC.Refused(STATE, where)
        p = self.plans[seq]
        k, res = ref.plan(p["map"].ravel(), self._plan_counts(seq), self.max_w, p["budget"], p["max_frames"])
        return p, k, res

    def _shaped(self, k):
        return np.asarray(k, np.uint32).reshape(self.acc.tr, self.acc.tx)

    def budget_plan(self, report_seq=0):
        _, k, res = self._plan("read_budget_plan", report_seq)
        return dict(res, used_seq=report_seq, k=self._shaped(k))

    def render_planned(self, report_seq=0):
        if not self.tracking:
            raise MC.Refused(STATE, "render_planned")
        if self.spheres is None:
            raise MC.Refused(NO_SCENE, "render_planned")
        if self.rng_mode == 1 and self.spp > AC.COUNTER_BLOCK:
            raise MC.Refused(INVALID_ARG, "render_planned")
        p, k, res = self._plan("render_planned", report_seq)
        left = self._left(p["n_q"], k)
        self.last_levels = []
        for tiles, run in budget_ref.levels(left):
            self.render_tiles(tiles, run)
            self.last_levels.append((len(tiles), run))
        self.targets.append((k.copy(), left.copy()))
        return dict(used_seq=report_seq, tile_frames=int(left.sum()), tiles=int((left > 0).sum()), frames=int(left.max(initial=0)),
                    var_before=res["var_before"], var_after=self._reported_after(report_seq, res, left), k=self._shaped(left),
                    planned_tile_frames=res["tile_frames"])


# ------------------------------------------------------------------ comparing

def _bits(x):
    return np.float64(x).view(np.uint64)


def compare_plan(name, got, want):
    for f in ("used_seq", "tile_frames", "tiles", "frames") + (("planned_tile_frames",) if name == "render_planned" else ()):
        if got[f] != want[f]:
            return f"plan result {f}: {got[f]} against {want[f]}"
    for f in ("var_before", "var_after"):
        if _bits(got[f]) != _bits(want[f]) and not (np.isnan(got[f]) and np.isnan(want[f])):
            return f"plan result {f}: {got[f]!r} against {want[f]!r}"
    if not np.array_equal(got["k"], want["k"]):
        return f"k_t {np.asarray(got['k']).ravel().tolist()} against {np.asarray(want['k']).ravel().tolist()}"
    return None


def _compare_for(run):
    """motion_chains.Run's compare hook, with the runner at hand: the launches of a rendered plan are told to the runner as
    mrt_render_budget's are (its prediction of every launch's camera table goes on behind them)"""
    def compare(name, got, want):
        if name in ("budget_plan", "render_planned"):
            bad = compare_plan(name, got, want)
            if bad is None and name == "render_planned":
                levels = run.model.last_levels
                for i, (listed, run_length) in enumerate(levels):
                    run.rendered(run_length, listed, last=i == len(levels) - 1)
            return bad
        return AC.compare(name, got, want)
    return compare


def extra_check(run):
    """adaptive_chains' check, then every plan the ring still holds"""
    AC.extra_check(run)
    m = run.model
    for seq in sorted(m.plans):
        if m.tracking and m._held(seq):
            status, got, want = run._both("budget_plan", (seq,))
            if status != OK:
                run._fail(f"budget_plan({seq}): both refuse with status {status}")
            bad = compare_plan("budget_plan", got, want)
            if bad:
                run._fail(f"budget_plan({seq}): {bad}")
            run.stats["plans checked"] = run.stats.get("plans checked", 0) + 1


# ------------------------------------------------------------------ the chains

_p, _start, _S, _U, _Q, _CAM, _MAT, CHECK = AC._p, AC._start, AC._S, AC._U, AC._Q, AC._CAM, AC._MAT, AC.CHECK
_P = lambda budget, max_frames=4, thr=0.3, fl=0.02: ("plan", thr, fl, budget, max_frames)
_RP = lambda seq: ("read_plan", seq)
_PL = lambda seq: ("planned", seq)
_NO = lambda kind, seq: ("refuse", kind, seq)

CHAINS = {
    # frames of all three kinds queued between a plan and its rendering: the target rule leaves a partial k'; the same plan rendered
    # again renders nothing
    "queued-subset": (_p("small"), _start("small", 4) + [
        _P(14, 4), _S((0, 1), 2), _S((4,)), _PL(1), CHECK, _PL(1), _RP(1), CHECK,
        _P(20, 3), _S((2, 3)), _U("jitter", 11), _S((2,)), _PL(2), _PL(2), CHECK]),
    "queued-adaptive": (_p("small", size=WIDE_IMAGE), _start("small", 4, 3) + [
        _S((0, 7)), _Q("max_rel", 0.05), _P(40, 4), ("adaptive", 1, 1), _PL(2), CHECK,
        _Q("max_rel", 0.2), _P(30, 3), ("adaptive", 2, 3), _RP(4), _PL(4), _PL(4), CHECK]),
    "queued-whole": (_p("small", 0.75), _start("small", None, 2) + [
        _P(12, 4), ("render", 1), _PL(1), CHECK, _P(18, 4), ("render", 2), _S((5,)), _PL(2), _RP(2), CHECK]),
    # plans rendered one query behind (render_until's pattern), and two plans rendered newest first
    "lag-1": (_p("small"), _start("small", 4) + [
        _P(8, 2), _P(8, 2), _PL(1), _P(10, 3), _PL(2), _P(10, 3), _PL(3), CHECK, _P(12, 4), _PL(4), _PL(5), CHECK]),
    "newest-first": (_p("small", size=WIDE_IMAGE), _start("small", 8, 3) + [
        _P(30, 3), _S((1, 2, 9)), _P(24, 2), _PL(2), _PL(1), CHECK, _RP(1), _RP(2), _PL(1), CHECK]),
    # a ninth query takes the first plan's ring entry; a max-rel report and a summed-S report without a plan next to planned ones
    "ring": (_p("small"), _start("small", 8, 3) + [
        _P(1, 1), _P(2, 2), _P(3, 3), _P(4, 4), _P(5, 2), _P(6, 3), _P(7, 4), CHECK, _P(8, 2), _RP(1), _P(9, 3), _NO("plan-not-held", 1), CHECK,
        _NO("planned-not-held", 1), _RP(2), _RP(9), _PL(5), _Q("max_rel"), _Q("sum_s"), _NO("plan-on-max-rel", 10), _NO("plan-on-sums", 11), CHECK,
        _RP(9), _PL(9), CHECK]),
    # a plan across every call that changes the scene or the view: kept, it is a list of counts
    "edits": (_p("small"), _start("small", 4) + [
        _P(16, 4), _U("jitter", 21), _RP(1), _MAT("recolour", 22), _RP(1), ("regroup",), _RP(1), CHECK, _CAM(0.2), _PL(1), CHECK,
        _P(18, 3), ("set_world", "large-quad"), _RP(2), _PL(2), CHECK, _P(12, 2), _U("scatter", 23), _MAT("types", 24), _PL(3), _RP(1), CHECK]),
    # ... and across the calls that discard the reports: mrt_reset, tracking switched off and on
    "reset": (_p("small", 0.75), _start("small", 4) + [
        _P(12, 4), _S((0, 1)), ("reset",), _NO("plan-not-held", 1), _NO("planned-not-held", 1), CHECK, ("render", 2), _P(10, 2), _RP(2),
        _NO("plan-not-held", 1), _PL(2), CHECK, ("reset",), ("tracking", False), ("tracking", True), _NO("plan-not-held", 2), ("render", 3),
        _NO("planned-not-held", 2), _P(9, 3), _PL(3), CHECK]),
    # a plan on a uniform accumulation, on one that diverges between the query and the rendering, on a diverged one; mandatory
    # frames (a plan made before the second frame)
    "divergence": (_p("small", size=WIDE_IMAGE), [("set_world", "small"), ("tracking", True), ("render", 1), _P(30, 3), _PL(1), CHECK,
        ("reset",), ("render", 3), _P(25, 3), _RP(2), _S((0, 6, 12)), _PL(2), CHECK, _P(40, 4), _PL(3), ("render", 1), _P(18, 2), _PL(4), CHECK]),
    # budget 0: a plan of zeros; budget 2^40: every candidate, whole frames while the accumulation is uniform
    "budgets": (_p("small"), _start("small", None, 3) + [
        _P(0, 4), _RP(1), _PL(1), CHECK, _P(1 << 40, 2), _RP(2), _PL(2), CHECK, _S((3,), 2), _P(1 << 40, 3), _P(0, 1), _PL(4), _PL(3), CHECK]),
    # 4 and 8 frames in flight, no wait between the frames, the query and the rendering
    "in-flight": (_p("small", size=WIDE_IMAGE), _start("small", 4, 2) + [
        ("render", 3), _S((0, 1, 2, 3)), ("render", 2), _P(36, 4), _S((4, 5)), _PL(1), ("render", 2), _P(30, 3), _PL(2), CHECK,
        ("set_frames_in_flight", 8), ("render", 4), _S((6, 7, 8), 2), _P(50, 4), ("render", 3), _PL(3), _P(20, 2), _S((9,)), _PL(4), _RP(3), CHECK]),
}
NAMES = tuple(CHAINS)


# ------------------------------------------------------------------ the generator
#
# chain(case) draws (params, ops) from np.random.default_rng(case) in a fixed order, under adaptive_chains' rules of legality: at
# most 40 ops, a check at least every 8 ops and at the end, behind every regroup before the grouping changes again and behind every
# third update; a stale camera set anew; a plan is always named, by a report of the ring since the last reset that carries one --
# unless the op is a ("refuse", ...).  PLAN[case % len(PLAN)] fixes the layout, the weight and the image.
PLAN = (("small", 1.0, SMALL_IMAGE), ("small", 0.75, WIDE_IMAGE), ("small", 0.0, SMALL_IMAGE), ("large-quad", 1.0, WIDE_IMAGE),
        ("large-lin", 0.75, SMALL_IMAGE), ("small", 0.0, WIDE_IMAGE))
SUITE_CASES = tuple(range(12))
MAX_OPS, CHECK_EVERY = 40, 8


def chain(case: int):
    """-> (params, ops) of a random chain"""
    rng = np.random.default_rng(1000 + case)
    layout, max_w, size = PLAN[case % len(PLAN)]
    p = dict(layout=layout, flavour="plan", max_w=max_w, size=size)
    n_tiles = -(-size[0] // 8) * -(-size[1] // 8)
    sh, ops = Shadow(), []
    g = dict(seq=0, first=1, planned=[], other={}, since=0, updates=0, owed=False, frames=0)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    seed = lambda: int(rng.integers(0, 2 ** 31))

    def emit(*op):
        if op != CHECK and ops and (g["since"] >= CHECK_EVERY - 1 or (op[0] in ("regroup", "set_world") and g["owed"])):
            emit(*CHECK)
        if op == CHECK and ops[-1] == CHECK:
            return
        ops.append(op)
        sh.calls(op)
        name = op[0]
        g["since"] = 0 if name == "check" else g["since"] + 1
        if name == "check":
            g.update(updates=0, owed=False)
        elif name == "regroup":
            g["owed"] = True
        elif name in ("render", "subset"):
            g["frames"] += op[-1]
        elif name == "reset":
            g.update(first=g["seq"] + 1, frames=0)
        elif name == "plan":
            g["seq"] += 1
            g["planned"].append(g["seq"])
        elif name == "query":
            g["seq"] += 1
            g["other"][g["seq"]] = op[3]
        elif name in ("read_plan", "planned"):
            assert op[1] in held(g["planned"])
        if name == "update":
            g["updates"] += 1
            if sh.camera_stale():
                emit("set_camera", float(rng.uniform(-0.5, 0.5)), float(rng.uniform(11.0, 15.0)), float(rng.uniform(2.0, 3.0)))
            if g["updates"] >= 3:
                emit(*CHECK)

    def held(seqs):
        oldest = max(g["first"], g["seq"] - NOISE_RING + 1, 1)
        return [s for s in seqs if s >= oldest]

    def tiles():
        k = int(rng.integers(1, min(4, n_tiles - 1) + 1))
        return tuple(sorted(int(t) for t in rng.choice(n_tiles, k, replace=False)))

    def plan():
        emit("plan", pick((0.2, 0.3, 0.5)), 0.02, pick((0, 3, n_tiles, 2 * n_tiles, 3 * n_tiles + 1, 1 << 40)), pick((1, 2, 3, 4, 32)))
        return g["seq"]

    def a_plan():
        return pick(held(g["planned"])) if held(g["planned"]) else plan()

    def queued():                               # frames of some kind between a query and its rendering
        kind = int(rng.integers(0, 3))
        if kind == 0:
            emit("subset", tiles(), int(rng.integers(1, 3)))
        elif kind == 1:
            emit("render", int(rng.integers(1, 3)))
        else:
            emit("update", pick(("jitter", "partial", "scatter")), seed())
            emit("subset", tiles(), 1)

    def seg_target():
        s = plan()
        queued()
        emit("planned", s)
        if rng.random() < 0.5:
            emit("planned", s)

    def seg_lag():
        prev = plan()
        for _ in range(int(rng.integers(2, 4))):
            s = plan()
            emit("planned", prev)
            prev = s
        emit("planned", prev)

    def seg_edits():
        s = a_plan()
        for kind in rng.permutation(4)[:int(rng.integers(2, 4))]:
            if kind == 0:
                emit("update", pick(("jitter", "partial")), seed())
            elif kind == 1:
                emit("materials", pick(XC.MATERIAL_KINDS), seed(), False)
            elif kind == 2:
                emit("regroup")
            else:
                emit("set_camera", float(rng.uniform(-0.4, 0.4)), float(rng.uniform(11.0, 15.0)), float(rng.uniform(2.0, 3.0)))
            emit("read_plan", s)
        emit("planned", s)

    def seg_reset():
        s = a_plan()
        emit("reset")
        emit("refuse", pick(("plan-not-held", "planned-not-held")), s)
        emit("render", int(rng.integers(1, 4)))
        seg_target()

    def seg_ring():
        first = plan()
        for i in range(NOISE_RING):
            emit("query", 0.3, 0.02, pick(("max_rel", "sum_s"))) if i % 3 == 1 else plan()
        emit("refuse", "plan-not-held", first)
        other = held(list(g["other"]))
        if other:
            s = pick(other)
            emit("refuse", "plan-on-max-rel" if g["other"][s] == "max_rel" else "plan-on-sums", s)
        emit("read_plan", pick(held(g["planned"])))
        emit("planned", pick(held(g["planned"])))

    def seg_newest_first():
        a = plan()
        emit("subset", tiles(), 1)
        b = plan()
        emit("planned", b)
        emit("planned", a)

    segs = dict(target=seg_target, lag=seg_lag, edits=seg_edits, reset=seg_reset, ring=seg_ring, newest=seg_newest_first)
    order = list(segs)
    in_flight = (4, 8, None)[case % 3]
    for op in _start(layout, in_flight, int(rng.integers(1, 4))):
        emit(*op)
    if case % 2:
        emit("subset", tiles(), 1)              # (diverged from the start)
    import copy
    for i in range(8):
        name = order[(case + i * (1 + case // len(order) % 2)) % len(order)] if i < 3 else pick(order)
        saved = (len(ops), copy.deepcopy(g), copy.deepcopy(sh), copy.deepcopy(rng.bit_generator.state))
        segs[name]()
        if len(ops) > MAX_OPS - 1:              # (it does not fit: taken back whole, the draws with it)
            del ops[saved[0]:]
            g.clear()
            g.update(saved[1])
            sh.__dict__.clear()
            sh.__dict__.update(saved[2].__dict__)
            rng.bit_generator.state = saved[3]
    emit(*CHECK)
    assert len(ops) <= MAX_OPS and {op[0] for op in ops} <= set(UNION_VOCABULARY)
    return p, ops


def params_and_ops(name):
    """a written chain by its name, a random one by its case number"""
    return chain(name) if isinstance(name, int) else CHAINS[name]


def new_model(O, name, cls=None):
    return MC.new_model(O, params_and_ops(name)[0], cls or Model)


def new_run(name, impl, model, O, stats=None, after=None, device_checks=True):
    label = f"random plan chain {name} (python tests/plan_chains.py {name})" if isinstance(name, int) else f"plan chain {name}"
    r = MC.Run(label, params_and_ops(name)[0], impl, model, O, stats, after, device_checks, shadow=Shadow(), extra_check=extra_check)
    r.compare = _compare_for(r)
    return r


def run(name, impl, model, O, stats=None, after=None, device_checks=True):
    """chain `name` on impl and model in lock step (motion_chains.Run); raises ChainMismatch at the first difference"""
    r = new_run(name, impl, model, O, stats, after, device_checks)
    for op in params_and_ops(name)[1]:
        r.step(op)
    return r


if __name__ == "__main__":                      # the case's params and ops, one per line, for replay and bug reports (no device)
    for case in (int(a) for a in sys.argv[1:]):
        params, case_ops = chain(case)
        print(f"case {case}: {params}")
        for i, op in enumerate(case_ops):
            print(f"{i:3d} {op!r}")
