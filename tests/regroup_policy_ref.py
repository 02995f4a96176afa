"""The auto-regroup policy of mrt_set_auto_regroup (include/myraytracer_amd.h, "scene"; myraytracer_amd/csrc/regroup_policy.hip),
restated in numpy and plain Python floats: the quality figure in the order of additions the device uses, and the state machine.

quality(h, n_pool): h is the dict of mrt_debug_read_hierarchy (or of test_refit_host.host_hierarchy).  Level k = 1 .. levels has
its records in h["nodes"][level_base[k]:level_base[k + 1]] -- the top level, k = levels, in h["top"] -- and record j of level k
covers the clusters [j 4^(k-1), (j+1) 4^(k-1)).  Q_k sums float64(-neg_r2_j) over the records with j 4^(k-1) < n_pool whose
neg_r2 is not +inf.  The order: "lane" l of 256 adds the records j = l, l + 256, .. ascending, starting from 0.0; the 256 partials
are added in lane order, starting from 0.0; Q = ((Q_1 + Q_2) + ..).  Every sum below is an explicit loop: np.sum is pairwise.

The state machine (dicts; every function returns a new one):
  new_state()                        what mrt_set_world* uploads: baseline pending, counters 0
  decide(s, levels, Q, ratio)        a check: -> (state, fired)
  baseline(s, levels, Q, mark)       behind a refit: takes q_ref if pending (mark: a regroup the caller asked for sets pending first)

variant= holds three references broken on purpose (tests/test_regroup_policy_host.py shows they are rejected): "never_hit" counts
never-hit records, "non_pool" includes the nodes that begin behind the pool, "stale_ref" keeps the first q_ref forever."""
import numpy as np

LANES = 256
DEFAULT_RATIO, DEFAULT_CHECK_EVERY = 1.5, 8        # mrt_auto_regroup_default
BROKEN = ("never_hit", "non_pool", "stale_ref")
# the walk of tests/test_gpu_auto_regroup.py on the `small` layout: 12 steps at ratio 1.05, mrt_regroup_spheres behind step 6
# (tests/test_regroup_policy_host.py shows on the host that some of its checks fire and some do not)
WALK_STEPS, WALK_AMOUNT, WALK_RATIO, WALK_MANUAL = 12, 0.007, 1.05, 6


def level_records(h, k):
    """the records of level k (1 .. levels) as the refit numbers them"""
    if k == h["levels"]:
        return h["top"]
    end = h["level_base"][k + 1] if k + 1 < h["levels"] else len(h["nodes"])
    return h["nodes"][h["level_base"][k]:end]


def judged(h, n_pool, k, variant=""):
    """the float32 neg_r2 of level k's records that count, in record order"""
    v = np.ascontiguousarray(level_records(h, k)[:, 3], np.float32)
    span = 4 ** (k - 1)
    if variant != "non_pool":
        v = v[:min(len(v), (n_pool + span - 1) // span)]
    return v


def _sequential(values):
    total = 0.0
    for x in values:
        total = total + float(x)
    return total


def quality(h, n_pool, variant=""):
    """-> ([Q_1 .. Q_levels], Q) as Python floats (float64), in the device's order of additions"""
    levels = []
    for k in range(1, h["levels"] + 1):
        v = judged(h, n_pool, k, variant)
        r2 = (-v).astype(np.float64)                       # (the negation and the widening are exact)
        keep = np.ones(len(v), bool) if variant == "never_hit" else ~(np.isinf(v) & (v > 0))
        partials = [_sequential(r2[l::LANES][keep[l::LANES]]) for l in range(LANES)]
        levels.append(_sequential(partials))
    q = levels[0]
    for x in levels[1:]:
        q = q + x
    return levels, q


def walk_steps(xyzr, steps, amount, seed=5):
    """the (n, 4) spheres of each step of a random walk: every sphere but the last (the ground) moves by a normal step of
    `amount` x the scene's size (the walk of scripts/animation_rates.py at another size)"""
    xyzr = np.asarray(xyzr, np.float32).reshape(-1, 4).copy()
    size = float(np.ptp(xyzr[:-1, :3], axis=0).max())
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        xyzr = xyzr.copy()
        xyzr[:-1, :3] += (rng.normal(size=(len(xyzr) - 1, 3)) * amount * size).astype(np.float32)
        out.append(xyzr)
    return out


def new_state():
    return dict(q_ref=0.0, q_last=0.0, q_level=[], pending=True, gate=False, checks=0, regroups=0, frozen=False)


def decide(s, levels, q, ratio, variant=""):
    """a check (every check_every-th update, before that update's refit) -> (the state after it, whether the gate opened)"""
    s = dict(s, q_level=list(levels), q_last=q, checks=s["checks"] + 1)
    if s["pending"]:
        return _take(s, q, variant, gate=False), False
    if q > float(np.float32(ratio)) * s["q_ref"]:
        s.update(gate=True, pending=True, regroups=s["regroups"] + 1)
        return s, True
    s["gate"] = False
    return s, False


def baseline(s, levels, q, mark=False, variant=""):
    """behind a refit (a check's, or mrt_regroup_spheres' with mark; also mrt_set_auto_regroup turning the policy on, with mark)"""
    if not (mark or s["pending"]):
        return dict(s)
    return _take(dict(s, q_level=list(levels), q_last=q), q, variant)


def _take(s, q, variant, **more):
    if not (variant == "stale_ref" and s["frozen"]):
        s["q_ref"] = q
    s.update(pending=False, frozen=True, **more)
    return s
