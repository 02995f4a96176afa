"""The host library's resource-failure paths, by failure injection (include/myraytracer_amd.h, "after MRT_ERR_HIP": C1-C4).

Each test starts ONE fresh child process (tests/failure_tour.py) against lib/libmyraytracer_amd_failinject.so -- the same
sources with every creation / release of device memory, pinned memory, streams and events routed through a shim
(tests/failinject/) -- with a time limit of its own.  The child walks N = 1 .. T once, refusing the N-th creation of a scripted
tour that reaches every creation site, and logs one JSON line per case.  Nothing is provoked on the GPU: the shim says "no"
without calling the runtime, and after a refusal mrt_debug_check_context (host only) must pass before anything is launched
again.  If the child dies or runs into its limit the test fails with the last logged case; nothing is run a second time.

The limits are three times what the walks took on an MI355X (profiles/failure_paths.txt)."""
import json
import os

import pytest

from failure_sites import GOLDEN, ROOT, run_child

pytestmark = pytest.mark.gpu

TOUR = os.path.join(ROOT, "tests", "failure_tour.py")
# 3 x what the child took on an MI355X, start-up included: about 4 s for the clean tour alone, + 24 s / + 49 s for the walks
LIMIT_S = {"clean": 15, "destroy": 85, "continue": 160}


def walk(mode, tmp_path):
    return run_child(TOUR, ["--mode", mode], tmp_path / f"{mode}.jsonl", LIMIT_S[mode])


def check(mode, recs):
    clean = recs[0]
    assert clean["mode"] == "clean" and clean["calls"] > 0
    findings = [f"N={r.get('n', r.get('summary'))}: {f}" for r in recs for f in r.get("findings", [])]
    assert not findings, f"{len(findings)} findings, the first of them:\n" + "\n".join(findings[:20])
    golden = json.load(open(GOLDEN))["sites"]
    assert clean["keys"] == sorted(golden), ("the clean tour's sites are not tests/golden/failure_sites.json: "
                                             f"new {sorted(set(clean['keys']) - set(golden))}, gone {sorted(set(golden) - set(clean['keys']))}")
    if mode == "clean":
        return
    T = clean["calls"]
    cases = [r for r in recs if r.get("mode") == mode]
    summary = [r for r in recs if r.get("summary") == mode]
    assert [r["n"] for r in cases] == list(range(1, T + 1)), "the walk covers N = 1 .. T once, in order"
    assert summary and summary[0]["first"] == 1 and summary[0]["last"] == T
    reached = [r for r in cases if r["reached"]]
    for r in cases:
        if not r["reached"]:
            print(f"N={r['n']}: not reached (the tour made {r['calls']} creator calls this time)")
    # judged by sites: a refusal at every site of the clean run (the summary's findings, asserted above), most N reached
    assert {r["site"] for r in reached} == set(clean["sites"])
    assert len(reached) >= T - 64, f"only {len(reached)} of {T} cases reached their refusal"
    print(f"{mode}: T = {T}, {len(clean['sites'])} sites, {len(reached)} refusals, clean tour {clean['seconds']} s, walk {summary[0]['seconds']} s")


def test_clean_tour_reaches_the_recorded_sites_and_leaves_nothing(tmp_path):
    """disarmed: every step succeeds, every creation site of tests/golden/failure_sites.json is seen, and after the last
    mrt_destroy nothing is live and no release or copy was withheld (a leak on the SUCCESS path is caught here)"""
    check("clean", walk("clean", tmp_path))


def test_destroy_after_every_refusal_releases_everything(tmp_path):
    """C1 and C2 for N = 1 .. T: the refused call returns MRT_ERR_HIP and names the runtime call; after mrt_destroy of every
    context -- half-built ones of a failed mrt_create included -- the live counts are what they were, exactly"""
    check("destroy", walk("destroy", tmp_path))


def test_every_refused_call_can_be_repeated_and_nothing_differs_afterwards(tmp_path):
    """C1-C4 for N = 1 .. T: sound after the refusal (mrt_debug_check_context), the same call succeeds when repeated, every
    later observable is bit-identical to the clean run's, and nothing is live after the end"""
    check("continue", walk("continue", tmp_path))
