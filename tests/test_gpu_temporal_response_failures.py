"""The temporal response's resource-failure paths, by failure injection (include/myraytracer_amd.h, "after MRT_ERR_HIP": C1-C4).

As tests/test_gpu_temporal_failures.py: ONE fresh child process per walk (tests/temporal_response_failure_walk.py) against
lib/libmyraytracer_amd_failinject.so, with a time limit of its own.  With the response on, the first mrt_temporal_step makes the
12 creator calls it always made and two more, the H2 pair, from the same line of denoise.cpp; each of the 14 is refused in turn
on a fresh context and the contract held.  With the response off the count is still 12.  Nothing is provoked on the GPU -- the
shim says "no" without calling the runtime -- and nothing is run a second time."""
import json
import os
import subprocess
import sys

import pytest

from failure_sites import ROOT, key_of

pytestmark = pytest.mark.gpu

WALK = os.path.join(ROOT, "tests", "temporal_response_failure_walk.py")
FI_LIB = os.path.join(ROOT, "myraytracer_amd", "lib", "libmyraytracer_amd_failinject.so")
LIMIT_S = 60        # fifteen contexts of 37 x 29 pixels, one frame each, behind one start-up of a few seconds
DEN_LINE = "denoise.cpp | if (!d) HIP_TRY(c, hipMalloc((void**)&d, n * 16)); | 1"


def walk(tmp_path, *flags):
    assert os.path.exists(FI_LIB), "build the failure-injecting library first (make)"
    log = tmp_path / "walk.jsonl"
    env = dict(os.environ, MRT_LIB_OVERRIDE=FI_LIB, GPU_MAX_HW_QUEUES="20")

    def records():
        return [json.loads(line) for line in open(log)] if log.exists() else []
    try:
        p = subprocess.run([sys.executable, WALK, "--log", str(log), *flags], env=env, timeout=LIMIT_S, capture_output=True, text=True, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.fail(f"the walk did not end within {LIMIT_S} s; last logged: {records()[-1:]} (find the cause there; not run again)")
    recs = records()
    if p.returncode not in (0, 1):
        stopped = [r for r in recs if "stopped" in r]
        pytest.fail(f"the walk's process ended with {p.returncode}; {stopped[-1]['stopped'] if stopped else p.stderr[-2000:]}")
    clean, cases = recs[0], recs[1:]
    assert clean.get("mode") == "clean" and not clean["reached"]
    T = clean["calls"]
    findings = [f"N={r['n']}: {f}" for r in recs for f in r.get("findings", [])]
    assert not findings, f"{len(findings)} findings, the first of them:\n" + "\n".join(findings[:20])
    assert [r["n"] for r in cases] == list(range(1, T + 1)) and all(r["reached"] for r in cases)
    keys = [key_of(r["site"]) for r in cases]
    assert all(k and k.startswith("denoise.cpp | ") for k in keys), keys
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "failure_sites.json")))["sites"]
    assert set(keys) <= set(golden)             # no creation site the recorded tour does not know
    return T, keys


def test_every_creation_of_the_first_step_with_the_response_on_can_be_refused(tmp_path):
    T, keys = walk(tmp_path)
    # the guides' four buffers and the bitmap, the filter's three, the history's four and the fast history's two
    assert T == 14, T
    assert keys.count(DEN_LINE) == 9
    print(f"T = {T}, sites: {sorted(set(keys))}")


def test_with_the_response_off_the_count_is_what_it_was(tmp_path):
    T, keys = walk(tmp_path, "--off")
    assert T == 12, T
    assert keys.count(DEN_LINE) == 7
