"""The resource-creation sites of the host library, named so that the names survive edits elsewhere in a file.

A site is a source line of a host file that calls one of the six creators.  The failure-injecting build (tests/failinject/)
reports a site as "file.cpp:LINE hipName"; a line number moves with every edit above it, so tests/golden/failure_sites.json and
the comparisons use a key instead: "file.cpp | <the line's code, stripped> | k", k counting identical lines within the file.
Used by tests/failure_tour.py and the drivers of tests/failure_walks.py (on the GPU machine) and tests/test_failure_sites.py
(without a GPU).

Below the sites, what the failure-injection tests on the GPU share: run_child, the one place that starts a child process
(tests/failure_tour.py or tests/failure_walks.py), and check_feature_walk, what every feature walk's log must show."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "myraytracer_amd", "csrc")
FI_LIB = os.path.join(ROOT, "myraytracer_amd", "lib", "libmyraytracer_amd_failinject.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "failure_sites.json")
WALKS = os.path.join(ROOT, "tests", "failure_walks.py")
# the host files (scripts/source_hash.py's compiled .cpp files and the headers they share)
HOST_FILES = ("api.cpp", "frames.cpp", "world.cpp", "noise.cpp", "present.cpp", "denoise.cpp", "multi_gpu.cpp", "hierarchy.cpp",
              "scenes.cpp", "image_io.cpp", "mrt_ctx.h", "mrt_internal.h", "hierarchy.h", "bounds.h", "width_policy.h")
CREATORS = ("hipMalloc", "hipHostMalloc", "hipStreamCreate", "hipStreamCreateWithFlags", "hipEventCreate", "hipEventCreateWithFlags")
WAITS = ("hipStreamWaitEvent",)       # the stream waits (tests/order_walks.py, tests/test_stream_wait_sites.py)


def _call(names):
    return re.compile(r"\b(" + "|".join(sorted(names, key=len, reverse=True)) + r")\s*\(")


def _code(line):
    """The line without its // comment (no creator call here shares a line with a string that holds "//")."""
    return line.split("//", 1)[0].strip()


def source_sites(csrc=CSRC, files=HOST_FILES, calls=CREATORS):
    """{(file, line number): key} for every call of one of `calls` (the creators) in the host files; a line with two calls is
    one site."""
    sites = {}
    call = _call(calls)
    for name in files:
        seen = {}
        with open(os.path.join(csrc, name)) as f:
            for no, line in enumerate(f, 1):
                code = _code(line)
                if code.startswith("#define") or not call.search(code):
                    continue
                k = seen[code] = seen.get(code, 0) + 1
                sites[(name, no)] = f"{name} | {code} | {k}"
    return sites


def key_of(shim_site, sites=None):
    """The key of a site as the shim reports it ("file.cpp:LINE hipName"); None if the sources have no creator call there."""
    sites = source_sites() if sites is None else sites
    where = shim_site.split(" ", 1)[0]
    name, _, no = where.rpartition(":")
    return sites.get((name, int(no)))


def run_child(script, args, log, limit_s):
    """ONE fresh child process of a tour or a walk, with a time limit of its own; returns the records of its log.  The child
    alone loads the substituted library; twenty hardware queues, as the package asks for where the host sets none.  A child that
    dies or runs into its limit fails the test with the last logged case; nothing is run a second time."""
    import pytest
    assert os.path.exists(FI_LIB), "build the failure-injecting library first (make)"
    what = " ".join([os.path.basename(script), *args])
    env = dict(os.environ, MRT_LIB_OVERRIDE=FI_LIB, GPU_MAX_HW_QUEUES="20")

    def records():
        return [json.loads(line) for line in open(log)] if os.path.exists(log) else []

    def last_case():
        r = [x for x in records() if "n" in x]
        return {k: v for k, v in r[-1].items() if k not in ("sites", "keys")} if r else "none"
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, script, *args, "--log", str(log)], env=env, timeout=limit_s, capture_output=True, text=True, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.fail(f"{what} did not end within {limit_s} s; last logged case: {last_case()} (find the cause there; not run again)")
    print(f"{what}: the child took {time.time() - t0:.1f} s of its {limit_s} s")
    recs = records()
    if p.returncode not in (0, 1):
        stopped = [r for r in recs if "stopped" in r]
        pytest.fail(f"the process of {what} ended with {p.returncode}; last logged case: {last_case()}; "
                    f"{stopped[-1]['stopped'] if stopped else p.stderr[-2000:]}")
    return recs


def check_feature_walk(recs):
    """What the log of every walk of tests/failure_walks.py must show: a clean case that counts T, no finding, N = 1 .. T once,
    in order and each reaching its refusal, at creation sites the recorded tour knows.  Returns T and the cases' keys in order."""
    clean, cases = recs[0], recs[1:]
    assert clean.get("mode") == "clean" and not clean["reached"]
    T = clean["calls"]
    findings = [f"N={r['n']}: {f}" for r in recs for f in r.get("findings", [])]
    assert not findings, f"{len(findings)} findings, the first of them:\n" + "\n".join(findings[:20])
    assert [r["n"] for r in cases] == list(range(1, T + 1)) and all(r["reached"] for r in cases)
    src = source_sites()
    keys = [key_of(r["site"], src) for r in cases]
    assert all(keys), keys
    golden = json.load(open(GOLDEN))["sites"]
    assert set(keys) <= set(golden)             # no creation site the recorded tour does not know
    return T, keys


def feature_walk(name, tmp_path, limit_s, *flags):
    """(T, keys) of the walk `name` of tests/failure_walks.py, run in a child and checked"""
    return check_feature_walk(run_child(WALKS, ["--walk", name, *flags], tmp_path / "walk.jsonl", limit_s))
