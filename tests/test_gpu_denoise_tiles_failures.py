"""The resource-failure paths of the denoise of an adaptive accumulation, by failure injection (include/myraytracer_amd.h, "after
MRT_ERR_HIP": C1-C4).

ONE fresh child process (tests/denoise_tiles_failure_walk.py) against lib/libmyraytracer_amd_failinject.so, with a time limit of
its own: it counts the creator calls T that mrt_set_denoise_adaptive(1), mrt_render_tiles on half the tiles and mrt_read_denoised
make on a prepared context of 37 x 29 with two frames rendered, then refuses the N-th of them for N = 1 .. T, each on a fresh context.  Nothing is provoked
on the GPU -- the shim says "no" without calling the runtime -- and after a refusal mrt_debug_check_context (host only) must pass
before anything is launched again.  If the child dies or runs into its limit the test fails with the last logged case; nothing is
run a second time."""
import json
import os
import subprocess
import sys

import pytest

from failure_sites import ROOT, key_of

pytestmark = pytest.mark.gpu

WALK = os.path.join(ROOT, "tests", "denoise_tiles_failure_walk.py")
FI_LIB = os.path.join(ROOT, "myraytracer_amd", "lib", "libmyraytracer_amd_failinject.so")
LIMIT_S = 90        # T + 1 contexts of 37 x 29 pixels, three frames each, behind one start-up of a few seconds


def test_every_creation_of_the_subset_frame_and_the_per_tile_denoise_can_be_refused(tmp_path):
    assert os.path.exists(FI_LIB), "build the failure-injecting library first (make)"
    log = tmp_path / "walk.jsonl"
    env = dict(os.environ, MRT_LIB_OVERRIDE=FI_LIB, GPU_MAX_HW_QUEUES="20")

    def records():
        return [json.loads(line) for line in open(log)] if log.exists() else []
    try:
        p = subprocess.run([sys.executable, WALK, "--log", str(log)], env=env, timeout=LIMIT_S, capture_output=True, text=True, cwd=ROOT)
    except subprocess.TimeoutExpired:
        pytest.fail(f"the walk did not end within {LIMIT_S} s; last logged: {records()[-1:]} (find the cause there; not run again)")
    recs = records()
    if p.returncode not in (0, 1):
        stopped = [r for r in recs if "stopped" in r]
        pytest.fail(f"the walk's process ended with {p.returncode}; {stopped[-1]['stopped'] if stopped else p.stderr[-2000:]}")
    clean, cases = recs[0], recs[1:]
    assert clean.get("mode") == "clean" and not clean["reached"]
    T = clean["calls"]
    # the first subset frame: the tiles' frame counts and the slot's tile list with its pinned staging copy -- 3, frames.cpp's existing
    # lines; the K tables, float and double -- 2, noise.cpp's existing lines (ensure_k_table, now called by the denoise as well);
    # the denoiser's first use: the guides' three buffers, the filter's three, the guide records and the bitmap -- 8, denoise.cpp's
    # existing lines.  Nothing of the feature's own.
    assert T == 13, T
    findings = [f"N={r['n']}: {f}" for r in recs for f in r.get("findings", [])]
    assert not findings, f"{len(findings)} findings, the first of them:\n" + "\n".join(findings[:20])
    assert [r["n"] for r in cases] == list(range(1, T + 1)) and all(r["reached"] for r in cases)
    keys = [key_of(r["site"]) for r in cases]
    assert all(k for k in keys), keys
    assert [k.split(" | ")[0] for k in keys] == ["frames.cpp"] * 3 + ["noise.cpp"] * 2 + ["denoise.cpp"] * 8, keys
    assert keys[0] == "frames.cpp | if (!c->d_tile_frames) HIP_TRY(c, hipMalloc((void**)&c->d_tile_frames, (size_t)c->n_tiles * sizeof(uint32_t))); | 1"
    assert keys[3] == "noise.cpp | HIP_TRY(c, hipMalloc((void**)&c->d_k_f32, (size_t)cap * sizeof(float))); | 1"
    assert keys.count("denoise.cpp | if (!d) HIP_TRY(c, hipMalloc((void**)&d, n * 16)); | 1") == 3
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "failure_sites.json")))["sites"]
    assert set(keys) <= set(golden)             # no creation site the recorded tour does not know
    print(f"T = {T}, sites: {sorted(set(keys))}")
