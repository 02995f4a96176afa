"""The resource-failure paths a diagnostic view reaches, by failure injection (include/myraytracer_amd.h, "after MRT_ERR_HIP":
C1-C4).

ONE fresh child process (tests/view_failure_walk.py: a scenario of tests/failure_walks.py's engine, defined outside it) against
lib/libmyraytracer_amd_failinject.so, with a time limit of its own: it counts the creator calls T that a NOISE_REL view -- the first
user of the denoiser's buffers -- and then a SPHERE view make on a prepared context of 37 x 29 with two frames rendered, then refuses
the N-th of them for N = 1 .. T, each on a fresh context.  Nothing is provoked on the GPU -- the shim says "no" without calling the
runtime -- and after a refusal mrt_debug_check_context (host only) must pass before anything is launched again.  If the child dies
or runs into its limit the test fails with the last logged case; nothing is run a second time."""
import os

import pytest

from failure_sites import ROOT, check_feature_walk, run_child

pytestmark = pytest.mark.gpu

LIMIT_S = 90        # T + 1 contexts of 37 x 29 pixels, two frames each, behind one start-up of a few seconds


def test_every_creation_a_view_reaches_can_be_refused(tmp_path):
    T, keys = check_feature_walk(run_child(os.path.join(ROOT, "tests", "view_failure_walk.py"), [], tmp_path / "walk.jsonl", LIMIT_S))
    # the denoiser's first use: the guides' three buffers, the filter's three, the guide records and the bitmap -- 8, denoise.cpp's
    # existing lines, all of them made by the first view.  Nothing of the view's own: it holds no resource.
    assert T == 8, T
    assert [k.split(" | ")[0] for k in keys] == ["denoise.cpp"] * 8, keys
    assert keys.count("denoise.cpp | if (!d) HIP_TRY(c, hipMalloc((void**)&d, n * 16)); | 1") == 3
    print(f"T = {T}, sites: {sorted(set(keys))}")
