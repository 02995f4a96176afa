"""Temporal reprojection's resource-failure paths, by failure injection (include/myraytracer_amd.h, "after MRT_ERR_HIP": C1-C4).

ONE fresh child process (tests/failure_walks.py --walk temporal) against lib/libmyraytracer_amd_failinject.so, with a time limit of its
own: it counts the creator calls T that mrt_set_temporal(1) plus the first mrt_temporal_step make on a prepared context, then
refuses the N-th of them for N = 1 .. T, each on a fresh context.  Nothing is provoked on the GPU -- the shim says "no" without
calling the runtime -- and after a refusal mrt_debug_check_context (host only) must pass before anything is launched again.  If
the child dies or runs into its limit the test fails with the last logged case; nothing is run a second time."""
import pytest

from failure_sites import feature_walk

pytestmark = pytest.mark.gpu

LIMIT_S = 60        # a dozen contexts of 37 x 29 pixels, one frame each, behind one start-up of a few seconds


def test_every_creation_of_the_first_step_can_be_refused(tmp_path):
    T, keys = feature_walk("temporal", tmp_path, LIMIT_S)
    # the guides' four buffers and the bitmap, the filter's three and the history's four: all from the denoiser's existing lines
    assert T == 12, T
    assert all(k and k.startswith("denoise.cpp | ") for k in keys), keys
    assert keys.count("denoise.cpp | if (!d) HIP_TRY(c, hipMalloc((void**)&d, n * 16)); | 1") == 7
    print(f"T = {T}, sites: {sorted(set(keys))}")
