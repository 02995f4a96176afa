"""The temporal response's resource-failure paths, by failure injection (include/myraytracer_amd.h, "after MRT_ERR_HIP": C1-C4).

As tests/test_gpu_temporal_failures.py: ONE fresh child process per walk (tests/failure_walks.py --walk temporal_response) against
lib/libmyraytracer_amd_failinject.so, with a time limit of its own.  With the response on, the first mrt_temporal_step makes the
12 creator calls it always made and two more, the H2 pair, from the same line of denoise.cpp; each of the 14 is refused in turn
on a fresh context and the contract held.  With the response off the count is still 12.  Nothing is provoked on the GPU -- the
shim says "no" without calling the runtime -- and nothing is run a second time."""
import pytest

from failure_sites import feature_walk

pytestmark = pytest.mark.gpu

LIMIT_S = 60        # fifteen contexts of 37 x 29 pixels, one frame each, behind one start-up of a few seconds
DEN_LINE = "denoise.cpp | if (!d) HIP_TRY(c, hipMalloc((void**)&d, n * 16)); | 1"


def walk(tmp_path, *flags):
    T, keys = feature_walk("temporal_response", tmp_path, LIMIT_S, *flags)
    assert all(k and k.startswith("denoise.cpp | ") for k in keys), keys
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
