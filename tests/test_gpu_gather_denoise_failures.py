"""The resource-failure paths of a gather that carries S and of the gathered frame's denoise, by failure injection
(include/myraytracer_amd.h, "after MRT_ERR_HIP": C1-C4).

ONE fresh child process (tests/failure_walks.py --walk gather_denoise) against lib/libmyraytracer_amd_failinject.so, with a time limit of
its own: it counts the creator calls T that mrt_set_gather_noise(1), mrt_gather and mrt_read_gathered_denoised make on two
prepared shards of 37 x 29 on device 0, then refuses the N-th of them for N = 1 .. T, each on fresh contexts.  Nothing is provoked
on the GPU -- the shim says "no" without calling the runtime -- and after a refusal mrt_debug_check_context (host only) must pass
before anything is launched again.  If the child dies or runs into its limit the test fails with the last logged case; nothing is
run a second time."""
import pytest

from failure_sites import feature_walk

pytestmark = pytest.mark.gpu

LIMIT_S = 90        # 13 pairs of contexts of 37 x 29 pixels, one frame each, behind one start-up of a few seconds


def test_every_creation_of_the_gather_and_the_denoise_can_be_refused(tmp_path):
    T, keys = feature_walk("gather_denoise", tmp_path, LIMIT_S)
    # the gather: the full frame's ONE allocation (colour, S behind it), the root's write-after-read event and an event per
    # shard -- 4, all from multi_gpu.cpp's existing lines; the denoise on the root: the guides' four buffers and the bitmap and the
    # filter's three -- 8, all from the denoiser's existing lines
    assert T == 12, T
    assert [k.split(" | ")[0] for k in keys] == ["multi_gpu.cpp"] * 4 + ["denoise.cpp"] * 8, keys
    assert keys[0] == "multi_gpu.cpp | HIP_TRY(R, hipMalloc((void**)&R->d_gather, need ? need : 16)); | 1"
    assert keys.count("denoise.cpp | if (!d) HIP_TRY(c, hipMalloc((void**)&d, n * 16)); | 1") == 3
    print(f"T = {T}, sites: {sorted(set(keys))}")
