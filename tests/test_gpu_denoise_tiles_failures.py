"""The resource-failure paths of the denoise of an adaptive accumulation, by failure injection (include/myraytracer_amd.h, "after
MRT_ERR_HIP": C1-C4).

ONE fresh child process (tests/failure_walks.py --walk denoise_tiles) against lib/libmyraytracer_amd_failinject.so, with a time limit of
its own: it counts the creator calls T that mrt_set_denoise_adaptive(1), mrt_render_tiles on half the tiles and mrt_read_denoised
make on a prepared context of 37 x 29 with two frames rendered, then refuses the N-th of them for N = 1 .. T, each on a fresh context.  Nothing is provoked
on the GPU -- the shim says "no" without calling the runtime -- and after a refusal mrt_debug_check_context (host only) must pass
before anything is launched again.  If the child dies or runs into its limit the test fails with the last logged case; nothing is
run a second time."""
import pytest

from failure_sites import feature_walk

pytestmark = pytest.mark.gpu

LIMIT_S = 90        # T + 1 contexts of 37 x 29 pixels, three frames each, behind one start-up of a few seconds


def test_every_creation_of_the_subset_frame_and_the_per_tile_denoise_can_be_refused(tmp_path):
    T, keys = feature_walk("denoise_tiles", tmp_path, LIMIT_S)
    # the first subset frame: the tiles' frame counts and the slot's tile list with its pinned staging copy -- 3, frames.cpp's existing
    # lines; the K tables, float and double -- 2, noise.cpp's existing lines (ensure_k_table, now called by the denoise as well);
    # the denoiser's first use: the guides' three buffers, the filter's three, the guide records and the bitmap -- 8, denoise.cpp's
    # existing lines.  Nothing of the feature's own.
    assert T == 13, T
    assert [k.split(" | ")[0] for k in keys] == ["frames.cpp"] * 3 + ["noise.cpp"] * 2 + ["denoise.cpp"] * 8, keys
    assert keys[0] == "frames.cpp | if (!c->d_tile_frames) HIP_TRY(c, hipMalloc((void**)&c->d_tile_frames, (size_t)c->n_tiles * sizeof(uint32_t))); | 1"
    assert keys[3] == "noise.cpp | HIP_TRY(c, hipMalloc((void**)&c->d_k_f32, (size_t)cap * sizeof(float))); | 1"
    assert keys.count("denoise.cpp | if (!d) HIP_TRY(c, hipMalloc((void**)&d, n * 16)); | 1") == 3
    print(f"T = {T}, sites: {sorted(set(keys))}")
