"""The gathered frame's denoise at the boundary, without a GPU: the new entry points and the present flag are declared in the
headers, listed in _lib.EXPORTS and exported by the product library and by the failure-injecting one alike."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mrt_set_gather_noise", "mrt_read_gathered_noise", "mrt_read_gathered_denoised")
NEW_DEBUG = ("mrt_debug_read_gathered_guides",)


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_new_entry_points_are_declared_listed_and_exported(mrt):
    from myraytracer_amd import _lib
    pub, dbg = _header("myraytracer_amd.h"), _header("myraytracer_amd_debug.h")
    for name in NEW:
        assert re.search(r"^int " + name + r"\(mrt_ctx\*", pub, re.M), name
    for name in NEW_DEBUG:
        assert re.search(r"^int " + name + r"\(mrt_ctx\*", dbg, re.M), name
    assert re.search(r"^#define MRT_ABI_VERSION 4$", pub, re.M)             # additions only
    for lib in ("libmyraytracer_amd.so", "libmyraytracer_amd_failinject.so"):
        names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "myraytracer_amd", "lib", lib)], capture_output=True,
                               text=True, check=True).stdout
        for name in NEW + NEW_DEBUG:
            assert name in _lib.EXPORTS and f" {name}\n" in names, (lib, name)


def test_the_present_flag_is_one_number_everywhere(mrt):
    from myraytracer_amd import _lib
    m = re.search(r"^#define MRT_PRESENT_GATHERED_DENOISED (\d+)u$", _header("myraytracer_amd.h"), re.M)
    assert m and int(m.group(1)) == _lib.PRESENT_GATHERED_DENOISED == 32
    others = (_lib.PRESENT_FLIP_Y, _lib.PRESENT_GATHERED, _lib.PRESENT_DENOISED, _lib.PRESENT_TEMPORAL)
    assert all(_lib.PRESENT_GATHERED_DENOISED & o == 0 for o in others)
    import inspect
    assert "gathered_denoised" in inspect.signature(mrt.State.present).parameters


def test_set_gather_noise_without_a_context(mrt):
    from myraytracer_amd import _lib
    L = _lib.load()
    assert L.mrt_set_gather_noise(None, 1) == 1             # MRT_ERR_INVALID_ARG
    assert L.mrt_read_gathered_noise(None, None, 0) == 1 and L.mrt_read_gathered_denoised(None, None, 0) == 1
    assert L.mrt_debug_read_gathered_guides(None, None, None, None, None, None, 0) == 1
