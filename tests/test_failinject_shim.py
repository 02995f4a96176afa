"""The failure-injection shim's own bookkeeping (tests/failinject/mrt_failinject.cpp), without a GPU: the shim is compiled with
the host compiler and linked against tests/failinject/hip_standin.cpp, a stand-in for the HIP functions it forwards to.  What
tests/test_gpu_failure_paths.py concludes from the shim's counts rests on these."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FI = os.path.join(ROOT, "tests", "failinject")
H2D, D2H, D2D = 1, 2, 3             # hipMemcpyKind
SUCCESS, INVALID, OOM = 0, 1, 2     # hipError_t


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    assert os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")), f"no HIP headers under {rocm}"
    so = str(tmp_path_factory.mktemp("shim") / "libshim_standin.so")
    # -Bsymbolic: the stand-in's hipMalloc & co. serve the shim even when the process has loaded the real runtime already
    subprocess.check_call(["g++", "-shared", "-fPIC", "-Wl,-Bsymbolic", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(FI, "mrt_failinject.cpp"), os.path.join(FI, "hip_standin.cpp"), "-o", so])
    L = C.CDLL(so)
    vp, sz, u64, cs, i = C.c_void_p, C.c_size_t, C.c_uint64, C.c_char_p, C.c_int
    for name, res, args in (
            ("mrt_fi_malloc", i, [cs, i, C.POINTER(vp), sz]), ("mrt_fi_host_malloc", i, [cs, i, C.POINTER(vp), sz, C.c_uint]),
            ("mrt_fi_stream_create", i, [cs, i, C.POINTER(vp), i, C.c_uint]), ("mrt_fi_event_create", i, [cs, i, C.POINTER(vp), i, C.c_uint]),
            ("mrt_fi_free", i, [cs, i, vp]), ("mrt_fi_host_free", i, [cs, i, vp]), ("mrt_fi_stream_destroy", i, [cs, i, vp]),
            ("mrt_fi_event_destroy", i, [cs, i, vp]), ("mrt_fi_memcpy_async", i, [cs, i, vp, vp, sz, i, vp]),
            ("mrt_fi_memcpy2d_async", i, [cs, i, vp, sz, vp, sz, sz, sz, i, vp]), ("mrt_fi_memset_async", i, [cs, i, vp, i, sz, vp]),
            ("mrt_fi_memset_d32_async", i, [cs, i, vp, i, sz, vp]),
            ("mrt_fi_arm", None, [u64]), ("mrt_fi_disarm", None, []), ("mrt_fi_calls", u64, []), ("mrt_fi_fired", i, [cs, sz]),
            ("mrt_fi_sites", sz, [cs, sz]), ("mrt_fi_live", None, [C.POINTER(u64)]), ("mrt_fi_violations", sz, [cs, sz]),
            ("mrt_fi_reset", None, []), ("standin_counts", None, [C.POINTER(C.c_ulonglong)]),
            ("mrt_fi_stream_wait_event", i, [cs, i, vp, vp, C.c_uint]), ("mrt_fi_skip_wait", None, [u64]), ("mrt_fi_waits", u64, []),
            ("mrt_fi_skipped", i, [cs, sz]), ("mrt_fi_wait_sites", sz, [cs, sz]), ("standin_waits", C.c_ulonglong, [])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def live(L):
    out = (C.c_uint64 * 4)()
    L.mrt_fi_live(out)
    return list(out)


def reached(L):
    out = (C.c_ulonglong * 4)()
    L.standin_counts(out)
    return list(out)


def violations(L):
    buf = C.create_string_buffer(4096)
    n = L.mrt_fi_violations(buf, len(buf))
    return n, buf.value.decode()


F = b"myraytracer_amd/csrc/api.cpp"


def test_the_armed_creator_call_is_refused_without_reaching_the_runtime(shim):
    L = shim
    L.mrt_fi_reset()
    base, made = live(L), reached(L)[0]
    L.mrt_fi_arm(3)
    p = [C.c_void_p() for _ in range(4)]
    assert L.mrt_fi_malloc(F, 10, C.byref(p[0]), 64) == SUCCESS
    assert L.mrt_fi_event_create(F, 11, C.byref(p[1]), 1, 2) == SUCCESS
    assert L.mrt_fi_fired(None, 0) == 0
    assert L.mrt_fi_host_malloc(F, 12, C.byref(p[2]), 64, 0) == OOM and not p[2].value
    site = C.create_string_buffer(64)
    assert L.mrt_fi_fired(site, len(site)) == 1 and site.value == b"api.cpp:12 hipHostMalloc"
    assert reached(L)[0] == made + 2, "the refused call must not reach the runtime"
    assert L.mrt_fi_stream_create(F, 13, C.byref(p[3]), 1, 1) == SUCCESS, "one shot: the next call goes through"
    assert L.mrt_fi_calls() == 4
    assert [a - b for a, b in zip(live(L), base)] == [1, 0, 1, 1]
    buf = C.create_string_buffer(L.mrt_fi_sites(None, 0))
    L.mrt_fi_sites(buf, len(buf))
    assert buf.value.decode().split("\n")[:-1] == ["api.cpp:10 hipMalloc", "api.cpp:11 hipEventCreateWithFlags", "api.cpp:12 hipHostMalloc",
                                                    "api.cpp:13 hipStreamCreateWithFlags"]
    assert L.mrt_fi_free(F, 20, p[0]) == SUCCESS and L.mrt_fi_event_destroy(F, 21, p[1]) == SUCCESS
    assert L.mrt_fi_stream_destroy(F, 22, p[3]) == SUCCESS
    assert live(L) == base and violations(L)[0] == 0
    # a stream or event refusal is hipErrorInvalidValue
    L.mrt_fi_arm(1)
    assert L.mrt_fi_stream_create(F, 13, C.byref(p[3]), 0, 0) == INVALID
    L.mrt_fi_arm(1)
    assert L.mrt_fi_event_create(F, 13, C.byref(p[3]), 0, 0) == INVALID
    assert live(L) == base


def test_a_release_of_what_is_not_live_is_recorded_and_withheld(shim):
    L = shim
    L.mrt_fi_reset()
    base = live(L)
    p = C.c_void_p()
    assert L.mrt_fi_malloc(F, 10, C.byref(p), 64) == SUCCESS
    released = reached(L)[1]
    assert L.mrt_fi_free(F, 20, p) == SUCCESS and reached(L)[1] == released + 1
    assert L.mrt_fi_free(F, 21, p) == INVALID, "a second free"
    assert reached(L)[1] == released + 1, "must not be forwarded"
    n, text = violations(L)
    assert n == 1 and "api.cpp:21 hipFree" in text and "not live" in text
    assert L.mrt_fi_free(F, 22, None) == SUCCESS and violations(L)[0] == 1, "hipFree(NULL) is no violation"
    assert L.mrt_fi_event_destroy(F, 23, C.c_void_p(0x1234)) == INVALID and L.mrt_fi_stream_destroy(F, 24, C.c_void_p(0x1234)) == INVALID
    assert L.mrt_fi_host_free(F, 25, C.c_void_p(0x1234)) == INVALID
    assert violations(L)[0] == 4 and reached(L)[1] == released + 1
    assert live(L) == base
    L.mrt_fi_reset()
    assert violations(L)[0] == 0


def test_copies_and_memsets_outside_the_live_device_allocations_are_withheld(shim):
    L = shim
    L.mrt_fi_reset()
    p = C.c_void_p()
    assert L.mrt_fi_malloc(F, 10, C.byref(p), 256) == SUCCESS
    host = C.create_string_buffer(512)
    h = C.cast(host, C.c_void_p)
    copies, sets = reached(L)[2:]
    assert L.mrt_fi_memcpy_async(F, 30, p, h, 256, H2D, None) == SUCCESS
    assert L.mrt_fi_memcpy_async(F, 31, h, C.c_void_p(p.value + 128), 128, D2H, None) == SUCCESS
    assert L.mrt_fi_memset_async(F, 32, C.c_void_p(p.value + 255), 0, 1, None) == SUCCESS
    assert L.mrt_fi_memset_d32_async(F, 33, p, 7, 64, None) == SUCCESS
    assert L.mrt_fi_memcpy2d_async(F, 34, p, 64, h, 32, 32, 4, H2D, None) == SUCCESS       # 3 x 64 + 32 = 224 bytes of the 256
    assert reached(L)[2:] == [copies + 3, sets + 2] and violations(L)[0] == 0
    assert L.mrt_fi_memcpy_async(F, 40, p, h, 257, H2D, None) == INVALID, "one byte past the end"
    assert L.mrt_fi_memcpy_async(F, 41, h, C.c_void_p(p.value + 200), 100, D2H, None) == INVALID
    assert L.mrt_fi_memset_async(F, 42, C.c_void_p(p.value - 1), 0, 2, None) == INVALID, "starts before the allocation"
    assert L.mrt_fi_memset_d32_async(F, 43, p, 7, 65, None) == INVALID
    assert L.mrt_fi_memcpy2d_async(F, 44, p, 64, h, 32, 33, 5, H2D, None) == INVALID       # 4 x 64 + 33 = 289
    assert L.mrt_fi_memcpy_async(F, 45, p, h, 16, D2D, None) == INVALID, "a host pointer as a device source"
    assert L.mrt_fi_memcpy_async(F, 46, None, h, 16, H2D, None) == INVALID, "a null destination"
    assert reached(L)[2:] == [copies + 3, sets + 2], "none of them forwarded"
    assert violations(L)[0] == 7
    assert L.mrt_fi_free(F, 50, p) == SUCCESS
    assert L.mrt_fi_memset_async(F, 51, p, 0, 1, None) == INVALID, "a stale pointer"
    assert L.mrt_fi_memcpy_async(F, 52, p, h, 0, H2D, None) == SUCCESS, "nothing to copy touches nothing"
    L.mrt_fi_reset()


def test_the_chosen_stream_wait_is_dropped_without_reaching_the_runtime(shim):
    L = shim
    L.mrt_fi_reset()
    s, e = C.c_void_p(), C.c_void_p()
    assert L.mrt_fi_stream_create(F, 10, C.byref(s), 1, 1) == SUCCESS and L.mrt_fi_event_create(F, 11, C.byref(e), 1, 2) == SUCCESS
    site = C.create_string_buffer(64)
    reached_before = L.standin_waits()
    # counting only: every wait is forwarded, with the runtime's own result
    assert L.mrt_fi_stream_wait_event(F, 20, s, e, 0) == SUCCESS and L.mrt_fi_stream_wait_event(F, 21, s, e, 0) == SUCCESS
    assert L.mrt_fi_stream_wait_event(F, 22, s, None, 0) != SUCCESS, "the runtime's refusal comes back as it is"
    assert L.mrt_fi_waits() == 3 and L.standin_waits() == reached_before + 3 and L.mrt_fi_skipped(site, len(site)) == 0
    # the second from now on is dropped: success, and the runtime has not seen it -- not even one it would have refused
    L.mrt_fi_skip_wait(2)
    assert L.mrt_fi_waits() == 0, "the count restarts"
    assert L.mrt_fi_stream_wait_event(F, 20, s, e, 0) == SUCCESS and L.mrt_fi_skipped(site, len(site)) == 0
    assert L.mrt_fi_stream_wait_event(F, 22, s, None, 0) == SUCCESS
    assert L.mrt_fi_skipped(site, len(site)) == 1 and site.value == b"api.cpp:22 hipStreamWaitEvent"
    assert L.standin_waits() == reached_before + 4, "the dropped wait must not reach the runtime"
    assert L.mrt_fi_stream_wait_event(F, 21, s, e, 0) == SUCCESS and L.standin_waits() == reached_before + 5, "one shot"
    assert L.mrt_fi_waits() == 3
    buf = C.create_string_buffer(L.mrt_fi_wait_sites(None, 0))
    L.mrt_fi_wait_sites(buf, len(buf))
    assert buf.value.decode().split("\n")[:-1] == [f"api.cpp:{n} hipStreamWaitEvent" for n in (20, 21, 22)]
    # the waits and the creators are counted apart, and neither arms the other
    assert L.mrt_fi_calls() == 2 and L.mrt_fi_fired(None, 0) == 0
    creators = C.create_string_buffer(L.mrt_fi_sites(None, 0))
    L.mrt_fi_sites(creators, len(creators))
    assert b"hipStreamWaitEvent" not in creators.value
    L.mrt_fi_skip_wait(1)
    p = C.c_void_p()
    assert L.mrt_fi_malloc(F, 30, C.byref(p), 16) == SUCCESS and L.mrt_fi_skipped(None, 0) == 0
    L.mrt_fi_arm(1)
    assert L.mrt_fi_stream_wait_event(F, 20, s, e, 0) == SUCCESS and L.mrt_fi_skipped(None, 0) == 1 and L.mrt_fi_fired(None, 0) == 0
    L.mrt_fi_disarm()
    # reset forgets the waits too
    L.mrt_fi_skip_wait(1)
    L.mrt_fi_reset()
    assert L.mrt_fi_waits() == 0 and L.mrt_fi_wait_sites(None, 0) == 1 and L.mrt_fi_skipped(None, 0) == 0
    assert L.mrt_fi_stream_wait_event(F, 20, s, e, 0) == SUCCESS and L.mrt_fi_skipped(None, 0) == 0, "reset cancels a pending drop"
    assert L.mrt_fi_free(F, 40, p) == SUCCESS and L.mrt_fi_stream_destroy(F, 41, s) == SUCCESS and L.mrt_fi_event_destroy(F, 42, e) == SUCCESS
    assert violations(L)[0] == 0
