#!/usr/bin/env python3
"""Run by tests/test_gpu_gather_denoise.py in a FRESH process (so that exactly one librccl is in it): mrt_gather_rccl with
mrt_set_gather_noise on, on an RCCL communicator created by this caller with /opt/rocm's librccl.

A one-GPU box allows a world of one (RCCL refuses two ranks on one device): the root's own S goes through the same un-permute
into the gathered frame's allocation, the snapshot is taken, and the reads and the denoise of the gathered frame run.  The
second message of a non-root rank and its receive on the root need two GPUs and are not exercised here.  Prints "ok" and exits 0
on success.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["MRT_HIP_RUNTIME"] = "system"      # a process without torch: /opt/rocm's HIP runtime for the library and for librccl
import myraytracer_amd as M  # noqa: E402


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def main():
    rccl = C.CDLL(os.environ.get("MRT_RCCL_LIB", "/opt/rocm/lib/librccl.so.1"), mode=C.RTLD_GLOBAL)
    comm = C.c_void_p()
    devs = (C.c_int * 1)(0)
    rccl.ncclCommInitAll.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int)]
    rc = rccl.ncclCommInitAll(C.byref(comm), 1, devs)
    assert rc == 0, f"ncclCommInitAll -> {rc}"
    sc, cam = M.scene_cover(1, True)
    with M.State(M.Args(96, 54, 2, 50), seed=1) as st:
        st.set_noise_tracking(True)
        st.set_world(sc)
        st.set_camera(cam)
        st.redraw()
        st.redraw()
        st.gather_rccl(comm.value, 0)               # the setting is off: colour alone
        try:
            st.read_gathered_noise()
            raise SystemExit("a gather with the setting off left a gathered S")
        except M.MrtError as e:
            assert e.status == 7, e
        st.set_gather_noise(True)
        st.gather_rccl(comm.value, 0)
        assert same(st.read_gathered(), st.read_framebuffer())
        assert same(st.read_gathered_noise(), st.read_noise())
        assert same(st.read_gathered_denoised(), st.read_denoised())
        st.redraw()                                 # the snapshot is the gather's
        two = st.read_gathered_denoised()
        assert not same(two, st.read_denoised())
        st.gather_rccl(comm.value, 0)
        assert same(st.read_gathered_denoised(), st.read_denoised())
    # a rank without noise tracking is refused before anything is sent
    with M.State(M.Args(96, 54, 2, 50), seed=1) as st:
        st.set_world(sc)
        st.redraw()
        st.set_gather_noise(True)
        try:
            st.gather_rccl(comm.value, 0)
            raise SystemExit("a rank without noise tracking was accepted")
        except M.MrtError as e:
            assert e.status == 7 and "noise tracking" in str(e), e
    rccl.ncclCommDestroy.argtypes = [C.c_void_p]
    rccl.ncclCommDestroy(comm)
    print("ok")


if __name__ == "__main__":
    main()
