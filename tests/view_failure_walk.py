"""The failure-injection walk over the creations a diagnostic view reaches, as a scenario of tests/failure_walks.py's engine defined
outside it.  Run in a child process of tests/test_gpu_view_failures.py against lib/libmyraytracer_amd_failinject.so
(MRT_LIB_OVERRIDE); the contract held is C1-C4 of include/myraytracer_amd.h, "after MRT_ERR_HIP".

    python tests/view_failure_walk.py --log FILE
"""
import argparse
import ctypes as C
import hashlib
import sys

import numpy as np

import failure_walks
from failure_walks import H, W, Scenario, Shim, logged_main, walk


class View(Scenario):
    """On a prepared context (noise tracking, scene, camera, two frames; nothing of the denoiser yet) the act is mrt_set_view
    (NOISE_REL) and mrt_read_view -- the view as the first user of ensure_denoise_buffers -- then mrt_set_view (SPHERE) and
    mrt_read_view, which builds the guides in the buffers the first made.  T: the guides' three buffers, the filter's three, the
    guide records and the bitmap; nothing of the view's own.  The observable is both views, the framebuffer and S."""
    what_differs = "a view, the framebuffer or S differs"

    def prepare(self):
        c = self.create(1.0)
        self.must(c, self.L.mrt_set_noise_tracking(c, 1), "mrt_set_noise_tracking")
        self.set_scene(c)
        self.must(c, self.L.mrt_render(c, 2), "mrt_render")
        return [c]

    def _set(self, c, kind):
        v = self.lib.MrtView()
        self.L.mrt_view_default(C.byref(v))
        v.kind, v.ramp, v.lo, v.hi = kind, self.lib.VIEW_RAMP_GREY, 0.0, 1.0
        return self.L.mrt_set_view(c, C.byref(v))

    def steps(self, ctxs):
        L, c = self.L, ctxs[0]
        img = np.zeros((H, W, 4), np.float32)
        return [lambda: self._set(c, self.lib.VIEW_NOISE_REL), lambda: L.mrt_read_view(c, img.ctypes.data, img.size),
                lambda: self._set(c, self.lib.VIEW_SPHERE), lambda: L.mrt_read_view(c, img.ctypes.data, img.size)]

    def observe(self, ctxs):
        c = ctxs[0]
        rel, sph, fb = (np.zeros((H, W, 4), np.float32) for _ in range(3))
        s = np.zeros((H, W), np.float32)
        self.must(c, self._set(c, self.lib.VIEW_NOISE_REL), "mrt_set_view")
        self.must(c, self.L.mrt_read_view(c, rel.ctypes.data, rel.size), "mrt_read_view")
        self.must(c, self._set(c, self.lib.VIEW_SPHERE), "mrt_set_view")
        self.must(c, self.L.mrt_read_view(c, sph.ctypes.data, sph.size), "mrt_read_view")
        self.must(c, self.L.mrt_read_framebuffer(c, fb.ctypes.data, fb.size), "mrt_read_framebuffer")
        self.must(c, self.L.mrt_read_noise(c, s.ctypes.data, s.size), "mrt_read_noise")
        if not np.isfinite(rel).all() or len(np.unique(sph.reshape(-1, 4), axis=0)) < 3:
            raise failure_walks.Unexpected("the views of the walk's scene are not what a view of it shows")
        return hashlib.sha1(rel.tobytes() + sph.tobytes() + fb.tobytes() + s.tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", required=True)
    a = ap.parse_args()

    def body(emit):
        from myraytracer_amd import _lib, api
        L = _lib.load()
        walk(L, Shim(L), View(L, _lib, api), emit)
    return logged_main(a.log, body)


if __name__ == "__main__":
    sys.exit(main())
