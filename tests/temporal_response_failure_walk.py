"""The failure-injection walk over the temporal response's resource creations, run in a child process of
tests/test_gpu_temporal_response_failures.py against lib/libmyraytracer_amd_failinject.so (MRT_LIB_OVERRIDE): tests/temporal_failure_walk.py's
walk -- the same prepared context, the same contract C1-C4 of include/myraytracer_amd.h, "after MRT_ERR_HIP", the same log -- with
another act and another observable.

    python tests/temporal_response_failure_walk.py --log FILE [--off]

The act is mrt_set_temporal_response (enabled 1; with --off enabled 0), mrt_set_temporal(1) and the first mrt_temporal_step; the
observable is mrt_read_temporal, the history and, with the response on, the fast history."""
import ctypes as C
import hashlib
import sys

import numpy as np

import temporal_failure_walk as base
from temporal_failure_walk import H, OK, W


class Walk(base.Walk):
    enabled = 1

    def act(self, c):
        r = self.lib.MrtTemporalResponse()
        self.L.mrt_temporal_response_default(C.byref(r))
        r.enabled = self.enabled
        st = self.L.mrt_set_temporal_response(c, C.byref(r))
        return st if st != OK else super().act(c)

    def observe(self, c):
        obs = super().observe(c)
        if not self.enabled:
            return obs
        h2 = np.zeros((H, W, 4), np.float32)
        self.must(c, self.L.mrt_debug_read_temporal_fast(c, h2.ctypes.data, H * W), "mrt_debug_read_temporal_fast")
        return hashlib.sha1(obs.encode() + h2.tobytes()).hexdigest()


if __name__ == "__main__":
    if "--off" in sys.argv:
        sys.argv.remove("--off")
        Walk.enabled = 0
    base.Walk = Walk
    sys.exit(base.main())
