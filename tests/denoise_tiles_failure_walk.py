"""The failure-injection walk over the resource creations of the denoise of an adaptive accumulation, run in a child process of
tests/test_gpu_denoise_tiles_failures.py against lib/libmyraytracer_amd_failinject.so (MRT_LIB_OVERRIDE); the shim plumbing is
tests/failure_tour.py's.  The contract held is C1-C4 of include/myraytracer_amd.h, "after MRT_ERR_HIP".

    python tests/denoise_tiles_failure_walk.py --log FILE

On a prepared context (noise tracking, scene, camera, two frames in flight at most and two frames rendered, so that both frame
slots exist; nothing adaptive, nothing of the denoiser yet) the act is mrt_set_denoise_adaptive(1), mrt_render_tiles on half the
tiles, mrt_read_denoised.  Disarmed, it makes T creator calls and its observable -- the framebuffer, S, the tiles' frame counts and
the denoised image -- is recorded.  Then for N = 1 .. T, each on a fresh prepared context: arm N, act; the refusal comes back as
MRT_ERR_HIP naming the refused runtime call (C1); mrt_debug_check_context, host only, passes before anything else is launched
(C3); disarmed, the refused call succeeds when repeated -- the act goes on from it, a subset frame is not rendered twice -- and
the observable is the clean run's bit for bit (C4); after mrt_destroy the live counts are what they were (C2).  One JSON line per
case; nothing is ever retried.  Exit 0: no finding; 1: findings (in the log); 3: stopped on something that is neither an injected
refusal nor a finding."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from failure_tour import ERR_HIP, OK, H, W, Tour, Unexpected      # noqa: E402

TILES_X, TILES_Y = (W + 7) // 8, (H + 7) // 8


class Walk:
    def __init__(self):
        self.t = Tour()                     # (the shim's functions declared, the scenes made; its steps are not run here)
        self.L, self.lib = self.t.L, self.t.lib
        self.n = len(self.t.small)
        self.half = np.arange(TILES_X * TILES_Y // 2, dtype=np.uint32)

    def must(self, c, st, what):
        if st != OK:
            raise Unexpected(f"{what}: status {st}: {(self.L.mrt_last_error(c) or b'').decode()}")

    def prepare(self):
        L = self.L
        args = self.lib.MrtArgs(W, H, 1, 6, 1.0)
        c = C.c_void_p()
        self.must(None, L.mrt_create(C.byref(args), 11, 0, C.byref(c)), "mrt_create")
        self.must(c, L.mrt_set_noise_tracking(c, 1), "mrt_set_noise_tracking")
        self.must(c, L.mrt_set_camera(c, C.byref(self.t.small_cam._c())), "mrt_set_camera")
        self.must(c, L.mrt_set_world(c, self.t.small.ctypes.data, self.n), "mrt_set_world")
        self.must(c, L.mrt_debug_set_frames_in_flight(c, 2), "mrt_debug_set_frames_in_flight")
        for _ in range(2):
            self.must(c, L.mrt_redraw(c), "mrt_redraw")
        self.must(c, L.mrt_sync(c), "mrt_sync")
        return [c]

    def act(self, ctxs, start=0):
        """(status, the step it ended in): the steps from `start` on"""
        L, c = self.L, ctxs[0]
        img = np.zeros((H, W, 4), np.float32)
        steps = (lambda: L.mrt_set_denoise_adaptive(c, 1),
                 lambda: L.mrt_render_tiles(c, self.half.ctypes.data, self.half.size, 1),
                 lambda: L.mrt_read_denoised(c, img.ctypes.data, img.size))
        for k in range(start, len(steps)):
            st = steps[k]()
            if st != OK:
                return st, k
        return OK, len(steps)

    def observe(self, ctxs):
        c = ctxs[0]
        fb, den, s = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32)
        tiles = np.zeros(TILES_X * TILES_Y, np.uint32)
        self.must(c, self.L.mrt_read_framebuffer(c, fb.ctypes.data, fb.size), "mrt_read_framebuffer")
        self.must(c, self.L.mrt_read_noise(c, s.ctypes.data, s.size), "mrt_read_noise")
        self.must(c, self.L.mrt_read_tile_frames(c, tiles.ctypes.data, tiles.size, None, None), "mrt_read_tile_frames")
        self.must(c, self.L.mrt_read_denoised(c, den.ctypes.data, den.size), "mrt_read_denoised")
        if sorted(set(tiles.tolist())) != [2, 3]:
            raise Unexpected(f"the tiles' frame counts are {sorted(set(tiles.tolist()))}, not 2 and 3: a subset frame too many or too few")
        return hashlib.sha1(fb.tobytes() + s.tobytes() + tiles.tobytes() + den.tobytes()).hexdigest()

    def sound(self, ctxs):
        why = C.create_string_buffer(512)
        for i, c in enumerate(ctxs):
            if self.L.mrt_debug_check_context(c, why, len(why)) != 0:
                return f"ctxs[{i}]: {why.value.decode()}"
        return None

    def case(self, n_arm, clean_obs):
        L, t = self.L, self.t
        rec = {"n": n_arm, "findings": []}
        bad = rec["findings"].append
        base = t.live()
        L.mrt_fi_reset()
        ctxs = self.prepare()
        R = ctxs[0]
        L.mrt_fi_arm(n_arm)                 # (counts from here: the act's creator calls alone; 0 only counts)
        st, step = self.act(ctxs)
        site = t.fired()
        rec["calls"] = int(L.mrt_fi_calls())
        if site is not None:
            rec["site"] = site
            msg = (L.mrt_last_error(R) or b"").decode()
            name = site.split(" ")[1]
            if st != ERR_HIP:
                bad(f"C1: the refusal at {site} came back as status {st}, not MRT_ERR_HIP ({msg})")
            if name + "(" not in msg:
                bad(f"C1: mrt_last_error does not name the refused call {name} at {site}: {msg!r}")
            finding = self.sound(ctxs)
            if finding:
                bad(f"C3: after the refusal at {site}: {finding}")
            L.mrt_fi_disarm()
            if not finding and st != OK:
                st, step = self.act(ctxs, step)         # C4: the refused call can be repeated, and the act goes on from it
                if st != OK:
                    bad(f"C4: repeated after the refusal at {site}: status {st} ({(L.mrt_last_error(R) or b'').decode()})")
                else:
                    finding = self.sound(ctxs)
                    if finding:
                        bad(f"C3: after the repeated call: {finding}")
                        st = ERR_HIP
        elif st != OK:
            raise Unexpected(f"status {st} that the shim did not inject: {(L.mrt_last_error(R) or b'').decode()}")
        L.mrt_fi_disarm()
        rec["reached"] = site is not None
        obs = None
        if st == OK and not rec["findings"]:
            obs = self.observe(ctxs)
            if clean_obs is not None and obs != clean_obs:
                bad(f"C4: the framebuffer, S, the tiles' frame counts or the denoised image differ from the run in which nothing was refused (after {site})")
        for c in ctxs:
            L.mrt_destroy(c)
        live = t.live()
        if live != base:
            bad(f"C2: live {{device, pinned, streams, events}} {live} after mrt_destroy, {base} before mrt_create")
        for v in t.violations():
            bad("shim: " + v)
        return rec, obs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", required=True)
    a = ap.parse_args()
    log = open(a.log, "a")

    def emit(rec):
        log.write(json.dumps(rec) + "\n")
        log.flush()
        os.fsync(log.fileno())

    findings = 0
    try:
        w = Walk()
        clean, clean_obs = w.case(0, None)
        clean["mode"] = "clean"
        emit(clean)
        findings += len(clean["findings"])
        if not clean["findings"]:
            for n in range(1, clean["calls"] + 1):
                rec, _ = w.case(n, clean_obs)
                emit(rec)
                findings += len(rec["findings"])
    except Unexpected as e:
        emit({"stopped": str(e)})
        print("stopped:", e, file=sys.stderr)
        return 3
    except Exception as e:          # noqa: BLE001  (whatever it is, the walk ends here and says why)
        import traceback
        emit({"stopped": "exception: " + repr(e), "traceback": traceback.format_exc()})
        traceback.print_exc()
        return 3
    return 1 if findings else 0


if __name__ == "__main__":
    sys.exit(main())
