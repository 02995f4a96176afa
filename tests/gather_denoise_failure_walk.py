"""The failure-injection walk over the resource creations of a gather that carries S and the gathered frame's denoise, run in a
child process of tests/test_gpu_gather_denoise_failures.py against lib/libmyraytracer_amd_failinject.so (MRT_LIB_OVERRIDE); the
shim plumbing is tests/failure_tour.py's.  The contract held is C1-C4 of include/myraytracer_amd.h, "after MRT_ERR_HIP".

    python tests/gather_denoise_failure_walk.py --log FILE

On two prepared shards of one image on device 0 (noise tracking, scene, camera, one frame each; nothing gathered, nothing of the
denoiser yet) the act is mrt_set_gather_noise(root, 1), mrt_gather, mrt_read_gathered_denoised on the root.  Disarmed, it makes T
creator calls and its observable -- the gathered colour, the gathered S and the denoised image -- is recorded.  Then for N = 1 ..
T, each on fresh prepared contexts: arm N, act; the refusal comes back as MRT_ERR_HIP naming the refused runtime call (C1);
mrt_debug_check_context, host only, passes on both contexts before anything else is launched (C3); disarmed, the same act
succeeds and its observable is the clean run's bit for bit (C4); after mrt_destroy the live counts are what they were (C2).
One JSON line per case; nothing is ever retried.  Exit 0: no finding; 1: findings (in the log); 3: stopped on something that is
neither an injected refusal nor a finding."""
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

WORLD, ROOT_RANK = 2, 1


class Walk:
    def __init__(self):
        self.t = Tour()                     # (the shim's functions declared, the scenes made; its steps are not run here)
        self.L, self.lib = self.t.L, self.t.lib
        self.n = len(self.t.small)

    def must(self, c, st, what):
        if st != OK:
            raise Unexpected(f"{what}: status {st}: {(self.L.mrt_last_error(c) or b'').decode()}")

    def prepare(self):
        L = self.L
        ctxs = []
        for r in range(WORLD):
            args = self.lib.MrtArgs(W, H, 1, 6, 0.0)
            c = C.c_void_p()
            self.must(None, L.mrt_create(C.byref(args), 11, 0, C.byref(c)), "mrt_create")
            ctxs.append(c)
            self.must(c, L.mrt_set_shard(c, r, WORLD), "mrt_set_shard")
            self.must(c, L.mrt_set_noise_tracking(c, 1), "mrt_set_noise_tracking")
            self.must(c, L.mrt_set_camera(c, C.byref(self.t.small_cam._c())), "mrt_set_camera")
            self.must(c, L.mrt_set_world(c, self.t.small.ctypes.data, self.n), "mrt_set_world")
            self.must(c, L.mrt_redraw(c), "mrt_redraw")
        return ctxs

    def act(self, ctxs):
        L, R = self.L, ctxs[ROOT_RANK]
        st = L.mrt_set_gather_noise(R, 1)
        if st != OK:
            return st
        arr = (C.c_void_p * WORLD)(*[c.value for c in ctxs])
        st = L.mrt_gather(arr, WORLD, ROOT_RANK)
        if st != OK:
            return st
        img = np.zeros((H, W, 4), np.float32)
        return L.mrt_read_gathered_denoised(R, img.ctypes.data, img.size)

    def observe(self, ctxs):
        R = ctxs[ROOT_RANK]
        fb, den, s = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32)
        self.must(R, self.L.mrt_read_gathered(R, fb.ctypes.data, fb.size), "mrt_read_gathered")
        self.must(R, self.L.mrt_read_gathered_noise(R, s.ctypes.data, s.size), "mrt_read_gathered_noise")
        self.must(R, self.L.mrt_read_gathered_denoised(R, den.ctypes.data, den.size), "mrt_read_gathered_denoised")
        return hashlib.sha1(fb.tobytes() + s.tobytes() + den.tobytes()).hexdigest()

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
        R = ctxs[ROOT_RANK]
        L.mrt_fi_arm(n_arm)                 # (counts from here: the act's creator calls alone; 0 only counts)
        st = self.act(ctxs)
        site = t.fired()
        rec["calls"] = int(L.mrt_fi_calls())
        if site is not None:
            rec["site"] = site
            msg = (L.mrt_last_error(R) or b"").decode()
            name = site.split(" ")[1]
            if st != ERR_HIP:
                bad(f"C1: the refusal at {site} came back as status {st}, not MRT_ERR_HIP ({msg})")
            if name + "(" not in msg:
                bad(f"C1: mrt_last_error of the root does not name the refused call {name} at {site}: {msg!r}")
            finding = self.sound(ctxs)
            if finding:
                bad(f"C3: after the refusal at {site}: {finding}")
            L.mrt_fi_disarm()
            if not finding and st != OK:
                st = self.act(ctxs)         # C4: the call can be repeated
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
                bad(f"C4: the gathered frame, its S or its denoise differs from the run in which nothing was refused (after {site})")
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
