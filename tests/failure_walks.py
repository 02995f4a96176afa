"""The failure-injection walks over single features' resource creations, and what they share with tests/failure_tour.py: the
shim's functions (Shim), the C1 judgement (c1_findings), the log and exit codes of a child process (logged_main).  Run in a child
process of tests/test_gpu_*_failures.py against lib/libmyraytracer_amd_failinject.so (MRT_LIB_OVERRIDE; tests/failinject/).  The
contract held is C1-C4 of include/myraytracer_amd.h, "after MRT_ERR_HIP".

    python tests/failure_walks.py --walk temporal|temporal_response|gather_denoise|denoise_tiles --log FILE [--off]

A scenario prepares fresh contexts, names the steps of its act and hashes what a caller can read back afterwards.  Disarmed, the
act makes T creator calls and its observable is recorded.  Then for N = 1 .. T, each on fresh prepared contexts: arm N, act; the
refusal comes back as MRT_ERR_HIP naming the refused runtime call (C1); mrt_debug_check_context, host only, passes on every
context before anything else is launched (C3); disarmed, the act succeeds when repeated -- from its first step or from the
refused one, as the scenario says -- and its observable is the clean run's bit for bit (C4); after mrt_destroy the live counts
are what they were (C2).  One JSON line per case is appended to the log before the next case starts; nothing is ever retried.
Exit 0: no finding; 1: findings (in the log); 3: stopped on something that is neither an injected refusal nor a finding."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OK, ERR_HIP = 0, 3
W, H = 37, 29                       # ragged: 5 tile columns (the last 5 pixels wide), 4 bands (the last 5 rows high)
TILES_X, TILES_Y = (W + 7) // 8, (H + 7) // 8
WORLD, ROOT_RANK = 2, 1             # the gather's shards, and the one that gathers


class Unexpected(RuntimeError):
    """Not an injected refusal: the child stops here."""


class Shim:
    """The failure-injecting build's own entry points (tests/failinject/mrt_failinject.h) on a loaded library."""

    def __init__(self, L):
        self.L = L
        u64, sz = C.c_uint64, C.c_size_t
        for name, res, args in (("mrt_fi_arm", None, [u64]), ("mrt_fi_disarm", None, []), ("mrt_fi_calls", u64, []),
                                ("mrt_fi_fired", C.c_int, [C.c_char_p, sz]), ("mrt_fi_sites", sz, [C.c_char_p, sz]),
                                ("mrt_fi_live", None, [C.POINTER(u64)]), ("mrt_fi_violations", sz, [C.c_char_p, sz]),
                                ("mrt_fi_reset", None, [])):
            fn = getattr(L, name)           # AttributeError: not the failure-injecting build
            fn.restype, fn.argtypes = res, args

    def live(self):
        out = (C.c_uint64 * 4)()
        self.L.mrt_fi_live(out)
        return list(out)

    def fired(self):
        buf = C.create_string_buffer(256)
        return buf.value.decode() if self.L.mrt_fi_fired(buf, len(buf)) else None

    def sites(self):
        n = self.L.mrt_fi_sites(None, 0)
        buf = C.create_string_buffer(n)
        self.L.mrt_fi_sites(buf, n)
        return [s for s in buf.value.decode().split("\n") if s]

    def violations(self):
        buf = C.create_string_buffer(1 << 16)
        n = self.L.mrt_fi_violations(buf, len(buf))
        return [s for s in buf.value.decode().split("\n") if s] if n else []


def c1_findings(site, status, message, label=""):
    """C1: the refusal at `site` ("file.cpp:LINE hipName") came back as MRT_ERR_HIP, and mrt_last_error names the runtime call"""
    name = site.split(" ")[1]
    out = []
    if status != ERR_HIP:
        out.append(f"C1: {label}the refusal at {site} came back as status {status}, not MRT_ERR_HIP ({message})")
    if name + "(" not in message:
        out.append(f"C1: {label}mrt_last_error does not name the refused call {name} at {site}: {message!r}")
    return out


def check_contexts(L, ctxs):
    """C3, host only: the first finding of mrt_debug_check_context over the contexts, or None"""
    why = C.create_string_buffer(512)
    for i, c in enumerate(ctxs):
        if L.mrt_debug_check_context(c, why, len(why)) != 0:
            return f"ctxs[{i}]: {why.value.decode()}"
    return None


def run_steps(steps, start=0):
    """(status, the step it ended in): the steps from `start` on, up to the first that does not succeed"""
    for k in range(start, len(steps)):
        st = steps[k]()
        if st != OK:
            return st, k
    return OK, len(steps)


def run_case(L, shim, scenario, n_arm, clean_obs):
    """One case on fresh contexts: the N-th creator call of the act refused (0: none, the calls are only counted).  Returns the
    case's record and its observable (None where the case did not get that far)."""
    rec = {"n": n_arm, "findings": []}
    bad = rec["findings"].append
    base = shim.live()
    L.mrt_fi_reset()
    ctxs = scenario.prepare()
    steps = scenario.steps(ctxs)

    def err():
        return (L.mrt_last_error(ctxs[scenario.root]) or b"").decode()
    L.mrt_fi_arm(n_arm)                     # (counts from here: the act's creator calls alone; 0 only counts)
    st, k = run_steps(steps)
    site = shim.fired()
    rec["calls"] = int(L.mrt_fi_calls())
    if site is not None:
        rec["site"] = site
        rec["findings"] += c1_findings(site, st, err())
        why = check_contexts(L, ctxs)
        if why:
            bad(f"C3: after the refusal at {site}: {why}")
        L.mrt_fi_disarm()
        if not why and st != OK:            # C4: the call can be repeated (a context that failed C3 gets no further launch)
            st, _ = run_steps(steps, k if scenario.repeat == "step" else 0)
            if st != OK:
                bad(f"C4: repeated after the refusal at {site}: status {st} ({err()})")
            else:
                why = check_contexts(L, ctxs)
                if why:
                    bad(f"C3: after the repeated call: {why}")
                    st = ERR_HIP
    elif st != OK:
        raise Unexpected(f"status {st} that the shim did not inject: {err()}")
    L.mrt_fi_disarm()
    rec["reached"] = site is not None
    obs = None
    if st == OK and not rec["findings"]:
        obs = scenario.observe(ctxs)
        if clean_obs is not None and obs != clean_obs:
            bad(f"C4: {scenario.what_differs} from the run in which nothing was refused (after {site})")
    for c in ctxs:
        L.mrt_destroy(c)
    live = shim.live()
    if live != base:
        bad(f"C2: live {{device, pinned, streams, events}} {live} after mrt_destroy, {base} before mrt_create")
    for v in shim.violations():
        bad("shim: " + v)
    return rec, obs


def walk(L, shim, scenario, emit):
    """The clean case, and if it has no finding N = 1 .. T, T being the creator calls the clean case counted."""
    clean, clean_obs = run_case(L, shim, scenario, 0, None)
    clean["mode"] = "clean"
    emit(clean)
    if not clean["findings"]:
        for n in range(1, clean["calls"] + 1):
            emit(run_case(L, shim, scenario, n, clean_obs)[0])


def logged_main(log_path, body):
    """body(emit) in the frame every child process shares.  emit(record) appends one JSON line to the log, on the disk before
    the next case starts.  Returns the exit code: 3 with a "stopped" record where body raised, 1 if any record had findings,
    else 0."""
    log = open(log_path, "a")
    findings = 0

    def emit(rec):
        nonlocal findings
        findings += len(rec.get("findings", ()))
        log.write(json.dumps(rec) + "\n")
        log.flush()
        os.fsync(log.fileno())

    try:
        body(emit)
    except Unexpected as e:
        emit({"stopped": str(e)})
        print("stopped:", e, file=sys.stderr)
        return 3
    except Exception as e:          # noqa: BLE001  (whatever it is, the walk ends here and says why)
        emit({"stopped": "exception: " + repr(e), "traceback": traceback.format_exc()})
        traceback.print_exc()
        return 3
    return 1 if findings else 0


# ---- the scenarios: contexts of 37 x 29 pixels on the small cover scene
class Scenario:
    root = 0                        # the context whose mrt_last_error names the refused call
    repeat = "act"                  # after a sound refusal: "act" repeats from the first step, "step" from the refused one

    def __init__(self, L, lib, api):
        self.L, self.lib = L, lib
        self.small, self.small_cam = api.scene_cover(1, True)
        self.n = len(self.small)

    def must(self, c, st, what):
        """a call that creates nothing the walk counts: any failure is unexpected"""
        if st != OK:
            raise Unexpected(f"{what}: status {st}: {(self.L.mrt_last_error(c) or b'').decode()}")

    def create(self, max_weight):
        args = self.lib.MrtArgs(W, H, 1, 6, max_weight)
        c = C.c_void_p()
        self.must(None, self.L.mrt_create(C.byref(args), 11, 0, C.byref(c)), "mrt_create")
        return c

    def set_scene(self, c):
        self.must(c, self.L.mrt_set_camera(c, C.byref(self.small_cam._c())), "mrt_set_camera")
        self.must(c, self.L.mrt_set_world(c, self.small.ctypes.data, self.n), "mrt_set_world")


class Temporal(Scenario):
    """On a prepared context (scene, camera, one frame; nothing of the denoiser yet) the act is mrt_set_temporal(1) plus the first
    mrt_temporal_step.  T: the guides' four buffers and the bitmap, the filter's three and the history's four.  The observable is
    mrt_read_temporal and the history."""
    what_differs = "the temporal image or the history differs"

    def prepare(self):
        c = self.create(0.0)
        self.set_scene(c)
        self.must(c, self.L.mrt_redraw(c), "mrt_redraw")
        return [c]

    def steps(self, ctxs):
        L, c = self.L, ctxs[0]
        return [lambda: L.mrt_set_temporal(c, 1, None), lambda: L.mrt_temporal_step(c)]

    def observe(self, ctxs):
        c = ctxs[0]
        img = np.zeros((H, W, 4), np.float32)
        h0, h1 = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
        prev = np.zeros((self.n, 4), np.float32)
        self.must(c, self.L.mrt_read_temporal(c, img.ctypes.data, img.size), "mrt_read_temporal")
        self.must(c, self.L.mrt_debug_read_temporal(c, h0.ctypes.data, h1.ctypes.data, prev.ctypes.data, max(H * W, self.n)), "mrt_debug_read_temporal")
        return hashlib.sha1(img.tobytes() + h0.tobytes() + h1[..., 2:].tobytes() + h1[..., :2].tobytes() + prev.tobytes()).hexdigest()


class TemporalResponse(Temporal):
    """Temporal's prepared context; the act is mrt_set_temporal_response (enabled 1; with --off enabled 0), mrt_set_temporal(1) and
    the first mrt_temporal_step.  T: Temporal's twelve and, with the response on, the fast history's two.  The observable is
    mrt_read_temporal, the history and, with the response on, the fast history."""
    enabled = 1

    def steps(self, ctxs):
        def set_response():
            r = self.lib.MrtTemporalResponse()
            self.L.mrt_temporal_response_default(C.byref(r))
            r.enabled = self.enabled
            return self.L.mrt_set_temporal_response(ctxs[0], C.byref(r))
        return [set_response] + super().steps(ctxs)

    def observe(self, ctxs):
        obs = super().observe(ctxs)
        if not self.enabled:
            return obs
        h2 = np.zeros((H, W, 4), np.float32)
        self.must(ctxs[0], self.L.mrt_debug_read_temporal_fast(ctxs[0], h2.ctypes.data, H * W), "mrt_debug_read_temporal_fast")
        return hashlib.sha1(obs.encode() + h2.tobytes()).hexdigest()


class GatherDenoise(Scenario):
    """On two prepared shards of one image on device 0 (noise tracking, scene, camera, one frame each; nothing gathered, nothing of
    the denoiser yet) the act is mrt_set_gather_noise(root, 1), mrt_gather, mrt_read_gathered_denoised on the root.  T: the
    gather's frame, the root's event and an event per shard, then the guides' four buffers and the bitmap and the filter's three.
    The observable is the gathered colour, the gathered S and the denoised image."""
    root = ROOT_RANK
    what_differs = "the gathered frame, its S or its denoise differs"

    def prepare(self):
        ctxs = []
        for r in range(WORLD):
            c = self.create(0.0)
            ctxs.append(c)
            self.must(c, self.L.mrt_set_shard(c, r, WORLD), "mrt_set_shard")
            self.must(c, self.L.mrt_set_noise_tracking(c, 1), "mrt_set_noise_tracking")
            self.set_scene(c)
            self.must(c, self.L.mrt_redraw(c), "mrt_redraw")
        return ctxs

    def steps(self, ctxs):
        L, R = self.L, ctxs[ROOT_RANK]
        arr = (C.c_void_p * WORLD)(*[c.value for c in ctxs])
        img = np.zeros((H, W, 4), np.float32)
        return [lambda: L.mrt_set_gather_noise(R, 1),
                lambda: L.mrt_gather(arr, WORLD, ROOT_RANK),
                lambda: L.mrt_read_gathered_denoised(R, img.ctypes.data, img.size)]

    def observe(self, ctxs):
        R = ctxs[ROOT_RANK]
        fb, den, s = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32)
        self.must(R, self.L.mrt_read_gathered(R, fb.ctypes.data, fb.size), "mrt_read_gathered")
        self.must(R, self.L.mrt_read_gathered_noise(R, s.ctypes.data, s.size), "mrt_read_gathered_noise")
        self.must(R, self.L.mrt_read_gathered_denoised(R, den.ctypes.data, den.size), "mrt_read_gathered_denoised")
        return hashlib.sha1(fb.tobytes() + s.tobytes() + den.tobytes()).hexdigest()


class DenoiseTiles(Scenario):
    """On a prepared context (noise tracking, scene, camera, two frames in flight at most and two frames rendered, so that both
    frame slots exist; nothing adaptive, nothing of the denoiser yet) the act is mrt_set_denoise_adaptive(1), mrt_render_tiles on
    half the tiles, mrt_read_denoised.  T: the first subset frame's three, the K tables' two and the denoiser's eight.  The
    observable is the framebuffer, S, the tiles' frame counts and the denoised image.  The refused call is repeated and the act
    goes on from it: a subset frame is not rendered twice."""
    repeat = "step"
    what_differs = "the framebuffer, S, the tiles' frame counts or the denoised image differ"

    def __init__(self, L, lib, api):
        super().__init__(L, lib, api)
        self.half = np.arange(TILES_X * TILES_Y // 2, dtype=np.uint32)

    def prepare(self):
        L = self.L
        c = self.create(1.0)
        self.must(c, L.mrt_set_noise_tracking(c, 1), "mrt_set_noise_tracking")
        self.set_scene(c)
        self.must(c, L.mrt_debug_set_frames_in_flight(c, 2), "mrt_debug_set_frames_in_flight")
        for _ in range(2):
            self.must(c, L.mrt_redraw(c), "mrt_redraw")
        self.must(c, L.mrt_sync(c), "mrt_sync")
        return [c]

    def steps(self, ctxs):
        L, c = self.L, ctxs[0]
        img = np.zeros((H, W, 4), np.float32)
        return [lambda: L.mrt_set_denoise_adaptive(c, 1),
                lambda: L.mrt_render_tiles(c, self.half.ctypes.data, self.half.size, 1),
                lambda: L.mrt_read_denoised(c, img.ctypes.data, img.size)]

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


SCENARIOS = {"temporal": Temporal, "temporal_response": TemporalResponse, "gather_denoise": GatherDenoise, "denoise_tiles": DenoiseTiles}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walk", choices=sorted(SCENARIOS), required=True)
    ap.add_argument("--log", required=True)
    ap.add_argument("--off", action="store_true", help="temporal_response: the response set, but not enabled")
    a = ap.parse_args()
    if a.off and a.walk != "temporal_response":
        ap.error("--off belongs to --walk temporal_response")

    def body(emit):
        from myraytracer_amd import _lib, api
        L = _lib.load()
        scenario = SCENARIOS[a.walk](L, _lib, api)
        if a.off:
            scenario.enabled = 0
        walk(L, Shim(L), scenario, emit)
    return logged_main(a.log, body)


if __name__ == "__main__":
    sys.exit(main())
