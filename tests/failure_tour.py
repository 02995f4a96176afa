"""The failure-injection tour: one scripted sequence of library calls that reaches every resource-creation site of the host
library, run in a child process of tests/test_gpu_failure_paths.py against lib/libmyraytracer_amd_failinject.so
(MRT_LIB_OVERRIDE; tests/failinject/).  The contract it holds is C1-C4 of include/myraytracer_amd.h, "after MRT_ERR_HIP".

    python tests/failure_tour.py --mode clean|destroy|continue --log FILE [--sites-out FILE] [--first N] [--last N]

clean     the tour once, disarmed: T (creator calls), the sites seen, every step's observable; nothing live, no violation after.
destroy   for N = 1 .. T: arm N, run until the armed call is refused, C1, destroy every context, C2.  Nothing is launched after
          the refusal.
continue  for N = 1 .. T: arm N, run until the refusal, C1 and C3 (mrt_debug_check_context on every context, host only), disarm,
          repeat the refused step, C3 again, finish the tour comparing every step's observable with the clean run's (C4),
          destroy, C2.  A context that fails C3 is destroyed without another launch and the case ends.
Both walks end by requiring that the sites at which a refusal was injected are the sites the clean run saw.

One JSON line per case is appended to the log before the next case starts.  The process stops (exit 3) at the first thing
that is neither an injected refusal nor a recorded finding: an unexpected status (MRT_ERR_STALLED and an MRT_ERR_HIP the shim
did not inject among them) or an exception.  Nothing is ever retried.  Exit 0: no finding; 1: findings (in the log)."""
import argparse
import ctypes as C
import hashlib
import json
import sys
import time

import numpy as np

from failure_walks import OK, H, W, Shim, Unexpected, c1_findings, logged_main      # (puts the repository on sys.path)


class Tour:
    def __init__(self):
        from myraytracer_amd import _lib, api
        self.lib, self.api = _lib, api
        self.L = _lib.load()
        self.shim = Shim(self.L)
        self.ctx = {}
        self.small, self.small_cam = api.scene_cover(1, True)
        self.large, self.large_cam = api.scene_stress(1, 40)
        self.tiny = api.scene_default()
        rng = np.random.default_rng(5)
        self.seeds = rng.integers(1, 2 ** 32, (H, W, 4), dtype=np.uint64).astype(np.uint32)
        self.last_seq = 0
        self.steps = self.build()

    # ---- the library
    def err(self, name):
        c = self.ctx.get(name)
        return (self.L.mrt_last_error(c) or b"").decode()

    def must(self, name, st, what):
        """a call of a step's prelude or tail that creates nothing: any failure is unexpected"""
        if st != OK:
            raise Unexpected(f"{what} on {name}: status {st}: {self.err(name)}")

    def check_contexts(self):
        """C3, host only: the first finding of mrt_debug_check_context over every context, or None"""
        why = C.create_string_buffer(512)
        for name, c in self.ctx.items():
            if self.L.mrt_debug_check_context(c, why, len(why)) != 0:
                return f"{name}: {why.value.decode()}"
        return None

    def destroy_all(self):
        for name in list(self.ctx):
            self.L.mrt_destroy(self.ctx.pop(name))

    def frames_done(self, name):
        return self.L.mrt_frames_done(self.ctx[name])

    # ---- steps: fn() -> (status, observable bytes or None); a step makes at most one kind of creating call and can be repeated
    def build(self):
        L, api, lib = self.L, self.api, self.lib
        steps = []

        def step(label, ctx_name):
            def deco(fn):
                steps.append((label, ctx_name, fn))
                return fn
            return deco

        def create(name, seed):
            @step(f"{name}: mrt_create", None)
            def _():
                args = lib.MrtArgs(W, H, 2, 6, 1.0)
                p = C.c_void_p()
                st = L.mrt_create(C.byref(args), seed, 0, C.byref(p))
                if st == OK:
                    self.ctx[name] = p
                elif p.value:
                    raise Unexpected(f"mrt_create failed with status {st} and left *out = {p.value:#x}")
                return st, None

        def simple(name, label, call, prelude=None):
            @step(f"{name}: {label}", name)
            def _():
                c = self.ctx[name]
                if prelude:
                    prelude(c)
                return call(c), None

        def set_world(name, label, spheres, cam, reset=False):
            def call(c):
                if reset:
                    self.must(name, L.mrt_reset(c), "mrt_reset")
                self.must(name, L.mrt_set_camera(c, C.byref(cam._c())), "mrt_set_camera")
                return L.mrt_set_world(c, spheres.ctypes.data, len(spheres))
            simple(name, label, call)

        def frames_to(name, label, target, prelude=None, batched=False, tiles=None):
            """whole frames (or frames of the listed tiles) until frames_done == target: repeated after a refusal, it renders
            what is still missing"""
            @step(f"{name}: {label}", name)
            def _():
                c = self.ctx[name]
                if prelude:
                    prelude(c)
                while self.frames_done(name) < target:
                    if tiles is not None:
                        st = L.mrt_render_tiles(c, tiles.ctypes.data, len(tiles), 1)
                    elif batched:
                        st = L.mrt_render(c, target - self.frames_done(name))
                    else:
                        st = L.mrt_redraw(c)
                    if st != OK:
                        return st, None
                return OK, None

        def observe(name, label="framebuffer, S, tile frames, counters"):
            """what a caller can read back (creates nothing)"""
            @step(f"{name}: read {label}", name)
            def _():
                c = self.ctx[name]
                rank, world, rows, width = (C.c_uint32() for _ in range(4))
                self.must(name, L.mrt_shard_info(c, C.byref(rank), C.byref(world), C.byref(rows), C.byref(width)), "mrt_shard_info")
                full = world.value == 1
                fb = np.zeros((H if full else rows.value, W, 4), np.float32)
                self.must(name, L.mrt_read_framebuffer(c, fb.ctypes.data, fb.size), "mrt_read_framebuffer")
                parts = [fb.tobytes()]
                s = np.zeros((H if full else rows.value, W), np.float32)
                st = L.mrt_read_noise(c, s.ctypes.data, s.size)
                if st == OK:
                    parts.append(s.tobytes())
                elif st != 7:
                    self.must(name, st, "mrt_read_noise")
                tf = np.zeros(64, np.uint32)
                self.must(name, L.mrt_read_tile_frames(c, tf.ctypes.data, tf.size, None, None), "mrt_read_tile_frames")
                parts.append(tf.tobytes())
                cnt = lib.MrtCounters()
                self.must(name, L.mrt_read_counters(c, C.byref(cnt)), "mrt_read_counters")
                loc = lib.MrtLocals()
                self.must(name, L.mrt_get_locals(c, C.byref(loc)), "mrt_get_locals")
                parts.append(repr((cnt.samples, cnt.world_hit_calls, cnt.rng_draws, self.frames_done(name), bytes(loc))).encode())
                return OK, b"".join(parts)

        def noise_query(name):
            simple(name, "mrt_noise_query", lambda c: L.mrt_noise_query(c, 0.02, 0.01))

            @step(f"{name}: mrt_noise_result", name)
            def _():
                r = lib.MrtNoiseReport()
                st = L.mrt_noise_result(self.ctx[name], 1, C.byref(r))
                self.last_seq = r.seq
                return st, bytes(r)

        def present(name, label, fmt, flags, prelude=None, tail=None):
            def call(c):
                st = L.mrt_present(c, fmt, flags)
                if st == OK and tail:
                    tail(c)
                return st
            simple(name, f"mrt_present {label}", call, prelude)

            @step(f"{name}: acquire / release {label}", name)
            def _():
                c = self.ctx[name]
                pix = C.POINTER(C.c_uint8)()
                info = lib.MrtPresentInfo()
                self.must(name, L.mrt_present_acquire(c, lib.ACQUIRE_NEWEST, 1, C.byref(pix), C.byref(info)), "mrt_present_acquire")
                if not pix:
                    raise Unexpected(f"{name}: nothing to acquire after a present")
                img = C.string_at(pix, info.rows * info.row_bytes)
                self.must(name, L.mrt_present_release(c), "mrt_present_release")
                meta = (info.seq, info.frames_done, info.width, info.rows, info.row_bytes, info.format, info.flags, info.dropped)
                return OK, img + repr(meta).encode()

        def read_denoised(name):
            @step(f"{name}: mrt_read_denoised", name)
            def _():
                out = np.zeros((H, W, 4), np.float32)
                return L.mrt_read_denoised(self.ctx[name], out.ctypes.data, out.size), out.tobytes()

        A = "A"
        create(A, 11)
        simple(A, "mrt_set_noise_tracking", lambda c: L.mrt_set_noise_tracking(c, 1))
        simple(A, "mrt_set_shard 0 / 1 (with tracking on)", lambda c: L.mrt_set_shard(c, 0, 1))
        set_world(A, "mrt_set_world small", self.small, self.small_cam)
        simple(A, "mrt_set_seeds", lambda c: L.mrt_set_seeds(c, self.seeds.ctypes.data, self.seeds.size))
        # the schedule pinned to (8, 2): sixteen frames in flight where the process runs them side by side (the stream
        # concurrency probe decides: 16, 8, 4 or 2), then sixteen slots whatever the probe said, then two for the rest
        frames_to(A, "3 frames at schedule (8, 2)", 3, lambda c: self.must(A, L.mrt_set_schedule_hint(c, 8, 2), "mrt_set_schedule_hint"))
        observe(A)

        def sixteen(c):
            self.must(A, L.mrt_set_schedule_hint(c, 0, 0), "mrt_set_schedule_hint")
            self.must(A, L.mrt_debug_set_frames_in_flight(c, 16), "mrt_debug_set_frames_in_flight")
        frames_to(A, "frame 4 with sixteen slots", 4, sixteen)
        frames_to(A, "frames 5, 6 with two slots", 6, lambda c: self.must(A, L.mrt_debug_set_frames_in_flight(c, 2), "mrt_debug_set_frames_in_flight"))

        def counter_mode(c):
            self.must(A, L.mrt_set_rng_mode(c, 1), "mrt_set_rng_mode")
            self.must(A, L.mrt_set_samples_per_frame(c, 130), "mrt_set_samples_per_frame")
        frames_to(A, "frames 7, 8: counter mode, 130 spp (3 layers of colour sums)", 8, counter_mode)
        observe(A)

        def stream_mode(form):
            def prelude(c):
                self.must(A, L.mrt_set_rng_mode(c, 0), "mrt_set_rng_mode")
                self.must(A, L.mrt_set_samples_per_frame(c, 2), "mrt_set_samples_per_frame")
                self.must(A, L.mrt_debug_set_frame_batching(c, form), "mrt_debug_set_frame_batching")
            return prelude
        frames_to(A, "frames 9 .. 13: one batch, a lane keeps its pixel", 13, stream_mode(2), batched=True)
        frames_to(A, "frames 14 .. 19: one batch, queue layers", 19, stream_mode(3), batched=True)
        observe(A)
        noise_query(A)
        present(A, "rgba8, flipped, ring of 2", lib.PRESENT_RGBA8_SRGB, lib.PRESENT_FLIP_Y,
                lambda c: self.must(A, L.mrt_set_present_ring(c, 2), "mrt_set_present_ring"))
        present(A, "bgra8, ring grown to 5", lib.PRESENT_BGRA8_SRGB, 0, lambda c: self.must(A, L.mrt_set_present_ring(c, 5), "mrt_set_present_ring"))
        present(A, "rgba8, copies on a stream of their own", lib.PRESENT_RGBA8_SRGB, 0,
                lambda c: self.must(A, L.mrt_debug_set_present_copy(c, 0), "mrt_debug_set_present_copy"),
                lambda c: self.must(A, L.mrt_debug_set_present_copy(c, 1), "mrt_debug_set_present_copy"))
        present(A, "denoised", lib.PRESENT_RGBA8_SRGB, lib.PRESENT_FLIP_Y | lib.PRESENT_DENOISED)
        read_denoised(A)
        n_waves = C.c_size_t()
        simple(A, "mrt_debug_wave_log (allocates the log)", lambda c: L.mrt_debug_wave_log(c, None, 0, C.byref(n_waves)))
        frames_to(A, "frame 20 with the wave log", 20, stream_mode(1))
        observe(A)
        # a large-layout scene in the small one's place
        set_world(A, "mrt_reset, mrt_set_world large", self.large, self.large_cam, reset=True)
        frames_to(A, "2 frames of the large scene", 2)
        observe(A)
        read_denoised(A)            # (more spheres: the guide pass' bitmap grows)
        tiles = np.array([0, 2, 5, 11, 19], np.uint32)
        frames_to(A, "2 frames of five tiles", 4, tiles=tiles)
        noise_query(A)              # (per tile now: the K tables)

        @step(f"{A}: mrt_render_adaptive", A)
        def _():
            used, sel = C.c_uint64(), C.c_uint32()
            st = L.mrt_render_adaptive(self.ctx[A], 1, self.last_seq, C.byref(used), C.byref(sel))
            return st, repr((used.value, sel.value)).encode() if st == OK else None
        observe(A)
        set_world(A, "mrt_reset, mrt_set_world small again", self.tiny, self.small_cam, reset=True)
        frames_to(A, "2 frames of the small scene", 2)
        observe(A)

        # ---- the debug entry points that allocate
        rng = np.random.default_rng(9)
        n = W * H
        rgba = rng.random((H, W, 4), dtype=np.float32)
        S = (rng.random((H, W), dtype=np.float32) * 0.01).astype(np.float32)
        guides = rng.random((n, 8), dtype=np.float32)

        @step(f"{A}: mrt_debug_noise_reduce", A)
        def _():
            r = lib.MrtNoiseReport()
            tiles_out = np.zeros(5 * 4, np.float32)
            st = L.mrt_debug_noise_reduce(self.ctx[A], S.ctypes.data, rgba.ctypes.data, W, H, 0.25, 0.02, 0.01, C.byref(r), tiles_out.ctypes.data)
            return st, bytes(r) + tiles_out.tobytes()

        plan_rng = np.random.default_rng(10)
        plan_s = np.exp(plan_rng.uniform(-9.0, 9.0, 70)).astype(np.float32)
        plan_n = plan_rng.integers(0, 41, 70).astype(np.uint32)         # (the K table's own sites are the per-tile query's, above)

        @step(f"{A}: mrt_debug_budget_plan", A)
        def _():
            r = lib.MrtBudgetResult()
            k = np.zeros(70, np.uint32)
            st = L.mrt_debug_budget_plan(self.ctx[A], plan_s.ctypes.data, plan_n.ctypes.data, 0, 70, 200, 8, k.ctypes.data, C.byref(r))
            return st, bytes(r) + k.tobytes()

        @step(f"{A}: mrt_debug_denoise", A)
        def _():
            out = np.zeros((H, W, 4), np.float32)
            st = L.mrt_debug_denoise(self.ctx[A], rgba.ctypes.data, S.ctypes.data, 0.25, guides.ctypes.data, W, H, None, out.ctypes.data)
            return st, out.tobytes()

        @step(f"{A}: mrt_debug_present_encode", A)
        def _():
            out = np.zeros((H, W, 4), np.uint8)
            st = L.mrt_debug_present_encode(self.ctx[A], rgba.ctypes.data, W, H, lib.PRESENT_BGRA8_SRGB, lib.PRESENT_FLIP_Y, out.ctypes.data)
            return st, out.tobytes()

        d = rng.standard_normal((70, 3)).astype(np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
        rays = np.ascontiguousarray(np.concatenate([np.tile(np.float32([0, 1, 3]), (70, 1)), d], axis=1), np.float32)

        @step(f"{A}: mrt_debug_world_hit", A)
        def _():
            hit = np.zeros((70, 2), np.int32)
            cand = np.zeros((70, 1), np.uint32)
            st = L.mrt_debug_world_hit(self.ctx[A], rays.ctypes.data, 70, hit.ctypes.data, cand.ctypes.data, 1)
            return st, hit.tobytes() + cand.tobytes()

        @step(f"{A}: mrt_debug_arith", A)
        def _():
            one = int(np.float32(1.0).view(np.uint32))
            rng4 = (C.c_uint32 * 4)(one, one + 1023, 0, 0)
            out = (C.c_uint64 * 3)()
            st = L.mrt_debug_arith(self.ctx[A], 0, rng4, 0, 1, out)
            return st, bytes(out)

        @step(f"{A}: mrt_debug_arith_pairs", A)
        def _():
            x = np.float32([1.0, 2.0, 3.0, 0.5])
            y = np.float32([3.0, 7.0, 0.25, 9.0])
            out = np.zeros((4, 6), np.uint32)
            st = L.mrt_debug_arith_pairs(self.ctx[A], x.ctypes.data, y.ctypes.data, 4, out.ctypes.data)
            return st, out.tobytes()

        @step(f"{A}: mrt_debug_stream_concurrency", A)
        def _():
            out = C.c_float()       # (how many streams ran side by side is scheduling: not compared)
            return L.mrt_debug_stream_concurrency(self.ctx[A], 16, C.byref(out)), None

        # ---- two shards of the image on the one device, gathered on the first
        for i, g in enumerate(("G0", "G1")):
            create(g, 11)
            simple(g, f"mrt_set_shard {i} / 2", lambda c, i=i: L.mrt_set_shard(c, i, 2))
            set_world(g, "mrt_set_world small", self.small, self.small_cam)
        simple("G0", "mrt_set_noise_tracking", lambda c: L.mrt_set_noise_tracking(c, 1))
        for g in ("G0", "G1"):
            frames_to(g, "2 frames", 2, lambda c, g=g: self.must(g, L.mrt_debug_set_frames_in_flight(c, 2), "mrt_debug_set_frames_in_flight"))
            observe(g)

        def gather(label, per_band):
            @step(f"G0: mrt_gather {label}", "G0")
            def _():
                self.must("G0", L.mrt_debug_set_gather_per_band(self.ctx["G0"], per_band), "mrt_debug_set_gather_per_band")
                arr = (C.c_void_p * 2)(self.ctx["G0"], self.ctx["G1"])
                return L.mrt_gather(arr, 2, 0), None

            @step(f"G0: mrt_read_gathered {label}", "G0")
            def _():
                out = np.zeros((H, W, 4), np.float32)
                return L.mrt_read_gathered(self.ctx["G0"], out.ctypes.data, out.size), out.tobytes()
        gather("in one copy", 0)
        gather("band by band", 1)
        present("G0", "the gathered frame", lib.PRESENT_RGBA8_SRGB, lib.PRESENT_FLIP_Y | lib.PRESENT_GATHERED)
        noise_query("G0")

        @step("G0: mrt_read_noise_tiles", "G0")
        def _():
            out = np.zeros(64, np.float32)
            tx, ty = C.c_uint32(), C.c_uint32()
            st = L.mrt_read_noise_tiles(self.ctx["G0"], out.ctypes.data, out.size, C.byref(tx), C.byref(ty))
            return st, out.tobytes() + repr((tx.value, ty.value)).encode()
        return steps

    # ---- one pass over the tour
    def run(self, n_arm, mode, clean_obs):
        """Returns the case's record.  mode: "clean", "destroy" or "continue"."""
        L, shim = self.L, self.shim
        rec = {"n": n_arm, "mode": mode, "findings": []}
        bad = rec["findings"].append
        self.last_seq = 0
        base = shim.live()
        L.mrt_fi_reset()
        L.mrt_fi_arm(n_arm)
        obs = []
        sound = True
        for i, (label, ctx_name, fn) in enumerate(self.steps):
            was_fired = shim.fired() is not None
            st, o = fn()
            site = shim.fired()
            if site is not None and not was_fired:                     # the armed call was refused in this step
                rec["site"], rec["step"] = site, label
                if st == OK:
                    raise Unexpected(f"{label}: a refused {site} was swallowed; the case cannot go on")
                rec["findings"] += c1_findings(site, st, self.err(ctx_name), label + ": ")
                if mode == "destroy":
                    break
                why = self.check_contexts()
                if why:
                    bad(f"C3: after the refusal at {site} in {label}: {why}")
                    sound = False
                    break
                L.mrt_fi_disarm()
                st, o = fn()                                           # C4: the call can be repeated
                if st != OK:
                    bad(f"C4: {label}: repeated after the refusal at {site}: status {st} ({self.err(ctx_name)})")
                    sound = False
                    break
                why = self.check_contexts()
                if why:
                    bad(f"C3: after {label} was repeated: {why}")
                    sound = False
                    break
            elif st != OK:
                raise Unexpected(f"{label}: status {st} that the shim did not inject: {self.err(ctx_name)}")
            h = hashlib.sha1(o).hexdigest() if o is not None else None
            obs.append(h)
            if clean_obs is not None and h != clean_obs[i]:
                bad(f"C4: {label}: differs from the run in which nothing was refused (after {rec.get('site', 'no refusal')})")
        L.mrt_fi_disarm()
        rec["reached"] = "site" in rec
        rec["calls"] = int(L.mrt_fi_calls())
        if mode == "clean":
            rec["sites"] = shim.sites()
        if not sound:
            rec["ended"] = "destroyed without another launch"
        self.destroy_all()
        live = shim.live()
        if live != base:
            bad(f"C2: live {{device, pinned, streams, events}} {live} after mrt_destroy, {base} before mrt_create"
                + (f" (refusal at {rec['site']})" if "site" in rec else ""))
        for v in shim.violations():
            bad("shim: " + v)
        return rec, obs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("clean", "destroy", "continue"), required=True)
    ap.add_argument("--log", required=True)
    ap.add_argument("--sites-out")
    ap.add_argument("--first", type=int, default=1)
    ap.add_argument("--last", type=int, default=0)
    a = ap.parse_args()
    from failure_sites import key_of, source_sites
    src = source_sites()

    def body(emit):
        t = Tour()
        t0 = time.time()
        clean, clean_obs = t.run(0, "clean", None)
        clean["seconds"] = round(time.time() - t0, 3)
        clean["keys"] = sorted({key_of(s, src) or ("? " + s) for s in clean["sites"]})
        emit(clean)
        T = clean["calls"]
        if a.sites_out:
            with open(a.sites_out, "w") as f:
                json.dump({"sites": clean["keys"]}, f, indent=1)
                f.write("\n")
        if a.mode == "clean" or clean["findings"]:
            return
        failed_at, not_reached = set(), 0
        last = a.last or T
        t0 = time.time()
        for n in range(a.first, last + 1):
            rec, _ = t.run(n, a.mode, clean_obs if a.mode == "continue" else None)
            emit(rec)
            if rec["reached"]:
                failed_at.add(rec["site"])
            else:
                not_reached += 1                  # (the tour made fewer calls this time: logged, no failure)
        summary = {"summary": a.mode, "T": T, "first": a.first, "last": last, "not_reached": not_reached,
                   "seconds": round(time.time() - t0, 3), "findings": []}
        if a.first == 1 and last == T:
            never = sorted(set(clean["sites"]) - failed_at)
            extra = sorted(failed_at - set(clean["sites"]))
            if never:
                summary["findings"].append(f"sites of the clean run at which no refusal was injected: {never}")
            if extra:
                summary["findings"].append(f"refusals at sites the clean run did not see: {extra}")
        emit(summary)
    return logged_main(a.log, body)


if __name__ == "__main__":
    sys.exit(main())
