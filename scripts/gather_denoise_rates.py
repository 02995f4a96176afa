#!/usr/bin/env python3
"""Dev helper (GPU box): what the noise estimate across shards costs (mrt_set_gather_noise, mrt_read_gathered_denoised).

Shards are contexts on device 0 (one MI355X): the copies are device-local, so this measures the queueing and the extra bytes,
NOT a link between GPUs -- cross-device numbers remain unmeasured.  Cover-glass scene, 1920x1080 x 1 spp, world 2 and 8.

  step   redraw of every shard + one mrt_gather, per step, wall time around `steps` steps that end in a sync of every context:
         the setting off on a library given with --parent-lib (the parent commit's build) against this tree's with the setting
         off, alternating, `reps` times each -- the expectation is the same within the run-to-run spread -- and this tree's with
         the setting on (a quarter more bytes);
  denoise  HIP events on the root's stream around one mrt_present, per source: the gathered frame, the gathered frame denoised
         (guides kept / rebuilt), and on the unsharded context in the same process its framebuffer and its denoised frame
         (guides kept / rebuilt).  Every window holds the same encode and the same copy of the 8-bit image; the difference to the
         plain present of its row is the guides + the filter.

Every figure comes from a child process of its own that loads ONE library through plain ctypes (the parent's build has no
mrt_set_gather_noise: the package's binding would refuse it).

    python scripts/gather_denoise_rates.py [--parent-lib FILE] [--out profiles/gather_denoise_rates.txt] [--steps 200] [--reps 3]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIS_LIB = os.path.join(ROOT, "myraytracer_amd", "lib", "libmyraytracer_amd.so")
W, H, SPP, DEPTH = 1920, 1080, 1, 50
FLIP, GATHERED, DENOISED, GATHERED_DENOISED = 1, 2, 8, 32


class Args(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("samples_per_frame", C.c_uint32), ("ray_depth", C.c_uint32),
                ("max_framebuffer_weight", C.c_float)]


class Lib:
    def __init__(self, path):
        self.L = L = C.CDLL(path)
        vp, u32, u64, i32, sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_size_t
        for name, res, args in (("mrt_create", i32, [C.POINTER(Args), u64, i32, C.POINTER(vp)]), ("mrt_destroy", None, [vp]),
                                ("mrt_set_shard", i32, [vp, u32, u32]), ("mrt_set_world", i32, [vp, vp, sz]),
                                ("mrt_set_camera", i32, [vp, vp]), ("mrt_set_noise_tracking", i32, [vp, i32]),
                                ("mrt_redraw", i32, [vp]), ("mrt_sync", i32, [vp]), ("mrt_set_stream", i32, [vp, vp]),
                                ("mrt_gather", i32, [C.POINTER(vp), u32, u32]), ("mrt_present", i32, [vp, i32, u32]),
                                ("mrt_scene_cover", i32, [u64, i32, vp, sz, vp]), ("mrt_last_error", C.c_char_p, [vp])):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        self.has_setting = hasattr(L, "mrt_set_gather_noise")
        if self.has_setting:
            L.mrt_set_gather_noise.restype, L.mrt_set_gather_noise.argtypes = i32, [vp, i32]
        self.spheres = C.create_string_buffer(36 * 4096)
        self.cam = C.create_string_buffer(52)
        self.n = L.mrt_scene_cover(1, 1, self.spheres, 4096, self.cam)
        assert self.n > 0

    def must(self, c, st, what):
        if st != 0:
            sys.exit(f"{what}: status {st}: {(self.L.mrt_last_error(c) or b'').decode()}")

    def context(self, shard=None, stream=None):
        L, c = self.L, C.c_void_p()
        args = Args(W, H, SPP, DEPTH, 1.0)
        self.must(None, L.mrt_create(C.byref(args), 1, 0, C.byref(c)), "mrt_create")
        if stream is not None:
            self.must(c, L.mrt_set_stream(c, stream), "mrt_set_stream")
        if shard is not None:
            self.must(c, L.mrt_set_shard(c, shard[0], shard[1]), "mrt_set_shard")
        self.must(c, L.mrt_set_noise_tracking(c, 1), "mrt_set_noise_tracking")
        self.must(c, L.mrt_set_world(c, self.spheres, self.n), "mrt_set_world")
        self.must(c, L.mrt_set_camera(c, self.cam), "mrt_set_camera")
        return c

    def step(self, ctxs, arr):
        for c in ctxs:
            self.must(c, self.L.mrt_redraw(c), "mrt_redraw")
        self.must(ctxs[0], self.L.mrt_gather(arr, len(ctxs), 0), "mrt_gather")

    def sync(self, ctxs):
        for c in ctxs:
            self.must(c, self.L.mrt_sync(c), "mrt_sync")


def child_step(a):
    lib = Lib(a.lib)
    ctxs = [lib.context((r, a.world)) for r in range(a.world)]
    arr = (C.c_void_p * a.world)(*[c.value for c in ctxs])
    if a.setting:
        lib.must(ctxs[0], lib.L.mrt_set_gather_noise(ctxs[0], 1), "mrt_set_gather_noise")
    for _ in range(a.warmup):
        lib.step(ctxs, arr)
    lib.sync(ctxs)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        lib.step(ctxs, arr)
    lib.sync(ctxs)
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    for c in ctxs:
        lib.L.mrt_destroy(c)
    print(json.dumps({"ms_per_step": ms}))


def child_denoise(a):
    lib = Lib(a.lib)
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    for name, args in (("hipStreamCreate", [C.POINTER(vp)]), ("hipEventCreate", [C.POINTER(vp)]), ("hipEventRecord", [vp, vp]),
                       ("hipEventSynchronize", [vp]), ("hipEventElapsedTime", [C.POINTER(C.c_float), vp, vp])):
        getattr(hip, name).restype, getattr(hip, name).argtypes = C.c_int, args

    def ok(rc, what):
        if rc != 0:
            sys.exit(f"{what} -> {rc}")
    stream, e0, e1 = vp(), vp(), vp()
    ok(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    one = lib.context(stream=stream)
    ctxs = [lib.context((r, a.world), stream=stream if r == 0 else None) for r in range(a.world)]
    arr = (C.c_void_p * a.world)(*[c.value for c in ctxs])
    lib.must(ctxs[0], lib.L.mrt_set_gather_noise(ctxs[0], 1), "mrt_set_gather_noise")
    for _ in range(4):
        lib.must(one, lib.L.mrt_redraw(one), "mrt_redraw")
        lib.step(ctxs, arr)
    lib.sync(ctxs + [one])

    def window(c, flags, stale):
        out = []
        for k in range(a.warmup + a.steps):
            if stale:
                lib.must(c, lib.L.mrt_set_camera(c, lib.cam), "mrt_set_camera")      # the guides go stale: the rebuild is in the window
            ok(hip.hipEventRecord(e0, stream), "hipEventRecord")
            lib.must(c, lib.L.mrt_present(c, 1, flags | FLIP), "mrt_present")
            ok(hip.hipEventRecord(e1, stream), "hipEventRecord")
            ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
            if k >= a.warmup:
                out.append(ms.value)
        return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "n": len(out)}
    R = ctxs[0]
    res = {"gathered, plain": window(R, GATHERED, False),
           "gathered, denoised, guides kept": window(R, GATHERED_DENOISED, False),
           "gathered, denoised, guides rebuilt": window(R, GATHERED_DENOISED, True),
           "unsharded, plain": window(one, 0, False),
           "unsharded, denoised, guides kept": window(one, DENOISED, False),
           "unsharded, denoised, guides rebuilt": window(one, DENOISED, True)}
    for c in ctxs + [one]:
        lib.L.mrt_destroy(c)
    print(json.dumps(res))


def run_child(extra):
    env = dict(os.environ)
    env.setdefault("GPU_MAX_HW_QUEUES", "20")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(x) for x in extra], capture_output=True, text=True,
                       timeout=300, env=env)
    if p.returncode != 0:
        sys.exit(f"child {extra} ended with {p.returncode}: {p.stdout[-1000:]}{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("step", "denoise"))
    ap.add_argument("--lib", default=THIS_LIB)
    ap.add_argument("--parent-lib")
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--setting", type=int, default=0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_denoise_rates.txt"))
    a = ap.parse_args()
    if a.child == "step":
        return child_step(a)
    if a.child == "denoise":
        return child_denoise(a)
    lines = [f"gather_denoise_rates.py: cover-glass, {W}x{H} x {SPP} spp, depth {DEPTH}; shards are contexts on device 0 of ONE MI355X "
             "(device-local copies: cross-device numbers remain unmeasured)",
             f"step = redraw of every shard + one mrt_gather; wall ms per step over {a.steps} steps ending in a sync, after {a.warmup} warm-up "
             f"steps; {a.reps} alternating repetitions, each in a process of its own"]
    for world in (2, 8):
        kinds = ([("parent commit, no setting", a.parent_lib, 0)] if a.parent_lib else []) + \
                [("this commit, setting off", THIS_LIB, 0), ("this commit, setting on", THIS_LIB, 1)]
        got = {k[0]: [] for k in kinds}
        for _ in range(a.reps):
            for name, lib, setting in kinds:          # alternating: every kind once per repetition
                got[name].append(run_child(["step", "--lib", lib, "--world", world, "--setting", setting, "--steps", a.steps,
                                            "--warmup", a.warmup])["ms_per_step"])
        lines.append(f"world {world}:")
        for name, v in got.items():
            lines.append(f"    {name:28s} median {statistics.median(v):8.3f} ms per step   (runs: {', '.join(f'{x:.3f}' for x in v)}; "
                         f"spread {max(v) - min(v):.3f})")
        colour = W * ((H + 7) // 8 * 8) * 16
        lines.append(f"    bytes gathered per step: {colour} of colour, + {colour // 4} of S with the setting on")
    lines.append(f"denoise = HIP events on the root's stream around ONE mrt_present (rgba8, flipped; the window holds the encode and the copy "
                 f"of the 8-bit image too), median of {a.steps} after {a.warmup}, ms (min .. max):")
    for world in (2, 8):
        res = run_child(["denoise", "--world", world, "--steps", a.steps, "--warmup", a.warmup])
        lines.append(f"world {world}:")
        for name, r in res.items():
            lines.append(f"    {name:38s} {r['median_ms']:8.3f}   ({r['min_ms']:.3f} .. {r['max_ms']:.3f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
