"""Stream-ordering scenarios: hold one stream of a context, queue producer and consumer calls with no sync between them, and
compare what a caller reads back with the oracle's frames.  Run in-process against the product library by
tests/test_gpu_stream_order.py, and in a child process (failure_sites.run_child) against
lib/libmyraytracer_amd_failinject.so, whose shim (tests/failinject/) can drop ONE hipStreamWaitEvent of the library:

    python tests/order_walks.py --scenarios NAME[,NAME...]|all --log FILE [--record tests/golden/order_sites.json]

A scenario prepares fresh contexts -- scene, camera, the frames in flight pinned, the feature warmed up once so that no buffer,
stream or event is created afterwards, a sync -- then holds a stream with mrt_debug_hold, queues its calls and reads an
observable.  The expected observable comes from the oracle (oracle/pyoracle.py) and the float32 restatements tests/noise_ref.py
and tests/present_ref.py, never from a second run of the library.  In the child every scenario runs clean first and counts its W
stream waits, from the hold to the last read-back (that run must equal the reference: else a finding), then for N = 1 .. W on
fresh contexts with the N-th wait dropped; the case is DETECTED if the observable differs from the reference.  Every scenario
names the wait it is built to miss (`misses`, a piece of the site's source line): there the held stream makes the detection
certain, and only those detections are recorded in tests/golden/order_sites.json and asserted; a dropped wait between two
streams that both run is detected or not as the race falls out, and is logged only.  One JSON line per case is appended to the log before
the next case starts; nothing is retried.  Exit 0: no finding; 1: findings (in the log); 3: stopped on a status that is not
MRT_OK, or an exception.

A dropped wait only ever changes values: the held stream's work has not begun while the other streams' work runs to completion,
so every kernel sees whole arrays of unchanged size, stale or too new; no scenario allocates, frees, resizes or changes the sphere
count between its hold and its last sync.  Each scenario's docstring says why no index or pointer a kernel follows can change.

The hold must outlast the host's queueing of the scenario's calls and the work they start on the streams that run on.  Measured on
an MI355X with the product library (`python tests/order_walks.py --measure` prints the figures): with a hold of ONE tick, the time
from just before the hold is queued to the return of the last read-back -- the host's queueing, all the work on the device and the
host's polling for it -- was at most MEASURED_UNHELD_MS below (gather: three contexts' frames and the copies; 0.23 - 1.39 ms for
the others), of which the queueing alone took at most 0.54 ms (0.03 - 0.13 ms but for the process' first calls); and a hold bounded by
its polls alone showed MEASURED_POLLS_PER_MS polls per millisecond between its two stamps.  The queueing time alone is too short a
yardstick: a hold of four times it, 1.3 ms, ended before the root had read the gathered frame, and the dropped wait behind that
read went unnoticed.  HOLD_TICKS is four times the end-to-end figure (100 ticks a microsecond: 1,359,600 ticks, 13.6 ms), HOLD_POLLS
four times the polls of that span (61,942), so the clock bound comes first and the poll bound still ends the kernel; both are far
below the call's cap (MRT_HOLD_MAX_TICKS, half a second).  Every case checks itself: queueing that took more than half the hold,
or a hold whose stamps show less than its ticks, fails the case as inconclusive."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import noise_ref  # noqa: E402
import present_ref  # noqa: E402
from common import to_oracle_camera, to_oracle_spheres  # noqa: E402
from failure_walks import Unexpected, logged_main  # noqa: E402

MEASURED_UNHELD_MS = 3.399          # gather (3.384 - 3.399 over four runs)
MEASURED_POLLS_PER_MS = 1139.0      # 4,096 polls between stamps 359,668 ticks apart (1,137.4 - 1,138.8 over three runs)
HOLD_TICKS = int(4 * MEASURED_UNHELD_MS * 100_000)
HOLD_POLLS = int(4 * 4 * MEASURED_UNHELD_MS * MEASURED_POLLS_PER_MS)
W, H, SPP, DEPTH, SEED = 37, 29, 2, 6, 11       # ragged: 5 tile columns (the last 5 pixels wide), 4 bands (the last 5 rows high)
COUNTER_KEYS = ("samples", "world_hit_calls", "rng_draws")
NOISE_THRESHOLD, NOISE_FLOOR = 0.05, 0.01
WORLD, ROOT_RANK = 3, 1             # the gather's shards, and the one that gathers


class Env:
    """what a scenario needs: the package, its loaded library, the oracle, the shim (None on the product library)"""

    def __init__(self, mrt, oracle, shim=None):
        from myraytracer_amd import _lib
        self.mrt, self.O, self.shim, self.L = mrt, oracle, shim, _lib.load()
        self._scenes, self._refs = {}, {}

    def scene(self, layout):
        """(spheres, camera, forced hierarchy) of "small" (the cover scene with glass) or "large" (1,100 spheres of one radius
        over a radius-1000 ground, hierarchy (4, 32): three levels and the boxes, as tests/test_gpu_update_spheres.py's)"""
        if layout not in self._scenes:
            mrt = self.mrt
            if layout == "small":
                sc, cam = mrt.scene_cover(1, True)
                forced = None
            else:
                n = 1100
                rng = np.random.default_rng(n)
                sc = np.zeros(n, mrt.SPHERE_DTYPE)
                sc["center"][:n - 1] = (rng.uniform(-8, 8, (n - 1, 3)) * [1.0, 0.15, 1.0]).astype(np.float32)
                sc["radius"][:n - 1] = 0.2
                sc["material_ty"] = 1 + np.arange(n) % 3
                sc["albedo"] = rng.uniform(0.2, 0.9, (n, 3)).astype(np.float32)
                sc["param"] = np.where(sc["material_ty"] == 3, 1.5, 0.1).astype(np.float32)
                sc["center"][n - 1], sc["radius"][n - 1], sc["material_ty"][n - 1] = (0.0, -1002.0, 0.0), 1000.0, 1
                cam = mrt.Camera(mode=1, lookfrom=(0.0, 2.5, 13.0), lookat=(0.0, 0.0, 0.0), vup=(0.0, 1.0, 0.0), vfov_deg=40.0,
                                 defocus_angle_deg=0.0, focus_dist=10.0)
                forced = (4, 32)
            self._scenes[layout] = (sc, cam, forced)
        sc, cam, forced = self._scenes[layout]
        return sc.copy(), cam, forced

    def moved(self, sc):
        """the scene with every sphere but the last (a ground) moved by up to 0.3, and its (n, 4) centres and radii"""
        rng = np.random.default_rng(len(sc) + 1)
        out = sc.copy()
        out["center"][:-1] += rng.uniform(-0.3, 0.3, (len(sc) - 1, 3)).astype(np.float32)
        return out, np.concatenate([out["center"], out["radius"][:, None]], axis=1).astype(np.float32)

    def scattered(self, sc):
        """the scene with every sphere but the grounds (radius above 100) placed anywhere in the box of their centres, so that the
        bounds of the kept grouping loosen many times over, and its (n, 4) centres and radii"""
        rng = np.random.default_rng(len(sc) + 3)
        out = sc.copy()
        small = np.abs(sc["radius"]) <= 100.0
        c = sc["center"][small].astype(np.float64)
        out["center"][small] = rng.uniform(c.min(0), c.max(0), c.shape).astype(np.float32)
        return out, np.concatenate([out["center"], out["radius"][:, None]], axis=1).astype(np.float32)

    def repainted(self, sc):
        """the scene with every sphere's material changed: the types rotated, new albedos"""
        rng = np.random.default_rng(len(sc) + 2)
        out = sc.copy()
        out["material_ty"] = 1 + (sc["material_ty"] % 3)
        out["albedo"] = rng.uniform(0.1, 0.95, (len(sc), 3)).astype(np.float32)
        out["param"] = np.where(out["material_ty"] == 3, 1.5, 0.3).astype(np.float32)
        return out

    def frames(self, frames, means=False):
        """the oracle's accumulation (max weight 1) of frame f = (spheres, camera) over the full image and its counters; means:
        the frames' own means instead, for tests/noise_ref.py"""
        O = self.O
        seeds = O.fill_seeds(SEED, W, H)
        cnt = O.Counters()
        fb, out = np.zeros((H, W, 4), np.float32), []
        for f, (sc, cam) in enumerate(frames):
            packed = O.pack_world(to_oracle_spheres(O, sc))
            if means:
                out.append(O.render_frame(W, H, SPP, DEPTH, packed, to_oracle_camera(O, cam), seeds, O.frame_shuffle(SEED, f), 0.0))
            else:
                fb = O.render_frame(W, H, SPP, DEPTH, packed, to_oracle_camera(O, cam), seeds, O.frame_shuffle(SEED, f),
                                    O.frame_weight(f, 1.0), fb, counters=cnt)
        return out if means else (fb, {k: int(cnt.as_dict()[k]) for k in COUNTER_KEYS})

    def reference(self, scenario):
        if scenario.name not in self._refs:
            self._refs[scenario.name] = scenario.reference()
        return self._refs[scenario.name]


class Clock:
    """the host time from just before the hold is queued to mark() -- or to the end of the act"""

    def __init__(self, ticks=None):
        self.t0 = self.t1 = None
        self.held = None
        self.ticks = HOLD_TICKS if ticks is None else ticks

    def hold(self, st, which, index=0):
        assert self.t0 is None, "one hold a case"
        self.held = st
        self.t0 = time.perf_counter()
        st.debug_hold(which, index, self.ticks, HOLD_POLLS)

    def mark(self):
        if self.t1 is None:
            self.t1 = time.perf_counter()

    @property
    def queue_ms(self):
        return (self.t1 - self.t0) * 1e3


def differs(got, ref):
    """the keys at which two observables differ: arrays bit for bit, Python floats to 1e-12 relative (the report's float64 sums,
    as tests/test_gpu_noise.py takes them), everything else exactly"""
    out = [k for k in ref if k not in got] + [k for k in got if k not in ref]
    for k in ref:
        if k not in got:
            continue
        a, b = got[k], ref[k]
        if isinstance(b, np.ndarray):
            same = isinstance(a, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
        elif isinstance(b, float):
            same = isinstance(a, float) and (a == b or abs(a - b) <= 1e-12 * max(abs(b), 1e-300))
        else:
            same = a == b
        if not same:
            out.append(k)
    return out


class Scenario:
    layout, slots = "small", 2
    misses = None                   # a piece of the source line of the stream wait whose loss the scenario is built to detect

    def __init__(self, env, name):
        self.env, self.name = env, name
        self.old, self.cam, self.forced = env.scene(self.layout)

    def state(self, **kw):
        """a context with the scene and the camera, the frames in flight pinned"""
        mrt = self.env.mrt
        st = mrt.State(mrt.Args(W, H, SPP, DEPTH, 1.0), seed=SEED, **kw)
        if self.forced:
            st.debug_set_hierarchy(*self.forced)
            st.debug_set_boxes(2)
        self.configure(st)
        st.set_world(self.old)
        st.set_camera(self.cam)
        st.debug_set_frames_in_flight(self.slots)
        return st

    def configure(self, st):
        pass

    def observe(self, sts, seen):
        st = sts[0]
        seen["framebuffer"] = st.read_framebuffer()
        seen.update(st.read_counters())
        for k in [k for k in seen if k in ("lane_slots", "member_tests", "sweep_records")]:
            del seen[k]

    def image_reference(self, frames):
        fb, cnt = self.env.frames(frames)
        return dict(framebuffer=fb, **cnt)


class Change(Scenario):
    """what the input scenarios share: `kind` names the call that changes the scene -- "spheres" (mrt_update_spheres), "materials"
    (mrt_update_materials), "regroup" (mrt_update_spheres then mrt_regroup_spheres), "auto" (mrt_set_auto_regroup judging every
    update: the spheres scattered, and the same update again, whose judgement sees the loosened bounds and opens the gate of the
    regroup queued behind it -- once, or the child stops); "+garbage": the caller's array is overwritten as soon as the call has
    returned ("may be reused as soon as it returns")"""

    def __init__(self, env, name, kind, layout="small"):
        self.layout = layout
        super().__init__(env, name)
        self.kind, self.garbage = kind.split("+")[0], kind.endswith("+garbage")
        self.old_xyzr = np.concatenate([self.old["center"], self.old["radius"][:, None]], axis=1).astype(np.float32)
        if self.kind == "materials":
            self.new = env.repainted(self.old)
        elif self.kind == "auto":
            self.new, self.new_xyzr = env.scattered(self.old)
        else:
            self.new, self.new_xyzr = env.moved(self.old)

    def configure(self, st):
        if self.kind == "auto":
            st.set_auto_regroup(True, check_every=1)

    def observe(self, sts, seen):
        super().observe(sts, seen)
        if self.kind == "auto":
            stats = sts[0].read_regroup_stats()
            if stats["regroups"] != 1:
                raise Unexpected(f"{self.name}: the gate opened {stats['regroups']} times, not once: {stats}")

    def change(self, st, new=True):
        if self.kind == "materials":
            arr = np.ascontiguousarray(self.env.mrt.materials_of(self.new if new else self.old)).copy()
            st.update_materials(0, arr)
            if self.garbage:
                arr.view(np.uint8)[:] = 0xFF
        else:
            arr = (self.new_xyzr if new else self.old_xyzr).copy()
            st.update_spheres(0, arr)
            if self.garbage:
                arr[:] = np.float32(3.0e30)
            if self.kind == "regroup":
                st.regroup_spheres()
            if self.kind == "auto":
                st.update_spheres(0, (self.new_xyzr if new else self.old_xyzr).copy())

    def prepare(self):
        st = self.state()
        for _ in range(2):
            st.redraw()
        self.change(st, new=False)          # the warm-up: the feature's buffers, with the scene as it is
        st.sync()
        return [st]


class InputsToRender(Change):
    """Two frames of the old scene; the context's stream is held; the change is queued behind the hold and a frame behind the
    change.  The frame shows the new input (frames.cpp, enter_slot: the side stream waits for ev_inputs).  A dropped wait lets the
    render run before the change, or the blend before the render: a refit rewrites bounds and records, not indices, a regroup
    permutes valid member indices (a gated one too), a material update rewrites shade records, and the render has ended before the held change
    begins, so it reads whole arrays of the old scene; the blend reads the slot's colour sums, whose address never changes."""

    misses = "hipStreamWaitEvent(S.stream, c->ev_inputs, 0)"

    def act(self, sts, clock):
        clock.hold(sts[0], "context")
        self.change(sts[0])
        sts[0].redraw()

    def reference(self):
        return self.image_reference([(self.old, self.cam)] * 2 + [(self.new, self.cam)])


class RenderToScatter(Change):
    """Two frames of the old scene; slot 0's side stream is held and frame 2 queued on it, then the change, then frame 3: the
    accumulation is the oracle's blend of three old frames and a new one (world.cpp, order_behind_frames, and the blend's wait for
    render_done).  A dropped wait lets the change or a blend run ahead of the held render, which then reads the new arrays whole:
    the same sizes, bounds and records rewritten in place, member indices permuted among valid ones."""

    misses = "hipStreamWaitEvent(c->stream, S.render_done, 0));"      # (launch_frame's; order_behind_frames' is implied by it)

    def act(self, sts, clock):
        clock.hold(sts[0], "slot", 0)
        sts[0].redraw()
        self.change(sts[0])
        sts[0].redraw()

    def reference(self):
        return self.image_reference([(self.old, self.cam)] * 3 + [(self.new, self.cam)])


class RenderToBlend(Scenario):
    """Two frames; slot 0's side stream is held, frame 2 queued on it and read back: the blend used frame 2's colour sums
    (frames.cpp, launch_frame: the context's stream waits for render_done).  A dropped wait lets the blend read the sums frame 0
    left in the same buffer: the address is the slot's, only the values are stale."""

    misses = "hipStreamWaitEvent(c->stream, S.render_done, 0));"

    def prepare(self):
        st = self.state()
        for _ in range(2):
            st.redraw()
        st.sync()
        return [st]

    def act(self, sts, clock):
        clock.hold(sts[0], "slot", 0)
        sts[0].redraw()

    def reference(self):
        return self.image_reference([(self.old, self.cam)] * 3)


class SlotReuse(RenderToBlend):
    """Two frames in flight; the context's stream is held ahead of frame 2's blend and frames 2, 3 and 4 are queued: frame 4
    renders into slot 0's colour sums only after frame 2's blend has read them (frames.cpp, enter_slot: the side stream waits for
    the slot's finalize_done).  A dropped wait lets frame 4 overwrite the sums first: same buffer, same size, other values."""

    misses = "hipStreamWaitEvent(S.stream, S.finalize_done, 0)"

    def act(self, sts, clock):
        clock.hold(sts[0], "context")
        for _ in range(3):
            sts[0].redraw()

    def reference(self):
        return self.image_reference([(self.old, self.cam)] * 5)


class CameraTables(Scenario):
    """Three frames in flight with the camera-ray tables forced on (`table`: 2 the sphere lists, 3 the cluster masks) and built by
    every slot over six frames; slot 0's side stream is held and frame 6 queued on it with camera A; mrt_set_camera(B); frames 7
    (which runs without tables: the first of its generation) and 8, whose slot builds B's tables -- behind slot 0's frame
    (frames.cpp, camera_masks: a build for a new generation waits for the other slots' frames).  Frame 6 is the oracle's for
    camera A.  A dropped wait lets the build overwrite the tables before frame 6 reads them: a list entry then holds B's member
    slots, which are valid level-0 slots of the same scene (or the all-ones overflow word), a mask entry B's bits over the same
    top records; no size changes."""
    slots = 3
    misses = "hipStreamWaitEvent(S.stream, T.render_done, 0)"

    def __init__(self, env, name, table):
        super().__init__(env, name)
        self.table = table
        mrt = env.mrt
        a = self.cam
        self.cam_b = mrt.Camera(mode=1, lookfrom=(-float(a.lookfrom[2]), float(a.lookfrom[1]) + 1.0, float(a.lookfrom[0])),
                                lookat=tuple(float(v) for v in a.lookat), vup=(0.0, 1.0, 0.0), vfov_deg=float(a.vfov_deg) * 0.8,
                                defocus_angle_deg=float(a.defocus_angle_deg), focus_dist=float(a.focus_dist))

    def configure(self, st):
        st.debug_set_camera_masks(self.table)

    def prepare(self):
        st = self.state()
        for _ in range(6):
            st.redraw()
        st.sync()
        info = st.debug_read_camera_masks(table=False)
        if not (info["in_force"] and info["built"] and info["lists"] == (self.table == 2)):
            raise Unexpected(f"{self.name}: the warm-up's last frame did not run with the tables asked for: {info}")
        return [st]

    def act(self, sts, clock):
        st = sts[0]
        clock.hold(st, "slot", 0)
        st.redraw()
        st.set_camera(self.cam_b)
        st.redraw()
        st.redraw()

    def observe(self, sts, seen):
        super().observe(sts, seen)
        info = sts[0].debug_read_camera_masks(table=False)
        if not (info["in_force"] and info["built"]):
            raise Unexpected(f"{self.name}: frame 8 did not run with tables built for camera B: {info}")

    def reference(self):
        return self.image_reference([(self.old, self.cam)] * 7 + [(self.old, self.cam_b)] * 2)


class Present(Scenario):
    """The present's copy on a stream of its own (mrt_debug_set_present_copy(0)), warmed up by one present.  `held` ("context" or
    "present") is held, a frame and its present are queued: mrt_present_acquire(wait = 0) returns no image while the hold runs,
    wait = 1 returns exactly present_ref.encode_host of the oracle's frame (present.cpp: the present stream waits for the encode).
    A dropped wait lets the copy read the entry's device image before the encode has written it: a copy of fixed size between two
    buffers of the ring entry, stale bytes at worst."""

    def __init__(self, env, name, held):
        super().__init__(env, name)
        self.held = held
        if held == "context":               # (with the present stream itself held the copy comes late whatever it waits for)
            self.misses = "hipStreamWaitEvent(c->present_stream, c->ev_presented, 0)"

    def configure(self, st):
        st.debug_set_present_copy(0)

    def prepare(self):
        st = self.state()
        for _ in range(2):
            st.redraw()
        st.present()
        if st.acquire_presented(wait=True) is None:
            raise Unexpected("the warm-up's present gave no image")
        st.release_presented()
        st.sync()
        return [st]

    def act(self, sts, clock):
        st = sts[0]
        clock.hold(st, self.held)
        st.redraw()
        st.present()
        clock.mark()
        self.polled = st.acquire_presented(wait=False)

    def observe(self, sts, seen):
        seen["nothing while the hold runs"] = self.polled is None
        got = sts[0].acquire_presented(newest=False, wait=True)
        if got is None:                     # (no image is left where the poll took it: an observable that differs)
            got = (None, {"seq": 0, "frames_done": 0, "dropped": 0})
        seen["image"], seen["seq"], seen["frames_done"], seen["dropped"] = got[0], got[1]["seq"], got[1]["frames_done"], got[1]["dropped"]

    def reference(self):
        fb, _ = self.env.frames([(self.old, self.cam)] * 3)
        return {"nothing while the hold runs": True, "image": present_ref.encode_host(self.env.L, fb, "rgba8", True), "seq": 2,
                "frames_done": 3, "dropped": 0}


class PresentRing(Present):
    """A ring of two entries, both warmed up; the context's stream is held and three frames are presented.  The third present finds
    both entries' copies in flight and waits on the host for the older one -- so it returns only when the hold has ended (the clock
    stops before it) -- drops that image and reuses its entry: the two images acquired afterwards are the second and the third
    frame's, each exactly its encode_host, with one image dropped.  A dropped wait changes which bytes a fixed-size copy finds."""

    def __init__(self, env, name):
        super().__init__(env, name, "context")

    def configure(self, st):
        st.debug_set_present_copy(0)
        st.set_present_ring(2)

    def prepare(self):
        st = self.state()
        for _ in range(2):
            st.redraw()
        for _ in range(2):
            st.present()
        for _ in range(2):
            if st.acquire_presented(newest=False, wait=True) is None:
                raise Unexpected("the warm-up's presents gave no image")
        st.release_presented()
        st.sync()
        return [st]

    def act(self, sts, clock):
        st = sts[0]
        clock.hold(st, "context")
        for _ in range(2):
            st.redraw()
            st.present()
        clock.mark()
        self.polled = st.acquire_presented(wait=False)
        st.redraw()
        st.present()

    def observe(self, sts, seen):
        seen["nothing while the hold runs"] = self.polled is None
        for k in ("second", "third"):
            got = sts[0].acquire_presented(newest=False, wait=True)
            if got is None:
                got = (None, {"seq": 0, "frames_done": 0, "dropped": 0})
            seen[k], seen[k + " seq"], seen[k + " frames_done"] = got[0], got[1]["seq"], got[1]["frames_done"]
            if k == "second":
                seen["dropped"] = got[1]["dropped"]

    def reference(self):
        enc = present_ref.encode_host
        fb4, _ = self.env.frames([(self.old, self.cam)] * 4)
        fb5, _ = self.env.frames([(self.old, self.cam)] * 5)
        return {"nothing while the hold runs": True, "second": enc(self.env.L, fb4, "rgba8", True), "second seq": 4, "second frames_done": 4,
                "third": enc(self.env.L, fb5, "rgba8", True), "third seq": 5, "third frames_done": 5, "dropped": 1}


class Noise(Scenario):
    """Noise tracking on, one report and one tile-map read as the warm-up.  `held` ("context" or "noise") is held, a frame and its
    query are queued: with the context's stream held the poll (mrt_noise_result, wait = 0) still gives the warm-up's report; the
    blocking tile-map read and the blocking report are noise_ref's for the oracle's three frames (noise.cpp, mrt_read_noise_tiles:
    the noise stream waits for the report's `copied`).  A dropped wait lets the map's copy run before the reduction: a copy of
    fixed size out of the ring entry's map, stale floats at worst."""

    def __init__(self, env, name, held):
        super().__init__(env, name)
        self.held = held
        if held == "context":
            self.misses = "hipStreamWaitEvent(c->noise_stream, c->noise_ring[c->noise_seq % kNoiseRing].copied, 0)"

    def configure(self, st):
        st.set_noise_tracking(True)

    def prepare(self):
        st = self.state()
        for _ in range(2):
            st.redraw()
        st.noise_query(NOISE_THRESHOLD, NOISE_FLOOR)
        if st.noise_result(wait=True) is None:
            raise Unexpected("the warm-up's query gave no report")
        st.read_noise_tiles()
        st.sync()
        return [st]

    def act(self, sts, clock):
        st = sts[0]
        clock.hold(st, self.held)
        st.redraw()
        st.noise_query(NOISE_THRESHOLD, NOISE_FLOOR)
        clock.mark()
        self.polled = st.noise_result(wait=False)

    def observe(self, sts, seen):
        st = sts[0]
        if self.held == "context":
            seen["polled seq"] = None if self.polled is None else self.polled["seq"]
        seen["tiles"] = st.read_noise_tiles()
        rep = st.noise_result(wait=True)
        if rep is None:
            return
        for k in ("seq", "frames_done", "pixels", "non_finite", "above"):
            seen[k] = int(rep[k])
        for k in ("noise_factor", "max_se", "sum_var", "sum_lum"):
            seen[k] = float(rep[k])

    def reference(self):
        means = self.env.frames([(self.old, self.cam)] * 3, means=True)
        fb, S, K = noise_ref.accumulate(means, [self.env.O.frame_weight(f, 1.0) for f in range(3)])
        rep = noise_ref.report(S, fb, K, NOISE_THRESHOLD, NOISE_FLOOR)
        out = {"tiles": noise_ref.tiles(S, fb, K, NOISE_THRESHOLD, NOISE_FLOOR), "seq": 2, "frames_done": 3, "pixels": rep["pixels"],
               "non_finite": rep["non_finite"], "above": rep["above"], "noise_factor": float(K), "max_se": float(rep["max_se"]),
               "sum_var": float(rep["sum_var"]), "sum_lum": float(rep["sum_lum"])}
        if self.held == "context":
            out["polled seq"] = 1
        return out


class Gather(Scenario):
    """Three shards of one image on one device, two frames each and one gather as the warm-up.  The stream of shard 0 (not the
    root) is held before its third frame; every shard redraws, the root gathers and reads: the full frame is the unsharded
    oracle's (multi_gpu.cpp: the root's stream waits for every shard's ev_gather).  A dropped wait lets the root read before a
    shard's bands have arrived: the copies are whole bands at fixed offsets of buffers that exist since the warm-up."""

    misses = "hipStreamWaitEvent(R->stream, ctxs[i]->ev_gather, 0)"

    def shards(self):
        sts = [self.state(shard=(r, WORLD)) for r in range(WORLD)]
        for _ in range(2):
            for st in sts:
                st.redraw()
        return sts

    def prepare(self):
        sts = self.shards()
        self.env.mrt.gather(sts, ROOT_RANK)
        sts[ROOT_RANK].read_gathered()
        for st in sts:
            st.sync()
        return sts

    def act(self, sts, clock):
        clock.hold(sts[0], "context")
        for st in sts:
            st.redraw()
        self.env.mrt.gather(sts, ROOT_RANK)

    def observe(self, sts, seen):
        seen["gathered"] = sts[ROOT_RANK].read_gathered()

    def reference(self):
        return {"gathered": self.env.frames([(self.old, self.cam)] * 3)[0]}


class GatherReader(Gather):
    """Gather's shards, and the root has presented the gathered frame once.  The root's stream is held and a present of the
    gathered frame -- a reader of the root's full frame -- queued behind the hold; every shard redraws and the root gathers again:
    the presented image is encode_host of the two-frame accumulation although the three-frame one has been gathered behind it
    (multi_gpu.cpp: every shard's stream waits for the root's ev_gather_root before its copies).  A dropped wait lets a shard's
    bands land before the reader has run: whole bands at fixed offsets, newer values."""

    misses = "hipStreamWaitEvent(c->stream, R->ev_gather_root, 0)"

    def prepare(self):
        sts = self.shards()
        self.env.mrt.gather(sts, ROOT_RANK)
        R = sts[ROOT_RANK]
        R.present(gathered=True)
        if R.acquire_presented(wait=True) is None:
            raise Unexpected("the warm-up's present gave no image")
        R.release_presented()
        for st in sts:
            st.sync()
        return sts

    def act(self, sts, clock):
        R = sts[ROOT_RANK]
        clock.hold(R, "context")
        R.present(gathered=True)
        for st in sts:
            st.redraw()
        self.env.mrt.gather(sts, ROOT_RANK)

    def observe(self, sts, seen):
        got = sts[ROOT_RANK].acquire_presented(newest=False, wait=True)
        seen["image"] = None if got is None else got[0]
        super().observe(sts, seen)

    def reference(self):
        fb2, _ = self.env.frames([(self.old, self.cam)] * 2)
        out = super().reference()
        out["image"] = present_ref.encode_host(self.env.L, fb2, "rgba8", True)
        return out


SCENARIOS = {
    "inputs/spheres": lambda e, n: InputsToRender(e, n, "spheres"),
    "inputs/materials": lambda e, n: InputsToRender(e, n, "materials"),
    "inputs/regroup": lambda e, n: InputsToRender(e, n, "regroup"),
    "inputs/auto-regroup": lambda e, n: InputsToRender(e, n, "auto"),
    "inputs/spheres-large": lambda e, n: InputsToRender(e, n, "spheres", "large"),
    "inputs/spheres-host-buffer": lambda e, n: InputsToRender(e, n, "spheres+garbage"),
    "inputs/materials-host-buffer": lambda e, n: InputsToRender(e, n, "materials+garbage"),
    "scatter/spheres": lambda e, n: RenderToScatter(e, n, "spheres"),
    "scatter/materials": lambda e, n: RenderToScatter(e, n, "materials"),
    "scatter/regroup": lambda e, n: RenderToScatter(e, n, "regroup"),
    "scatter/spheres-large": lambda e, n: RenderToScatter(e, n, "spheres", "large"),
    "blend": RenderToBlend,
    "slot-reuse": SlotReuse,
    "camera/lists": lambda e, n: CameraTables(e, n, 2),
    "camera/masks": lambda e, n: CameraTables(e, n, 3),
    "present/context": lambda e, n: Present(e, n, "context"),
    "present/present": lambda e, n: Present(e, n, "present"),
    "present/ring": PresentRing,
    "noise/context": lambda e, n: Noise(e, n, "context"),
    "noise/noise": lambda e, n: Noise(e, n, "noise"),
    "gather": Gather,
    "gather/reader": GatherReader,
}
# the children of tests/test_gpu_stream_order.py: one per group
GROUPS = {"frames": [n for n in SCENARIOS if n.split("/")[0] in ("inputs", "scatter", "blend", "slot-reuse")],
          "tables": [n for n in SCENARIOS if n.split("/")[0] in ("camera", "present", "noise")],
          "shards": [n for n in SCENARIOS if n.split("/")[0] == "gather"]}


def run_case(env, scenario, n_skip=0, ticks=None):
    """One case on fresh contexts: the scenario with the n_skip-th stream wait of its act dropped (0: none; without a shim the
    waits are not counted).  Returns the record: what differs from the reference, the queueing time, and with a shim the waits,
    the dropped wait's site and the sites seen."""
    rec = {"scenario": scenario.name, "n": n_skip, "misses": scenario.misses, "findings": []}
    ref = env.reference(scenario)
    shim = env.shim
    if shim:
        shim.L.mrt_fi_reset()
    sts = scenario.prepare()
    try:
        clock = Clock(ticks)
        if shim:
            shim.L.mrt_fi_skip_wait(n_skip)
        scenario.act(sts, clock)
        clock.mark()
        seen = {}
        scenario.observe(sts, seen)
        for st in sts:
            st.sync()
        if shim:                            # (the read-backs' waits count too: mrt_read_noise_tiles queues one)
            rec["waits"] = int(shim.L.mrt_fi_waits())
            rec["site"] = shim.skipped()
            shim.L.mrt_fi_skip_wait(0)
        rec["read_ms"] = round((time.perf_counter() - clock.t0) * 1e3, 3)       # (from the hold to the last read-back)
        start, end, _ = clock.held.debug_hold_stamps()
        rec["queue_ms"], rec["hold_ms"] = round(clock.queue_ms, 3), round((end - start) / 1e5, 3)
        if rec["queue_ms"] > 0.5 * clock.ticks / 1e5:
            rec["findings"].append(f"inconclusive: queueing took {rec['queue_ms']} ms, more than half the hold of {clock.ticks / 1e5} ms")
        if end - start < clock.ticks:
            rec["findings"].append(f"inconclusive: the hold ended after {end - start} of its {clock.ticks} ticks (its {HOLD_POLLS} polls came first)")
        rec["differs"] = differs(seen, ref)
        if shim:
            rec["wait_sites"] = shim.wait_sites()
            for v in shim.violations():
                rec["findings"].append("shim: " + v)
    finally:
        for st in sts:
            st.close()
    return rec


def walk(env, name, emit):
    """the clean case, and if it equals the reference N = 1 .. W, W being the stream waits the clean case counted"""
    scenario = SCENARIOS[name](env, name)
    clean = run_case(env, scenario, 0)
    clean["mode"] = "clean"
    if clean["differs"]:
        clean["findings"].append(f"with no wait dropped, {clean['differs']} differ from the reference")
    emit(clean)
    if clean["findings"]:
        return
    for n in range(1, clean["waits"] + 1):
        rec = run_case(env, scenario, n)
        rec["detected"] = bool(rec["differs"])
        if rec["site"] is None:
            rec["findings"].append(f"the {n}-th wait of {clean['waits']} was never reached")
        emit(rec)


class WaitShim:
    """the shim's stream-wait interface (tests/failinject/mrt_failinject.h) on a loaded library"""

    def __init__(self, L):
        import ctypes as C
        from failure_walks import Shim
        self.C, self.L, self._creators = C, L, Shim(L)
        for name, res, args in (("mrt_fi_skip_wait", None, [C.c_uint64]), ("mrt_fi_waits", C.c_uint64, []),
                                ("mrt_fi_skipped", C.c_int, [C.c_char_p, C.c_size_t]), ("mrt_fi_wait_sites", C.c_size_t, [C.c_char_p, C.c_size_t])):
            fn = getattr(L, name)           # AttributeError: not the failure-injecting build
            fn.restype, fn.argtypes = res, args

    def skipped(self):
        buf = self.C.create_string_buffer(256)
        return buf.value.decode() if self.L.mrt_fi_skipped(buf, len(buf)) else None

    def wait_sites(self):
        n = self.L.mrt_fi_wait_sites(None, 0)
        buf = self.C.create_string_buffer(n)
        self.L.mrt_fi_wait_sites(buf, n)
        return [s for s in buf.value.decode().split("\n") if s]

    def violations(self):
        return self._creators.violations()


def detected_sites(recs):
    """{the key of a stream-wait site (tests/failure_sites.py): the scenarios built to miss that wait in which dropping it was
    detected}"""
    from failure_sites import WAITS, key_of, source_sites
    src = source_sites(calls=WAITS)
    out = {}
    for r in recs:
        if r.get("detected") and r.get("site"):
            key = key_of(r["site"], src)
            if key is None:
                raise AssertionError(f"the sources have no stream wait at {r['site']}")
            if r.get("misses") and r["misses"] in key and r["scenario"] not in out.setdefault(key, []):
                out[key].append(r["scenario"])
    return out


def measure(env):
    """the figures behind HOLD_TICKS and HOLD_POLLS: every scenario once, and one hold that its polls alone end"""
    worst = (0.0, None)
    for name in SCENARIOS:
        rec = run_case(env, SCENARIOS[name](env, name), 0)
        # ... and with a hold of one tick: the host's queueing, all the work on the device and the read-backs, end to end
        free = run_case(env, SCENARIOS[name](env, name), 0, ticks=1)
        print(json.dumps(dict({k: rec[k] for k in ("scenario", "queue_ms", "hold_ms", "differs", "findings")}, unheld_ms=free["read_ms"])))
        worst = max(worst, (free["read_ms"], name))
    sc = RenderToBlend(env, "blend")
    st = sc.prepare()[0]
    polls = 4096
    st.debug_hold("context", 0, 50_000_000, polls)
    st.sync()
    start, end, given = st.debug_hold_stamps()
    st.close()
    print(json.dumps({"longest unheld ms": worst[0], "in": worst[1], "polls": given, "ticks": end - start,
                      "polls per ms": given / ((end - start) / 1e5)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenarios", default="all", help="names of SCENARIOS or GROUPS, comma-separated, or all")
    ap.add_argument("--log")
    ap.add_argument("--record", help="write the detected sites to this file (tests/golden/order_sites.json)")
    ap.add_argument("--measure", action="store_true", help="product library: print every scenario's queueing time and the polls per ms")
    a = ap.parse_args()
    names = []
    for n in (list(SCENARIOS) if a.scenarios == "all" else a.scenarios.split(",")):
        names += [n] if n in SCENARIOS else GROUPS.get(n, [n])
    unknown = [n for n in names if n not in SCENARIOS]
    if unknown:
        ap.error(f"unknown scenarios {unknown}")
    import myraytracer_amd as mrt
    from myraytracer_amd import _lib
    from oracle import pyoracle
    pyoracle.lib()
    if a.measure:
        measure(Env(mrt, pyoracle))
        return 0
    if not a.log:
        ap.error("--log FILE")
    recs = []

    def body(emit):
        env = Env(mrt, pyoracle, WaitShim(_lib.load()))

        def keep(rec):
            recs.append(rec)
            emit(rec)
        for name in names:
            walk(env, name, keep)
    code = logged_main(a.log, body)
    if a.record and code == 0:
        with open(a.record, "w") as f:
            json.dump({"sites": detected_sites(recs)}, f, indent=1, sort_keys=True)
            f.write("\n")
    return code


if __name__ == "__main__":
    sys.exit(main())
