"""Random call sequences on one context, checked in lock step against tests/state_model.py.

sequence(case) draws the image size, the creation arguments and a whole list of ops from np.random.default_rng(case) in a
fixed order: a case number reproduces its sequence anywhere.  Ops are plain tuples, ("render", 3), ("set_world", 1021, 1), ...;
run(case, impl, model) applies each to both and compares what that op makes observable, bit for bit (the doubles of a noise
report at rel 1e-12, as tests/test_gpu_adaptive.py holds them).

The generator keeps sequences legal to compare.  It follows a small shadow of the state to know what is defined:
  - the calls whose result depends on what has finished -- noise_result(wait=False), render_adaptive(k, 0), a NEWEST acquire
    with more than one image queued (it takes the newest finished one and waits only if none has) -- directly follow a sync;
    the other acquires wait;
  - at most three presented images are outstanding (queued or held): the smallest automatic ring has three entries (one frame
    in flight + 2), and which image a fuller ring drops depends on the schedule;
  - refusals are drawn one reason at a time, so the status does not depend on the order the library checks in;
  - geometry and cameras stay far inside the limits mrt_set_world_raw and mrt_set_camera enforce.
Scheduling is never compared."""
import numpy as np
import pytest

import myraytracer_amd as M
import noise_ref
from common import mismatch_report
from state_model import COUNTER_KEYS, OK, Refused

# 993 / 994: the last small-layout and the first large-layout scene of make_scene's streams.  world.cpp takes the large layout
# when the hierarchy's n_members > 1024, and n_members is the clusters' member slots, padded to 32, plus 4 where the scene has
# spheres too large to cluster (here: the ground) -- 992 + 4 against 1024 + 4.  (tests/test_state_model.py checks it.)
SPHERE_COUNTS = (0, 1, 17, 300, 993, 994, 2500)
SMALL_MAX = 993
SUITE_CASES = tuple(range(20))
HINTS = [(0, 0)] + [(d, m) for d in range(1, 9) for m in range(1, 9) if max(2, d) * m <= 16]
REPORT_REL = 1e-12
VOCABULARY = ("redraw", "render", "render_tiles", "render_adaptive", "sync", "set_camera", "set_samples_per_frame", "set_rng_mode",
              "set_rng_shuffle", "set_schedule_hint", "debug_set_frames_in_flight", "debug_set_frame_batching", "set_world",
              "set_seeds", "reset", "set_shard", "set_noise_tracking", "read_framebuffer", "read_noise", "tile_frames",
              "read_counters", "frames_done", "locals", "read_seeds", "noise_query", "noise_result", "read_noise_tiles", "present",
              "acquire_presented", "release_presented", "read_denoised", "debug_read_guides")


# ------------------------------------------------------------------ inputs an op names

def make_scene(n: int, scene_seed: int) -> np.ndarray:
    """The first n spheres of stream `scene_seed`: in front of both kinds of camera, mixed materials, radii shrinking with n so
    that sky stays visible.  Sphere 0 is the ground whenever there are two or more."""
    rng = np.random.default_rng(77000 + scene_seed)
    N = max(SPHERE_COUNTS)
    sc = np.zeros(N, M.SPHERE_DTYPE)
    r = (0.9 / max(n, 1) ** (1 / 3)) * rng.uniform(0.6, 1.6, N)
    sc["center"] = np.stack([rng.uniform(-3, 3, N), rng.uniform(-1.5, 2.5, N), rng.uniform(-8, -1.5, N)], 1)
    sc["radius"] = np.where(rng.random(N) < 0.03, -r, r)                       # (a few hollow ones)
    ty = rng.choice([1, 1, 1, 2, 2, 3], N)
    sc["material_ty"] = ty
    sc["albedo"] = rng.uniform(0.1, 1.0, (N, 3))
    sc["param"] = np.where(ty == 2, rng.uniform(0, 0.8, N), 1.5)
    if n >= 2:
        sc[0] = ((0.0, -101.5, -4.0), 100.0, 1, (0.5, 0.55, 0.4), 0.0)        # the ground
    return sc[:n].copy()


def make_seeds(seed_seed: int, w: int, h: int) -> np.ndarray:
    return np.random.default_rng(seed_seed).integers(0, 2 ** 32, (h, w, 4), dtype=np.uint64).astype(np.uint32)


def make_camera(cam):
    return M.Camera(*cam)


def _draw_camera(rng):
    if rng.random() < 0.25:
        return (0, (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 90.0, 0.0, 1.0)
    r = lambda lo, hi: round(float(rng.uniform(lo, hi)), 3)
    return (1, (r(-2, 2), r(0, 2), r(0.5, 3)), (r(-1, 1), r(-0.5, 0.5), r(-5, -3)), (round(0.1 * float(rng.normal()), 3), 1.0, 0.0),
            r(30, 90), float(rng.choice([0.0, 0.0, 0.6, 2.0])), r(2, 6))


def _draw_size(rng):
    kind = rng.choice(["ragged", "ragged", "ragged", "one tile wide", "one row high", "large"])
    odd = lambda lo, hi: int(rng.choice([v for v in range(lo, hi) if v % 8]))
    if kind == "one tile wide":
        return odd(1, 8), odd(9, 50)
    if kind == "one row high":
        return odd(9, 90), 1
    if kind == "large":
        return odd(90, 103), odd(52, 62)
    return odd(9, 64), odd(9, 46)


# ------------------------------------------------------------------ the generator

def sequence(case: int):
    """-> (params, ops): params = dict(width, height, spp, depth, max_w, seed); ops = the case's list of tuples."""
    rng = np.random.default_rng(case)
    w, h = _draw_size(rng)
    p = dict(width=w, height=h, spp=int(rng.choice([1, 2, 3])), depth=int(rng.choice([1, 3, 8, 13])),
             max_w=float(rng.choice([1.0, 0.75])), seed=int(rng.integers(0, 2 ** 62)))
    tx, tr = -(-w // 8), -(-h // 8)
    n_tiles = tx * tr
    g = dict(world=False, n=0, frames=0, tracking=False, shards=1, diverged=False, mode=0, spp=p["spp"], queued=0, held=False,
             presented=False, nseq=0, nfirst=1, quiet=True, budget=float(rng.choice([0.6, 1.0, 1.4])) * 4e7, shuffled=False)
    if case % 8 == 7:              # a long case: frames heavy enough to be in flight still when the next call arrives
        g["budget"] *= 6
        w, h = p["width"], p["height"] = 90 + w % 13 + (w % 13 == 6), 52 + h % 9 + (h % 9 == 4)      # (neither a multiple of 8)
        p["depth"], p["spp"], g["spp"] = 13, 3, 3
        tx, tr = -(-w // 8), -(-h // 8)
        n_tiles = tx * tr
    ops = []
    chance = lambda q: bool(rng.random() < q)

    def frame_cost(pixels):
        return pixels * max(g["spp"], 1) * min(p["depth"], 6) * (40 + g["n"]) / 60

    def frames_ok(k, pixels=w * h):
        c = k * frame_cost(pixels // g["shards"] + 1)
        if c > g["budget"]:
            return False
        g["budget"] -= c
        return True

    def emit(*op):
        ops.append(op)

    def some_tiles():
        n = int(rng.integers(1, max(2, n_tiles)))
        return tuple(int(t) for t in np.sort(rng.choice(n_tiles, min(n, n_tiles), replace=False)))

    def framed(k, subset=False):
        g["frames"] += k
        g["quiet"] = g["shuffled"] = False
        if subset:
            g["diverged"] = True

    def observe():
        kind = rng.choice(["read_framebuffer", "read_framebuffer", "read_noise", "tile_frames", "read_counters", "frames_done", "locals",
                           "read_seeds", "noise", "noise", "present", "present", "read_denoised", "debug_read_guides"])
        if kind == "noise":
            if not g["tracking"]:
                return emit(str(rng.choice(["read_noise", "read_noise_tiles"])))      # refused: tracking is off
            burst = 10 if chance(0.12) else 1                          # (more than the ring of eight without reading)
            for _ in range(burst):
                emit("noise_query", float(rng.choice([0.02, 0.1, 0.3, 1.0])), float(rng.choice([0.01, 0.05])))
                g["nseq"] += 1
            g["quiet"] = False
            if chance(0.8):
                emit("noise_result", True)
            if chance(0.5):
                emit("read_noise_tiles")
            return
        if kind == "present":
            want_denoise = chance(0.3)
            flip = chance(0.5) if g["shards"] == 1 or chance(0.1) else False    # (a shard's flip is refused: rarely)
            for _ in range(int(rng.choice([1, 1, 2, 3]))):
                if g["queued"] + g["held"] > 2:
                    break
                emit("present", str(rng.choice(["rgba8", "bgra8"])), flip, want_denoise)
                refused = (want_denoise and (not g["tracking"] or g["shards"] > 1 or not g["world"] or g["diverged"])) or \
                          (not want_denoise and g["shards"] > 1 and flip)
                if not refused:                                         # (diverged unknown: counted as queued, the safe side)
                    g["queued"] += 1
                    g["presented"] = True
                    g["quiet"] = False
            if g["presented"] and chance(0.85):
                newest = chance(0.5)
                if newest and g["queued"] > 1:
                    emit("sync")                                        # (newest = the newest FINISHED: defined once all have)
                emit("acquire_presented", newest)
                if g["queued"]:
                    g["queued"] = 0 if newest else g["queued"] - 1
                    g["held"] = True
                else:
                    g["held"] = False
                if chance(0.6):
                    emit("release_presented")
                    g["held"] = False
            return
        emit(str(kind))

    refused_so_far = set()

    def refusal():
        """One call the header refuses in this state (or nothing, if none applies)."""
        kinds = []
        if g["frames"] > 0:
            kinds += ["tracking", "shard"]
        if g["diverged"] is True and g["tracking"] and g["world"] and g["shards"] == 1:
            kinds += ["denoise", "present-denoise"]
        if g["shards"] > 1 and g["world"]:
            kinds += ["tiles-on-shard", "denoise"]
        if g["tracking"] and g["nseq"] >= 9:
            kinds += ["old-report", "old-report"]
        if g["tracking"]:
            kinds += ["future-report"]
        if g["mode"] == 1 and g["spp"] > 64 and g["world"] and g["shards"] == 1:
            kinds += ["counter-tiles"]
        if g["world"] and g["shards"] == 1 and not (g["mode"] == 1 and g["spp"] > 64):
            kinds += ["bad-tile", "twice"]
        if not g["held"]:
            kinds += ["release"]
        if not kinds:
            return
        fresh = sorted(set(kinds) - refused_so_far)                    # (a kind this case has not had yet comes first)
        k = str(rng.choice(fresh or kinds))
        refused_so_far.add(k)
        if k == "tracking":
            emit("set_noise_tracking", not g["tracking"])
        elif k == "shard":
            emit("set_shard", 1, 2)
        elif k == "denoise":
            emit("read_denoised")
        elif k == "present-denoise":
            emit("present", "rgba8", True, True)
        elif k == "tiles-on-shard":
            emit("render_tiles", (0,), 1)
        elif k == "old-report":
            emit("render_adaptive", 1, g["nseq"] - 8)
        elif k == "future-report":
            emit("render_adaptive", 1, g["nseq"] + 2)
        elif k == "counter-tiles":
            emit("render_tiles", (0,), 1)
        elif k == "bad-tile":
            emit("render_tiles", (0, n_tiles), 1)
        elif k == "twice":
            emit("render_tiles", (0, 0), 1)
        elif k == "release":
            emit("release_presented")

    # before a scene: what is refused for the lack of one
    if chance(0.7):
        emit("set_noise_tracking", True)
        g["tracking"] = True
    if chance(0.5):
        emit(*[("redraw",), ("render", 2), ("render_tiles", (0,), 1), ("read_denoised",), ("debug_read_guides",)][int(rng.integers(0, 5))])
    if chance(0.2):
        emit("acquire_presented", True)                                # refused: nothing presented yet

    def set_world():
        if g["n"] <= SMALL_MAX and g["world"]:
            pool = [994, 994, 2500, 0, 1, 17, 300, 993]
        else:
            pool = [993, 993, 300, 17, 17, 1, 0, 994, 2500]
        n = int(rng.choice(pool)) if g["world"] else int(rng.choice(SPHERE_COUNTS))
        emit("set_world", n, int(rng.integers(0, 2)))
        g["world"], g["n"] = True, n

    set_world()
    if chance(0.6):
        emit("set_camera", _draw_camera(rng))

    for _ in range(int(rng.integers(26, 40))):
        u = rng.random()
        if u < 0.30:                                                    # frames
            kind = rng.choice(["redraw", "render", "render", "render_tiles", "render_tiles", "render_adaptive", "sync"])
            if kind == "redraw" and frames_ok(1):
                emit("redraw")
                framed(1)
            elif kind == "render":
                k = int(rng.choice([1, 2, 3, 5, 8, 12, int(rng.integers(33, 41))]))
                if g["shuffled"]:
                    k = max(k, 2)
                if frames_ok(k):
                    emit("render", k)
                    framed(k)
            elif kind == "render_tiles" and g["shards"] == 1 and n_tiles > 1 and not (g["mode"] == 1 and g["spp"] > 64):
                tiles = tuple(range(n_tiles)) if chance(0.12) else some_tiles()
                if chance(0.1):
                    tiles = ()
                k = int(rng.choice([1, 1, 2, 3, 5]))
                if frames_ok(k, 64 * len(tiles)):
                    emit("render_tiles", tiles, k)
                    if tiles:
                        framed(k, subset=len(tiles) < n_tiles)
                    if g["tracking"] and chance(0.4):
                        emit("read_noise")
            elif kind == "render_adaptive" and g["tracking"] and g["shards"] == 1 and g["frames"] > 0 and not (g["mode"] == 1 and g["spp"] > 64):
                k = int(rng.choice([1, 2, 3]))
                if not frames_ok(k):
                    continue
                live = [s for s in range(max(g["nfirst"], g["nseq"] - 7, 1), g["nseq"] + 1)]
                if live and chance(0.7):
                    emit("render_adaptive", k, int(rng.choice(live)))
                else:
                    emit("sync")
                    emit("render_adaptive", k, 0)
                g["quiet"] = g["shuffled"] = False
                g["diverged"] = None if g["diverged"] is not True else True      # (depends on the selection)
            else:
                emit("sync")
                g["quiet"] = True
                if g["tracking"] and chance(0.4):
                    emit("noise_result", False)
        elif u < 0.50:                                                  # between frames, no wait
            kind = rng.choice(["set_camera", "set_camera", "spp", "spp", "spp", "mode", "mode", "shuffle", "shuffle", "hint", "in_flight", "batching"])
            if kind == "set_camera":
                emit("set_camera", _draw_camera(rng))
                if chance(0.5):
                    emit(str(rng.choice(["debug_read_guides", "debug_read_guides", "read_denoised"])))
            elif kind == "spp":
                big = g["mode"] == 1 and w * h <= 1500 and g["n"] <= SMALL_MAX
                g["spp"] = int(rng.choice([64, 65, 130] if big and chance(0.6) else [0, 1, 1, 2, 2, 3, 5]))
                if g["spp"] <= 5 and chance(0.25):
                    g["spp"] = (0, 5)[(case + len(ops)) % 2]
                emit("set_samples_per_frame", g["spp"])
                if chance(0.4) and frames_ok(1):
                    emit("redraw")
                    framed(1)
            elif kind == "mode":
                g["mode"] ^= 1
                emit("set_rng_mode", g["mode"])
                if g["mode"] == 1 and w * h <= 1500 and g["n"] <= SMALL_MAX and chance(0.6):
                    g["spp"] = (64, 65, 130)[(case + len(ops)) % 3]         # a block, a block and one, three blocks
                    emit("set_samples_per_frame", g["spp"])
                    if frames_ok(1):
                        emit("redraw")
                        framed(1)
                if g["mode"] == 0 and g["spp"] > 5:
                    g["spp"] = int(rng.choice([1, 2, 3]))
                    emit("set_samples_per_frame", g["spp"])
            elif kind == "shuffle":
                s = tuple(int(x) for x in rng.integers(0, 2 ** 32, 4))
                emit("set_rng_shuffle", s)
                if chance(0.3):
                    emit("set_rng_shuffle", s)                          # the same one twice
                g["shuffled"] = True
                if chance(0.7) and frames_ok(3):
                    k = int(rng.choice([2, 3]))
                    emit("render", k)
                    framed(k)
            elif kind == "hint":
                emit("set_schedule_hint", *HINTS[0 if chance(0.2) else int(rng.integers(0, len(HINTS)))])
            elif kind == "in_flight":
                emit("debug_set_frames_in_flight", int(rng.choice([0, 1, 2, 3, 4, 8])))
            else:
                emit("debug_set_frame_batching", int(rng.choice([0, 1, 2, 3])))
        elif u < 0.61:                                                  # between frames, waits
            kind = rng.choice(["set_world", "set_world", "set_world", "set_seeds", "reset", "reset", "reset"])
            if kind == "set_world":
                set_world()
            elif kind == "set_seeds":
                emit("set_seeds", int(rng.integers(0, 1000)))
            else:
                was_diverged = g["diverged"]
                if g["world"] and chance(0.4) and frames_ok(1):             # (both parities of the ping-pong buffers meet a reset)
                    emit("redraw")
                    framed(1)
                emit("reset")
                g.update(frames=0, diverged=False, queued=0, held=False, nfirst=g["nseq"] + 1, shuffled=False)
                if chance(0.65):                                        # what a reset must have cleared, before a frame hides it
                    emit(str(rng.choice(["read_framebuffer", "read_framebuffer", "read_framebuffer", "tile_frames", "read_counters", "locals"])))
                    if g["tracking"] and chance(0.5):
                        emit("read_noise")
                if chance(0.2):
                    g["tracking"] = not g["tracking"]
                    emit("set_noise_tracking", g["tracking"])
                    g["nfirst"] = g["nseq"] + 1
                if chance(0.3):
                    world = int(rng.choice([1, 2, 3, 5, 8]))
                    emit("set_shard", int(rng.integers(0, world)), world)
                    g["shards"] = world
                    if g["tracking"]:
                        g["nfirst"] = g["nseq"] + 1
                if was_diverged and chance(0.6):
                    set_world()
        elif u < 0.68:
            refusal()
        else:
            observe()
    emit("sync")
    for o in ("frames_done", "locals", "read_counters", "tile_frames", "read_framebuffer"):
        emit(o)
    if g["tracking"]:
        emit("read_noise")
    return p, ops


# ------------------------------------------------------------------ applying and comparing

def apply(obj, op):
    """Calls op on a State or a Model -> (status, value)."""
    name, a = op[0], op[1:]
    try:
        if name == "set_world":
            return OK, obj.set_world(make_scene(a[0], a[1]))
        if name == "set_camera":
            return OK, obj.set_camera(make_camera(a[0]))
        if name == "set_seeds":
            return OK, obj.set_seeds(make_seeds(a[0], obj.shard_info()[3], _height(obj)))
        if name in ("frames_done", "locals"):
            return OK, getattr(obj, name)
        if name == "present":
            return OK, obj.present(a[0], flip=a[1], denoise=a[2])
        if name == "acquire_presented":
            return OK, obj.acquire_presented(newest=a[0], wait=True)
        if name == "noise_result":
            return OK, obj.noise_result(wait=a[0])
        return OK, getattr(obj, name)(*a)
    except (Refused, M.MrtError) as e:
        return e.status, None


def _height(obj):
    return obj.h if hasattr(obj, "h") else obj.args.height


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:                  # bit for bit; a NaN equals a NaN (as scripts/parity_campaign.py has it)
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def _describe(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape / type {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    if a.dtype == np.float32 and a.ndim == 3:
        return mismatch_report(a, b)
    neq = np.argwhere(a != b)
    return f"{len(neq)} of {a.size} differ; first at {tuple(neq[0])}: {a[tuple(neq[0])]!r} against {b[tuple(neq[0])]!r}"


def _locals_tuple(L):
    return (tuple(L.shape), int(L.samples_per_frame), int(L.ray_depth), tuple(int(x) for x in L.rng_shuffle),
            np.float32(L.framebuffer_weight).view(np.uint32).item(), int(L.rng_mode))


def compare(op, got, want, shard_valid=None):
    """None if `got` (impl) equals `want` (model) for this op, else what differs."""
    name = op[0]
    if got is None or want is None:
        return None if got is None and want is None else f"{got!r} against {want!r}"
    if name in ("read_framebuffer", "read_noise", "tile_frames", "read_noise_tiles", "read_denoised"):
        return None if _same(got, want) else _describe(got, want)
    if name == "read_seeds":
        v = shard_valid
        return None if _same(got[v], want[v]) else _describe(got[v], want[v])
    if name == "debug_read_guides":
        for k in ("rays", "index", "t", "normal", "albedo"):
            if not _same(got[k], want[k]):
                return f"guide {k}: " + _describe(got[k], want[k])
        return None
    if name == "read_counters":
        bad = [f"{k} {got[k]} against {want[k]}" for k in COUNTER_KEYS if got[k] != want[k]]
        return ", ".join(bad) or None
    if name == "frames_done":
        return None if got == want else f"{got} against {want}"
    if name == "locals":
        g, w = _locals_tuple(got), _locals_tuple(want)
        return None if g == w else f"{g} against {w}"
    if name == "render_adaptive":
        return None if tuple(got) == tuple(want) else f"(report used, tiles selected) {tuple(got)} against {tuple(want)}"
    if name == "noise_result":
        for k in ("seq", "frames_done", "pixels", "non_finite", "above", "threshold", "floor", "noise_factor", "max_se", "sum_lum", "sum_var",
                  "rmse", "rel_rmse"):
            exact = k not in ("sum_lum", "sum_var", "rmse", "rel_rmse")
            if not (got[k] == want[k] if exact else got[k] == pytest.approx(want[k], rel=REPORT_REL, abs=0.0)):
                return f"report field {k}: {got[k]!r} against {want[k]!r}"
        return None
    if name == "acquire_presented":
        for k in ("seq", "frames_done", "width", "rows", "row_bytes", "format", "flags", "dropped"):      # (ring_depth: the schedule's)
            if got[1][k] != want[1][k]:
                return f"present info {k}: {got[1][k]} against {want[1][k]}"
        return None if _same(got[0], want[0]) else "presented bytes: " + _describe(got[0], want[0])
    return None


class SequenceMismatch(AssertionError):
    pass


class SequenceStopped(RuntimeError):
    """A status that is no comparison failure (a stalled wait, a HIP error): the case, and a campaign, end here."""


def run_ops(label, ops, impl, model, stats=None, after=None):
    """after(i, op, status, impl): called behind every op that compared equal (the GPU test reads launch diagnostics there)."""
    for i, op in enumerate(ops):
        st_i, got = apply(impl, op)
        st_m, want = apply(model, op)
        where = f"{label}, op {i} {op!r}"
        if st_i in (3, 9):
            raise SequenceStopped(f"{where}: status {st_i}: {_last_error(impl)}\nops so far: {ops[:i + 1]!r}")
        bad = None
        if st_i != st_m:
            bad = f"status {st_i} against the model's {st_m} ({_last_error(impl)})"
        elif st_i == OK:
            r, wld, rows, _ = model.shard_info()
            bad = compare(op, got, want, noise_ref.shard_rows(_height(model), r, wld) >= 0)
        if bad:
            raise SequenceMismatch(f"{where}: {bad}\nops so far: {ops[:i + 1]!r}")
        if after is not None:
            after(i, op, st_i, impl)
        if stats is not None:
            stats["ops"] = stats.get("ops", 0) + 1
            stats.setdefault("statuses", set()).add((op[0], st_m))
    if stats is not None:
        stats["frames"] = stats.get("frames", 0) + model.frames_total


def _last_error(impl):
    try:
        return impl._L.mrt_last_error(impl._ctx).decode()
    except Exception:
        return ""


def check_context(label, impl):
    """mrt_debug_check_context on a real State (host only): nothing a later call would touch is missing."""
    L, ctx = getattr(impl, "_L", None), getattr(impl, "_ctx", None)
    if L is None or not ctx or not hasattr(L, "mrt_debug_check_context"):
        return          # (a model in the State's place: tests/test_state_model.py)
    import ctypes
    why = ctypes.create_string_buffer(512)
    if L.mrt_debug_check_context(ctx, why, len(why)) != 0:
        raise SequenceMismatch(f"{label}: the context is not sound after its sequence: {why.value.decode()}")


def run(case, impl, model, stats=None, after=None):
    """Applies case `case` to impl and model in lock step; raises SequenceMismatch at the first difference -- or if the
    context is not sound after the last op."""
    run_ops(f"case {case}", sequence(case)[1], impl, model, stats, after)
    check_context(f"case {case}", impl)


def new_model(O, params, cls=None):
    from state_model import Model
    args = M.Args(params["width"], params["height"], params["spp"], params["depth"], params["max_w"])
    return (cls or Model)(O, M._lib.load(), args, params["seed"])


def new_state(params):
    return M.State(M.Args(params["width"], params["height"], params["spp"], params["depth"], params["max_w"]), seed=params["seed"])
