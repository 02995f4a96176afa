"""Chains that put the adaptive accumulation on a scene that changes: subset frames (mrt_render_tiles, mrt_render_adaptive,
mrt_render_budget), the per-tile blend, noise reports of both map kinds, the per-tile denoise and its blend, next to
mrt_update_spheres, mrt_regroup_spheres, mrt_set_auto_regroup, mrt_update_materials, mrt_set_camera, mrt_set_world, mrt_reset and
mrt_temporal_step, up to forty ops each, checked against a host model.

The runner is motion_chains' own (Run, CameraTables, ChainStopped, ChainMismatch, new_state), through the hooks it has for this
module: an image size per chain (params["size"]), a Shadow of the caller's, a compare(name, got, want) behind every call both sides
accepted, an extra_check in every check, and render launches that name their tile list.  The chains are written out (CHAINS); a
name reproduces its ops anywhere.  On top of motion_chains' and material_chains' ops:

  ("tracking", on)                          mrt_set_noise_tracking
  ("subset", tiles, k)                      mrt_render_tiles(tiles, k)
  ("query", threshold, floor, kind)         mrt_noise_query / _map; kind "max_rel" | "sum_s"
  ("adaptive", frames, seq)                 mrt_render_adaptive(frames, seq): always a named report (0 depends on what has finished)
  ("budget", budget, max_frames, seq)       mrt_render_budget(budget, max_frames, seq)
  ("denoise_adaptive", on) ("denoise_variance", mode, spatial_frames) ("denoise_mix", on, gain)
  ("read_denoised",) ("read_temporal",)     compared where they stand (a check compares them again)
  ("present", "denoised" | "temporal")      mrt_present(rgba8, flip) of that source and an OLDEST acquire that waits
  ("auto_regroup", on, ratio, check_every)  mrt_set_auto_regroup
  ("spp", n) ("rng_mode", m)                mrt_set_samples_per_frame, mrt_set_rng_mode
  ("refuse", kind[, seq])                   one call the header refuses, REFUSALS; the next check shows that nothing changed

The model (Model) is material_chains.Model -- motion_chains.Model with mrt_update_materials -- with the accumulation replaced by
adaptive_ref.Accum, in the pattern of tests/state_model.py: a frame is its scene (spheres and materials), derived camera, tile
list or None and shuffle; the oracle renders the frame's rectangles with them and Accum.frame blends the means, so that fb, S and
n_t follow the header's recursion.  Reports are Accum.report / Accum.tiles and budget_ref.tile_sums, numbered in a ring of 8 as
state_model.py numbers them; selections adaptive_ref.select; allocations budget_ref.allocate / levels; the denoise
denoise_tiles_ref / denoise_mix_ref's per-tile forms after divergence and denoise_var_ref / denoise_mix_ref's uniform ones before,
through the model's guides with motion_chains' staleness rule; the temporal step and image read the per-tile framebuffer.  It
follows the header, not the code, and reads nothing back from the library (K is adaptive_ref.k_table's).

A check compares what motion_chains.Run.check compares and, bit for bit as uint32 views, tile_frames, read_noise, the newest
report (its doubles at state_sequences.REPORT_REL) and its tile map, and read_denoised where it is legal; a render_budget's doubles
are compared bit for bit where the call stands, as tests/test_gpu_adaptive_budget.py compares them."""
import numpy as np

import adaptive_ref
import budget_ref
import denoise_mix_ref
import denoise_tiles_ref
import denoise_var_ref
import material_chains as XC
import motion_chains as MC
import myraytracer_amd as M
import state_sequences as SS
from common import to_oracle_spheres
from present_ref import encode_host

OK, INVALID_ARG, NO_SCENE, STATE = MC.OK, MC.INVALID_ARG, MC.NO_SCENE, MC.STATE
KEYS = MC.KEYS
COUNTER_BLOCK, NOISE_RING = 64, 8
FLIP_Y, DENOISED, TEMPORAL = 1, 8, 16
K_TABLE_FIRST = 4096                            # noise.cpp, ensure_k_table: the device's table of K(n) begins here and doubles
REFUSALS = ("denoise-off", "adaptive-on-sums", "budget-on-max-rel", "old-report", "duplicate-tile", "counter-65")
VOCABULARY = ("tracking", "subset", "query", "adaptive", "budget", "denoise_adaptive", "denoise_variance", "denoise_mix", "read_denoised",
              "read_temporal", "present", "auto_regroup", "spp", "rng_mode", "refuse", "materials")
SMALL_IMAGE, WIDE_IMAGE = (20, 12), (44, 20)    # 3 x 2 and 6 x 3 tiles, both with a ragged right column and top band


class Shadow(XC.Shadow):
    def calls(self, op):
        name, a = op[0], op[1:]
        if name == "subset":
            return [("render_tiles", (a[0], a[1]))]
        if name == "present":
            return [("present", ("rgba8", True, False, a[0] == "denoised", a[0] == "temporal")), ("acquire_presented", (False, True))]
        if name == "refuse":
            kind = a[0]
            return [{"denoise-off": ("read_denoised", ()), "duplicate-tile": ("render_tiles", ((0, 2, 0), 1)),
                     "counter-65": ("render_tiles", ((0,), 1)), "adaptive-on-sums": ("render_adaptive", (1,) + a[1:]),
                     "old-report": ("render_adaptive", (1,) + a[1:]), "budget-on-max-rel": ("render_budget", (6, 2) + a[1:])}[kind]]
        simple = {"tracking": "set_noise_tracking", "query": "noise_query", "adaptive": "render_adaptive", "budget": "render_budget",
                  "denoise_adaptive": "set_denoise_adaptive", "denoise_variance": "set_denoise_variance", "denoise_mix": "set_denoise_mix",
                  "read_denoised": "read_denoised", "read_temporal": "read_temporal", "auto_regroup": "set_auto_regroup",
                  "spp": "set_samples_per_frame", "rng_mode": "set_rng_mode"}
        if name in simple:
            return [(simple[name], a)]
        return super().calls(op)


# ------------------------------------------------------------------ the model

_RECTS = {}                                     # oracle means of a rectangle: pure functions of their inputs, shared by every model


class Model(XC.Model):
    """material_chains.Model over adaptive_ref.Accum.  What the seeded defects of tests/test_adaptive_chains_host.py override:
    _frame_inputs, _blend, _counted, _guides_for, _denoise_counts, _sum_map, _budget_report, reset."""

    def __init__(self, O, max_w, w=MC.W, h=MC.H):
        super().__init__(O, max_w, w, h)
        self.L = M._lib.load()                  # (host only: mrt_srgb8 for present_ref)
        self.spp, self.rng_mode = MC.SPP, 0
        self.acc = adaptive_ref.Accum(h, w, max_w)
        self.counters = dict.fromkeys(KEYS, 0)
        self.tracking = False
        self.noise_seq, self.noise_first, self.reports = 0, 1, {}
        self.denoise_adaptive_on, self.var_mode, self.spatial_frames = False, 0, 3
        self.mix_on, self.mix_gain = False, M.denoise_mix_default()["gain"]
        self.present_seq, self.queue, self.held, self.dropped = 0, [], False, 0
        self.last_levels = []                   # the (tiles listed, run length) of the latest render_budget's render_tiles calls
        self.seeds_key = MC._key(self.seeds)
        self._packed = (None, None, None)
        self.selections, self.allocations, self.denoises = [], [], []      # statistics for the host tests' conditions
        self.k_consumers = []                   # (consumer, largest n_t) of every call that needs the device's table of K(n)

    # ---- what the seeded defects change
    def _frame_inputs(self, tiles):
        """(spheres, derived camera, its key) a frame over `tiles` (None: a whole frame) is rendered with"""
        return self.spheres, self.cam_raw, self.cam_key

    def _blend(self, mean, tiles):
        self.acc.frame(mean, tiles)

    def _counted(self, tiles, frames):
        """behind the `frames` subset frames of one mrt_render_tiles call"""

    def _guides_for(self, consumer):
        """the guides, rebuilt first if stale; consumer: "denoise", "denoise-tiles", "step", "read" """
        return self._ensure_guides()

    def _denoise_counts(self):
        return self.acc.tile_frames()

    def _sum_map(self):
        return budget_ref.tile_sums(self.acc.S, self.acc.fb)

    def _budget_report(self, seq):
        return self.reports[seq]

    # ---- frames
    @property
    def n_tiles(self):
        return self.acc.n_tiles

    @property
    def frames_done(self):
        return self.acc.frames_done

    def _rects(self, tiles):
        if tiles is None:
            return [(0, self.w, 0, self.h)]
        tx = self.acc.tx
        return [((t % tx) * 8, min((t % tx) * 8 + 8, self.w), (t // tx) * 8, min((t // tx) * 8 + 8, self.h)) for t in tiles]

    def _render(self, spheres, cam_raw, cam_key, shuffle, rect):
        if self._packed[0] is not spheres:      # (the model never writes a sphere list in place: identity names the scene)
            self._packed = (spheres, self.O.pack_world(to_oracle_spheres(self.O, spheres)), MC._key(spheres))
        _, packed, scene_key = self._packed
        k = (scene_key, cam_key, self.seeds_key, self.w, self.h, self.spp, self.rng_mode, shuffle, rect)
        if k not in _RECTS:
            if len(_RECTS) > 40000:
                _RECTS.clear()
            cnt = self.O.Counters()
            x0, x1, y0, y1 = rect
            img = self.O.render_frame(self.w, self.h, self.spp, MC.DEPTH, packed, cam_raw, self.seeds, shuffle, 0.0, rows=(y0, y1),
                                      cols=(x0, x1), counters=cnt, rng_mode=self.rng_mode)
            _RECTS[k] = (img[y0:y1, x0:x1].copy(), tuple(int(cnt.as_dict()[c]) for c in KEYS))
        return _RECTS[k]

    def _frame(self, tiles=None):
        shuffle = tuple(int(x) for x in self.O.frame_shuffle(MC.SEED, self.acc.frames_done))
        spheres, cam_raw, cam_key = self._frame_inputs(tiles)
        mean = np.zeros((self.h, self.w, 4), np.float32)
        for rect in self._rects(tiles):
            img, cnt = self._render(spheres, cam_raw, cam_key, shuffle, rect)
            x0, x1, y0, y1 = rect
            mean[y0:y1, x0:x1] = img
            for c, v in zip(KEYS, cnt):
                self.counters[c] += v
        self._blend(mean, tiles)

    def render(self, frames=1):
        for _ in range(frames):
            if self.spheres is None:
                raise MC.Refused(NO_SCENE, "render")
            self._frame(None)

    def render_tiles(self, tiles, frames=1):
        tiles = [int(t) for t in np.asarray(tiles).ravel()]
        if not tiles or frames == 0:
            return
        if self.spheres is None:
            raise MC.Refused(NO_SCENE, "render_tiles")
        if self.rng_mode == 1 and self.spp > COUNTER_BLOCK:
            raise MC.Refused(INVALID_ARG, "render_tiles")
        if len(tiles) > self.n_tiles or max(tiles) >= self.n_tiles or len(set(tiles)) != len(tiles):
            raise MC.Refused(INVALID_ARG, "render_tiles")
        if len(tiles) == self.n_tiles:
            return self.render(frames)
        for _ in range(frames):
            self._frame(tiles)
        self._counted(tiles, frames)

    def _oldest(self):
        return max(self.noise_first, self.noise_seq - NOISE_RING + 1 if self.noise_seq >= NOISE_RING else 1)

    def _named_report(self, where, seq, kind):
        if not self.tracking:
            raise MC.Refused(STATE, where)
        assert seq != 0, "the chains always name a report: 0 depends on what has finished"
        if seq > self.noise_seq or seq < self._oldest() or self.reports[seq]["kind"] != kind:
            raise MC.Refused(STATE, where)

    def render_adaptive(self, frames=1, report_seq=0):
        self._named_report("render_adaptive", report_seq, "max_rel")
        r = self.reports[report_seq]
        sel = adaptive_ref.select(r["map"], r["report"]["threshold"])
        if len(sel):
            self.render_tiles(sel, frames)
        self.selections.append((len(sel), self.n_tiles))
        return report_seq, len(sel)

    def render_budget(self, budget, max_frames=8, report_seq=0):
        if not self.tracking:
            raise MC.Refused(STATE, "render_budget")
        if self.spheres is None:
            raise MC.Refused(NO_SCENE, "render_budget")
        if (self.rng_mode == 1 and self.spp > COUNTER_BLOCK) or not 1 <= max_frames <= 32:
            raise MC.Refused(INVALID_ARG, "render_budget")
        self._named_report("render_budget", report_seq, "sum_s")
        k, res = budget_ref.allocate(self._budget_report(report_seq)["map"], self.acc.n.reshape(self.acc.tr, self.acc.tx), self.max_w,
                                     budget, max_frames)
        self.last_levels = []
        for tiles, run in budget_ref.levels(k):
            self.render_tiles(tiles, run)
            self.last_levels.append((len(tiles), run))
        self.allocations.append(k.ravel().copy())
        return dict(res, used_seq=report_seq, k=k)

    def reset(self):
        self.queue, self.held, self.dropped = [], False, 0
        self.acc.reset()
        self.noise_first = self.noise_seq + 1
        self.counters = dict.fromkeys(KEYS, 0)
        self._after_reset()

    def set_samples_per_frame(self, spp):
        self.spp = spp

    def set_rng_mode(self, mode):
        if mode > 1:
            raise MC.Refused(INVALID_ARG, "set_rng_mode")
        self.rng_mode = mode

    def set_auto_regroup(self, enabled=True, ratio=None, check_every=None):
        pass                                    # (when the library regroups changes no output)

    # ---- output
    def read_framebuffer(self):
        return self.acc.fb.copy()

    def read_counters(self):
        return dict(self.counters)

    def tile_frames(self):
        return self.acc.tile_frames()

    # ---- noise estimate
    def set_noise_tracking(self, enabled):
        if self.acc.frames_done != 0:
            raise MC.Refused(STATE, "set_noise_tracking")
        if bool(enabled) == self.tracking:
            return
        self.tracking = bool(enabled)
        self.noise_first = self.noise_seq + 1

    def noise_query(self, threshold=0.02, floor=0.01, tile_map="max_rel"):
        if not self.tracking:
            raise MC.Refused(STATE, "noise_query")
        a = self.acc
        rep = a.report(threshold, floor, diverged=a.diverged)
        if a.diverged:
            self.k_consumers.append(("query", int(a.n.max())))
        tmap = self._sum_map() if tile_map == "sum_s" else a.tiles(threshold, floor, diverged=a.diverged)
        self.noise_seq += 1
        rep.update(seq=self.noise_seq, frames_done=a.frames_done, threshold=float(np.float32(threshold)), floor=float(np.float32(floor)))
        self.reports[self.noise_seq] = {"report": rep, "map": tmap, "kind": tile_map}
        self.reports.pop(self.noise_seq - NOISE_RING, None)

    def noise_result(self, wait=True):
        if self.noise_seq < self.noise_first:
            return None
        return dict(self.reports[self.noise_seq]["report"])

    def read_noise(self):
        if not self.tracking:
            raise MC.Refused(STATE, "read_noise")
        return self.acc.S.copy()

    def read_noise_tiles(self):
        if not self.tracking or self.noise_seq < self.noise_first:
            raise MC.Refused(STATE, "read_noise_tiles")
        return self.reports[self.noise_seq]["map"].copy()

    # ---- denoiser
    def set_denoise_adaptive(self, enabled):
        self.denoise_adaptive_on = bool(enabled)

    def set_denoise_variance(self, mode, spatial_frames=3):
        if mode not in (0, 1, 2) or not 1 <= spatial_frames <= 64:
            raise MC.Refused(INVALID_ARG, "set_denoise_variance")
        self.var_mode, self.spatial_frames = mode, spatial_frames

    def set_denoise_mix(self, enabled, gain=None):
        self.mix_on = bool(enabled)
        if gain is not None:
            self.mix_gain = gain

    def _denoise_check(self, where, tracking=True):
        if tracking and not self.tracking:
            raise MC.Refused(STATE, where)
        if self.spheres is None:
            raise MC.Refused(NO_SCENE, where)
        if self.acc.diverged and not self.denoise_adaptive_on:
            raise MC.Refused(STATE, where)

    def _denoised(self):
        a = self.acc
        if a.diverged:
            g = self._guides_for("denoise-tiles")
            counts = self._denoise_counts()
            table = adaptive_ref.k_table(int(np.max(counts)), self.max_w)
            kw = dict(mode=self.var_mode, spatial_frames=self.spatial_frames, k_of=lambda n: table[int(n)])
            self.denoises.append(np.asarray(counts).ravel().copy())
            self.k_consumers.append(("denoise", int(a.n.max())))
            if self.mix_on:
                return denoise_mix_ref.denoise_mix_tiles(a.fb, a.S, counts, g, None, gain=self.mix_gain, **kw)
            return denoise_tiles_ref.denoise_tiles(a.fb, a.S, counts, g, None, **kw)
        g = self._guides_for("denoise")
        K = adaptive_ref.k_table(a.frames_done, self.max_w)[-1]
        variance = denoise_var_ref.variance_of(self.var_mode, a.frames_done, self.spatial_frames)
        if self.mix_on:
            return denoise_mix_ref.denoise_mix(a.fb, a.S, K, g, None, variance, self.mix_gain)
        return denoise_var_ref.denoise_var(a.fb, a.S, K, g, None, variance)

    def read_denoised(self):
        self._denoise_check("read_denoised")
        return self._denoised()

    def debug_read_guides(self):
        self._denoise_check("debug_read_guides", tracking=False)
        return {k: v.copy() for k, v in self._guides_for("read").items()}

    # ---- temporal reprojection: motion_chains.Model's step, which reads the guides and the (per-tile) framebuffer
    def _step_guides(self):
        return self._guides_for("step")

    # ---- present pass
    def present(self, fmt="rgba8", flip=True, gathered=False, denoise=False, temporal=False):
        assert not gathered and not (denoise and temporal) and len(self.queue) + self.held <= 2
        if denoise:
            self._denoise_check("present")
            src = self._denoised()
        elif temporal:
            self._temporal_check("present", True)
            src = self.read_temporal()
        else:
            src = self.acc.fb
        img = encode_host(self.L, src, fmt, flip)
        self.present_seq += 1
        info = {"seq": self.present_seq, "frames_done": self.acc.frames_done, "width": self.w, "rows": img.shape[0], "row_bytes": 4 * self.w,
                "format": {"rgba8": 1, "bgra8": 2}[fmt], "flags": (FLIP_Y if flip else 0) | (DENOISED if denoise else 0) | (TEMPORAL if temporal else 0)}
        self.queue.append((img, info))

    def acquire_presented(self, newest=True, wait=True, copy=True):
        if self.present_seq == 0:
            raise MC.Refused(STATE, "acquire_presented")
        assert not newest, "the chains acquire the oldest image: the newest finished one depends on the schedule"
        self.held = False
        if not self.queue:
            return None
        img, info = self.queue.pop(0)
        info = dict(info, dropped=self.dropped)
        self.dropped, self.held = 0, True
        return img, info


# ------------------------------------------------------------------ comparing

def compare(name, got, want):
    """None, or what differs between the implementation's and the model's value of one call (motion_chains.Run's hook)"""
    if name in ("tile_frames", "read_noise", "read_noise_tiles", "read_denoised", "render_adaptive", "noise_result", "acquire_presented"):
        return SS.compare((name,), got, want)   # bit for bit; a report's doubles at REPORT_REL
    if name == "read_temporal":
        return None if MC._same(got, want) else MC._describe(got, want)
    if name == "render_budget":
        for f in ("used_seq", "tile_frames", "tiles", "frames"):
            if got[f] != want[f]:
                return f"budget result {f}: {got[f]} against {want[f]}"
        for f in ("var_before", "var_after"):   # bit for bit, as tests/test_gpu_adaptive_budget.py holds them
            if np.float64(got[f]).view(np.uint64) != np.float64(want[f]).view(np.uint64):
                return f"budget result {f}: {got[f]!r} against {want[f]!r}"
        if not np.array_equal(got["k"], want["k"]):
            return f"k_t {got['k'].ravel().tolist()} against {want['k'].ravel().tolist()}"
    return None


def extra_check(run):
    """what a check compares on top of motion_chains.Run.check: n_t, S, the newest report and its map, the denoised image"""
    m = run.model
    names = ["tile_frames"] + (["read_noise", "noise_result", "read_noise_tiles", "read_denoised"] if m.tracking else [])
    for name in names:
        status, got, want = run._both(name)
        if status != OK:                        # (refused by both: no report since the reset, a denoise the state does not allow)
            continue
        bad = compare(name, got, want)
        if bad:
            run._fail(f"{name}: {bad}")
    run.stats["diverged checks"] = run.stats.get("diverged checks", 0) + bool(m.acc.diverged)


# ------------------------------------------------------------------ the chains

def _p(layout, max_w=1.0, size=SMALL_IMAGE):
    return dict(layout=layout, flavour="adaptive", max_w=max_w, size=size)


def _start(layout, in_flight=None, frames=2, temporal=False):
    """a scene, tracking, the per-launch settings, `frames` whole frames"""
    ops = [("set_world", layout), ("tracking", True)]
    if in_flight:
        ops += [("set_frame_batching", 0), ("set_frames_in_flight", in_flight)]
    if temporal:
        ops += [("set_temporal", True)]
    return ops + [("render", frames)]


_U = lambda kind, seed: ("update", kind, seed)
_S = lambda tiles, k=1: ("subset", tuple(tiles), k)
_Q = lambda kind="max_rel", thr=0.3, fl=0.02: ("query", thr, fl, kind)
_CAM = lambda a, d=13.0, h=2.5: ("set_camera", a, d, h)
_MAT = lambda kind, seed, restart=False: ("materials", kind, seed, restart)
_STEP = ("temporal_step",)
CHECK = ("check",)
LONG = K_TABLE_FIRST + 4                        # one tile's run of subset frames that takes its n_t past a K table's length

CHAINS = {
    # 1: every kind of mrt_update_spheres between subset frames queued without a wait, then whole frames
    "edits": (_p("small"), _start("small", 4) + [
        _S((0, 3)), _U("jitter", 101), _S((1, 4), 2), _U("scatter", 102), ("render", 2), CHECK,
        _Q("sum_s"), _S((2,)), _U("partial", 103), ("budget", 8, 2, 1), _S((0, 5)), _U("shrink", 104), ("render", 2), _U("ground", 105), CHECK,
        _S((3, 4), 2), _U("jitter", 106), _S((1,)), _U("partial", 107), ("render", 2), _Q(), CHECK]),
    # 2: the caller's regroup and the policy's, subset frames on both sides; the gate opens behind the scatter
    "regroups": (_p("small"), _start("small", 8) + [
        _S((1, 2)), _U("scatter", 201), ("regroup",), _S((0, 1)), _U("jitter", 202), ("render", 2), CHECK,
        ("auto_regroup", True, 1.0, 1), _S((4,)), _U("jitter", 203), _S((3, 5)), _U("scatter", 204), _S((0,), 2), _U("jitter", 205), CHECK,
        _S((2, 4)), _U("jitter", 206), _S((1,)), ("render", 1), ("auto_regroup", False, 1.0, 1), ("regroup",), _S((5,)), _Q("sum_s"), CHECK]),
    # 3: every kind of material edit between subset frames; the flagged one with a temporal step right behind it
    "materials": (_p("small", 0.75), _start("small", 4, temporal=True) + [
        _CAM(0.0, 5.0, 1.5), _S((0, 1)), _MAT("recolour", 301), _S((2, 3)), _MAT("types", 302), _S((4,), 2), ("render", 1), _STEP, CHECK,
        _MAT("partial", 303), _S((1, 5)), _MAT("ground", 304), _S((0,)), _MAT("glass-one", 305), _S((5,)), ("render", 1), _STEP, CHECK,
        _S((3, 4)), _MAT("partial", 306, True), _STEP, ("read_temporal",), _S((2,)), _STEP, _Q(), CHECK]),
    # 4: another camera and another sphere count on a diverged accumulation, no reset: S, n_t and the blend go on over two pictures
    "two-pictures": (_p("small", size=WIDE_IMAGE), _start("small", 8, 3) + [
        _S((0, 7, 14)), _Q(), _CAM(0.35, 12.0, 3.0), _S((1, 8, 15), 2), ("render", 1), _Q(), CHECK,
        ("set_world", "large-quad"), _S((2, 3, 9), 2), ("render", 2), _Q("sum_s"), CHECK,
        ("budget", 20, 2, 3), ("adaptive", 1, 2), _S((4, 10, 16, 17)), _CAM(-0.3, 14.0, 2.0), _S((5, 11)), ("set_world", "small"), _S((6, 12, 13)), ("render", 1), _Q(), CHECK]),
    # 5: the intended temporal loop (weight 0): a step behind every frame, subset frames among them, both orders of update and subset
    "temporal-0": (_p("small", 0.0), _start("small", 4, 1, temporal=True) + [
        _STEP, _S((0, 1)), _STEP, _U("jitter", 501), _S((2, 4)), _STEP, CHECK,
        _S((3,)), _U("jitter", 502), _STEP, ("read_temporal",), ("render", 1), _STEP, ("present", "temporal"), CHECK,
        _CAM(0.03), _S((1, 5)), _STEP, _U("partial", 503), ("render", 1), _STEP, _S((0, 2)), _U("ground", 504), _STEP, CHECK]),
    # 5 again at 0.75, on the wider image: the blend weights differ per tile while the history follows the motion
    "temporal-075": (_p("small", 0.75, WIDE_IMAGE), _start("small", None, 2, temporal=True) + [
        _STEP, _S((0, 6, 12, 17)), _STEP, _U("jitter", 511), _S((1, 7, 13), 2), _STEP, _Q(), CHECK,
        _S((5, 11)), _U("partial", 512), _STEP, ("read_temporal",), ("present", "temporal"), ("render", 1), _STEP, CHECK,
        _MAT("recolour", 513, True), _S((2, 8)), _STEP, _U("jitter", 514), ("render", 1), _STEP, CHECK]),
    # 6: the per-tile denoise in every variance mode, with and without the blend, right behind an update and a material edit
    "denoise": (_p("small", size=WIDE_IMAGE), _start("small", 4, 3) + [
        ("denoise_adaptive", True), _S((0, 7, 8), 2), _S((3, 10, 17)), _U("jitter", 601), ("read_denoised",),
        ("denoise_variance", 1, 3), _MAT("recolour", 602), ("read_denoised",), ("denoise_mix", True, 1.0), ("read_denoised",), CHECK,
        ("denoise_variance", 2, 5), _S((1, 2)), _U("partial", 603), ("read_denoised",), ("denoise_mix", False, 1.0), ("read_denoised",),
        ("denoise_variance", 0, 3), ("denoise_mix", True, 2.0), _S((4,), 3), ("read_denoised",), ("present", "denoised"), CHECK]),
    # 6, the long runs: one tile's n_t passes the device K table's length twice (4096, then 8192), a denoise and a report behind each
    # (the device makes its table at the first per-tile consumer: the denoise and the report behind the first subset frames make the
    # one of 4096 entries, which the consumers behind the long runs then replace twice, each time under queued work that read it)
    "denoise-long": (_p("small"), _start("small", None, 2) + [
        ("denoise_adaptive", True), _S((1,), 2), ("read_denoised",), _Q(), _U("jitter", 611), _S((4,), LONG), ("read_denoised",), _Q(), CHECK,
        ("denoise_variance", 2, 6), _MAT("types", 612), _S((4,), LONG), ("read_denoised",), ("denoise_mix", True, 1.0),
        ("denoise_variance", 1, 3), ("read_denoised",), ("present", "denoised"), _Q("sum_s"), CHECK]),
    # 7: reports of both kinds before and after an edit, selections and allocations from the older ones, the ring of 8
    "reports": (_p("small", size=WIDE_IMAGE), _start("small", 4, 3) + [
        _Q("max_rel", 0.5), _Q("sum_s"), _S((0, 1)), _U("jitter", 701), _Q("max_rel", 0.6), _Q("sum_s"), ("adaptive", 2, 1), ("budget", 20, 3, 2), CHECK,
        _MAT("recolour", 702), ("adaptive", 1, 3), ("budget", 30, 4, 4), _Q("max_rel", 0.25), ("refuse", "adaptive-on-sums", 4),
        ("refuse", "budget-on-max-rel", 5), CHECK,
        _U("partial", 703), _Q("sum_s"), ("budget", 36, 2, 6), ("adaptive", 1, 5), _Q(), _Q(), _Q(), ("refuse", "old-report", 1), CHECK]),
    # 7 again: nine queries in a row and the refusal of the first, selections on the small image, a budget that gives every tile the same
    "ring": (_p("small"), _start("small", 8, 4) + [
        _Q("sum_s"), ("budget", 12, 2, 1), CHECK, _Q("max_rel", 0.35), ("adaptive", 1, 2), _S((4,)), _U("jitter", 711),
        _Q("max_rel", 0.5), _Q("sum_s"), _Q("max_rel", 0.2), _Q(), _Q("sum_s"), _Q(), _Q("max_rel", 0.25), _Q(), _Q(),
        ("refuse", "old-report", 3), CHECK, ("adaptive", 2, 5), ("budget", 9, 3, 7), _U("scatter", 712), ("adaptive", 1, 9), ("budget", 7, 2, 4),
        ("refuse", "duplicate-tile"), CHECK]),
    # 8: the masks forced, then the lists: subset launches under generations begun by an update, a regroup and a camera, twice
    "tables": (_p("small"), _start("small", 4) + [
        ("set_camera_masks", 3), _S((0, 1)), _U("jitter", 801), _S((2, 3), 2), ("regroup",), _S((4,), 2), _CAM(0.2), _S((0, 5), 2),
        ("render", 2), CHECK,
        ("set_camera_masks", 2), ("set_frames_in_flight", 8), _S((1, 2), 2), _U("partial", 802), _S((3,), 2), ("regroup",), _S((4, 5), 2),
        _CAM(-0.2), _S((0,), 2), CHECK, _U("jitter", 803), _S((1,), 3), ("render", 1), CHECK]),
    # 9: a reset in the middle of a diverged, moving chain: the uniform paths are back, then the accumulation diverges again
    "reset": (_p("small"), _start("small", 4) + [
        _S((0, 1), 2), _U("jitter", 901), _S((2,)), ("refuse", "denoise-off"), CHECK,
        _U("scatter", 902), ("reset",), CHECK, ("render", 2), ("read_denoised",), _Q(), CHECK,
        _S((3, 4)), _U("jitter", 903), ("refuse", "denoise-off"), ("denoise_adaptive", True), ("read_denoised",), _S((5,), 2), ("render", 1),
        ("reset",), ("render", 1), _S((0,)), _Q("sum_s"), CHECK]),
    # 10: the samples per frame change between subset frames; counter mode renders 64 a frame by tiles and refuses 65
    "spp-rng": (_p("small"), _start("small", 4) + [
        _S((0, 1)), ("spp", 3), _S((2, 3)), _U("jitter", 1001), ("spp", 1), _S((4,), 2), ("render", 1), CHECK,
        ("rng_mode", 1), ("spp", 64), _S((5,)), _S((1, 2)), _U("partial", 1002), ("spp", 65), ("refuse", "counter-65"), CHECK,
        ("spp", 2), _S((0, 3)), ("rng_mode", 0), _S((4, 5)), ("render", 1), _Q(), CHECK]),
    # 11: batched whole frames behind an update are blended per tile, in both forms of a batch
    "batched": (_p("small", size=WIDE_IMAGE), _start("small", None, 2) + [
        _S((0, 6, 12)), _Q("sum_s"), ("set_frame_batching", 2), _U("jitter", 1101), ("render", 3), ("budget", 24, 3, 1), _S((1, 7), 2),
        _Q("max_rel", 0.2), CHECK,
        ("set_frame_batching", 3), _U("partial", 1102), ("render", 4), ("adaptive", 2, 2), _S((2, 8, 14), 3), _U("ground", 1103), ("render", 2),
        _Q(), CHECK]),
    # 12: the large layout through 1, 2, 5 and 6
    "large": (_p("large-quad", 0.75), _start("large-quad", 4, temporal=True) + [
        ("set_regroup_block", 4), ("denoise_adaptive", True), _STEP, _S((0, 4)), _U("jitter", 1201), _S((1, 2), 2), _STEP, CHECK,
        _U("scatter", 1202), ("regroup",), _S((3,)), _STEP, ("read_denoised",), ("auto_regroup", True, 1.0, 1), _U("jitter", 1203), CHECK,
        _S((5,)), _U("scatter", 1204), _S((0, 1)), _U("jitter", 1205), ("render", 1), _STEP, ("denoise_variance", 1, 3), ("read_denoised",),
        ("read_temporal",), _Q(), CHECK]),
}
NAMES = tuple(CHAINS)


def new_model(O, name, cls=None):
    return MC.new_model(O, CHAINS[name][0], cls or Model)


def new_run(name, impl, model, O, stats=None, after=None, device_checks=True):
    return MC.Run(f"adaptive chain {name}", CHAINS[name][0], impl, model, O, stats, after, device_checks, shadow=Shadow(),
                  compare=compare, extra_check=extra_check)


def run(name, impl, model, O, stats=None, after=None, device_checks=True):
    """chain `name` on impl and model in lock step (motion_chains.Run); raises ChainMismatch at the first difference"""
    r = new_run(name, impl, model, O, stats, after, device_checks)
    for op in CHAINS[name][1]:
        r.step(op)
    return r
