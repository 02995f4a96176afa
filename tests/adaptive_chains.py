"""Chains that put the adaptive accumulation on a scene that changes: subset frames (mrt_render_tiles, mrt_render_adaptive,
mrt_render_budget), the per-tile blend, noise reports of both map kinds, the per-tile denoise and its blend, next to
mrt_update_spheres, mrt_regroup_spheres, mrt_set_auto_regroup, mrt_update_materials, mrt_set_camera, mrt_set_world, mrt_reset and
mrt_temporal_step, up to forty ops each, checked against a host model.

The runner is motion_chains' own (Run, CameraTables, ChainStopped, ChainMismatch, new_state), through the hooks it has for this
module: an image size per chain (params["size"]), a Shadow of the caller's, a compare(name, got, want) behind every call both sides
accepted, an extra_check in every check, and render launches that name their tile list.  Seventeen chains are written out
(CHAINS); a name reproduces its ops anywhere.  chain(case) draws further ones from a seed (its rules stand above PLAN), and
`python tests/adaptive_chains.py CASE` prints one.  On top of motion_chains' and material_chains' ops:

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
  ("temporal_response", enabled, fast_history, clamp_sigma, antilag)    mrt_set_temporal_response (motion_chains.Model has it)
  ("get_temporal_response",)                mrt_get_temporal_response, compared where it stands
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
import os
import sys

import numpy as np

if __name__ == "__main__":                      # (python tests/adaptive_chains.py CASE: the package lies one directory up)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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
# mrt_set_temporal_response's refusals, one reason at a time: the setting as it stands but for the one number (or reserved word)
RESPONSE_REFUSALS = {"fast-history-0": ("fast_history", 0), "fast-history-17": ("fast_history", 17), "clamp-sigma-0": ("clamp_sigma", 0.0),
                     "clamp-sigma-nan": ("clamp_sigma", float("nan")), "clamp-sigma-inf": ("clamp_sigma", float("inf")),
                     "antilag-negative": ("antilag", -0.1), "antilag-above-1": ("antilag", 1.5), "antilag-nan": ("antilag", float("nan")),
                     "response-reserved": ("reserved", 1)}
REFUSALS = ("denoise-off", "adaptive-on-sums", "budget-on-max-rel", "old-report", "duplicate-tile", "counter-65",
            "present-temporal-dropped") + tuple(RESPONSE_REFUSALS)
REFUSAL_STATUS = dict({"denoise-off": STATE, "adaptive-on-sums": STATE, "budget-on-max-rel": STATE, "old-report": STATE,
                       "duplicate-tile": INVALID_ARG, "counter-65": INVALID_ARG, "present-temporal-dropped": STATE},
                      **dict.fromkeys(RESPONSE_REFUSALS, INVALID_ARG))
VOCABULARY = ("tracking", "subset", "query", "adaptive", "budget", "denoise_adaptive", "denoise_variance", "denoise_mix", "read_denoised",
              "read_temporal", "present", "auto_regroup", "spp", "rng_mode", "refuse", "materials", "temporal_response",
              "get_temporal_response")
UNION_VOCABULARY = tuple(dict.fromkeys(MC.VOCABULARY + ("refused_materials",) + VOCABULARY))       # what the runner accepts
SMALL_IMAGE, WIDE_IMAGE = (20, 12), (44, 20)    # 3 x 2 and 6 x 3 tiles, both with a ragged right column and top band


class Shadow(XC.Shadow):
    response = (False, 4, 2.0, 1.0)             # mrt_set_temporal_response's setting as the legal calls have left it

    def calls(self, op):
        name, a = op[0], op[1:]
        if name == "temporal_response":
            self.response = tuple(a)
        if name == "refuse" and a[0] in RESPONSE_REFUSALS:
            field, bad = RESPONSE_REFUSALS[a[0]]
            now = dict(zip(("enabled", "fast_history", "clamp_sigma", "antilag"), self.response))
            if field == "reserved":
                return [("set_temporal_response_raw", tuple(self.response) + (bad,))]
            return [("set_temporal_response", dict(now, **{field: bad}))]
        if name == "refuse" and a[0] == "present-temporal-dropped":
            return [("present", ("rgba8", True, False, False, True))]
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
_R = lambda on, fh=4, cs=2.0, al=1.0: ("temporal_response", on, fh, cs, al)
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
    # 13: the temporal response at weight 0: steps with the fast history, the clamp and the anti-lag behind subset frames, an
    # update and a flagged material edit (the NaN stays in "previous"); `enabled` off and on again in the middle, a check of
    # each dropped history (the read refuses; the H2 the next step reads is zeroes); the numbers alone changed; five refusals
    "response-0": (_p("small", 0.0), _start("small", 4, 1, temporal=True) + [
        _R(True, 2, 1.0, 1.0), _STEP, _S((0, 1)), _STEP, _U("jitter", 1301), _S((2, 4)), _STEP, ("get_temporal_response",), CHECK,
        _MAT("partial", 1302, True), _S((3,)), _STEP, ("read_temporal",), ("refuse", "fast-history-0"), ("refuse", "clamp-sigma-nan"),
        ("refuse", "antilag-negative"), CHECK,
        _R(False, 2, 1.0, 1.0), ("refuse", "present-temporal-dropped"), CHECK, _S((1, 5)), _STEP, _R(True, 2, 1.0, 1.0), CHECK,
        _U("partial", 1303), _S((0, 2)), _STEP,
        _R(True, 3, 0.5, 0.5), ("render", 1), _STEP, ("present", "temporal"), ("refuse", "response-reserved"), ("refuse", "antilag-nan"), CHECK]),
    # 13 on the large layout at 0.75, the wider image: the policy regroups between two steps, the per-tile denoise is read right
    # behind a step, fast_history 1 (every clamped length turns fractional at once)
    "response-large": (_p("large-quad", 0.75, WIDE_IMAGE), _start("large-quad", 4, 2, temporal=True) + [
        ("set_regroup_block", 4), ("denoise_adaptive", True), _R(True), _STEP, _S((0, 6, 12)), _STEP, ("auto_regroup", True, 1.0, 1),
        _U("jitter", 1401), _S((1, 7), 2), _STEP, ("read_denoised",), CHECK,
        _U("scatter", 1402), _S((2, 8)), _STEP, ("read_temporal",), ("refuse", "fast-history-17"), ("refuse", "clamp-sigma-0"), CHECK,
        _R(True, 1, 0.5, 1.0), _U("jitter", 1403), ("render", 1), _STEP, ("read_denoised",), ("present", "temporal"),
        ("refuse", "clamp-sigma-inf"), ("refuse", "antilag-above-1"), CHECK]),
}
NAMES = tuple(CHAINS)


# ------------------------------------------------------------------ the generator
#
# chain(case) draws (params, ops) from np.random.default_rng(case) in a fixed order: a case number reproduces its chain anywhere
# (`python tests/adaptive_chains.py CASE` prints it).  PLAN[case % len(PLAN)] fixes the layout, max_framebuffer_weight, image and
# flavour, so the cross product is covered by construction; case // len(PLAN) rotates the segments a flavour is made of.  The
# generator follows a Shadow (geometry, camera) and a few scalars of its own and emits only chains that are legal to compare:
#   - at most 40 ops; a check at least every 8 ops and at the end; a segment that would not fit is taken back whole;
#   - a check follows every regroup before the grouping changes again (a regroup, another scene), and every third update;
#   - a camera the update left stale (Shadow.camera_stale) is set anew right behind it; coordinates stay below half of 1e7;
#   - mrt_render_adaptive and mrt_render_budget always name a report (never 0): one of the ring of 8, since the last reset, of
#     the right map kind -- unless the op is a ("refuse", ...), which breaks exactly one of these;
#   - they are drawn on a diverged accumulation only, and a subset lists fewer tiles than the image has, so whether the
#     accumulation has diverged never depends on what a selection or an allocation happened to hold;
#   - a present is followed by its oldest acquire that waits (one op): at most two presented images are outstanding;
#   - in counter mode a subset frame has at most 64 samples; 65 is set only for the "counter-65" refusal and taken back behind it;
#     the samples stay below 96, where the camera tables' decision would depend on the device;
#   - read_denoised and the denoised present: noise tracking on, and the per-tile denoise enabled once the accumulation has
#     diverged; read_temporal and the temporal present: a step since the history was last dropped (mrt_set_world,
#     mrt_temporal_reset, mrt_set_temporal off, a change of the response's `enabled`); mrt_temporal_step: a frame since the reset.
#     Where one of them is not legal it is drawn only as a refusal, one reason at a time;
#   - mrt_debug_set_frame_batching(0) with 4 or 8 frames in flight right behind the scene, as _start has them, or neither; the
#     batched forms (2, 3) only in a chain that began with neither; the forced tables (3, 2) only on the small layout;
#   - no run of subset frames past the device's K table (LONG): those stay in "denoise-long".
PLAN = (("small", 1.0, SMALL_IMAGE, "plain"), ("small", 0.0, SMALL_IMAGE, "response"), ("large-quad", 0.75, WIDE_IMAGE, "response"),
        ("large-lin", 1.0, SMALL_IMAGE, "denoise"), ("small", 0.75, WIDE_IMAGE, "tables"), ("large-lin", 0.0, SMALL_IMAGE, "temporal"),
        ("large-quad", 1.0, SMALL_IMAGE, "plain"), ("small", 0.75, SMALL_IMAGE, "response"), ("large-lin", 0.75, WIDE_IMAGE, "response"),
        ("small", 1.0, WIDE_IMAGE, "denoise"), ("large-quad", 0.0, SMALL_IMAGE, "temporal"), ("large-lin", 1.0, WIDE_IMAGE, "plain"))
SUITE_CASES = tuple(range(24))
FLAVOURS = ("plain", "temporal", "response", "denoise", "tables")
MAX_OPS, CHECK_EVERY = 40, 8
EDIT_KINDS = ("jitter", "scatter", "partial", "shrink", "ground")
# the segments of a flavour, by the case's ordinal among the cases of that flavour (a segment that does not fit is left out)
SEGMENTS = {
    "plain": (("reports", "two_pictures", "refusals"), ("spp", "reset", "edits"), ("spp", "batched", "edits"),
              ("regroups", "materials", "edits"), ("reports", "two_pictures", "refusals"), ("reset", "spp", "regroups")),
    "temporal": (("temporal_reset", "temporal", "materials"), ("large", "temporal_reset", "temporal"), ("temporal", "reset", "edits"),
                 ("temporal_reset", "large")),
    "response": (("response", "temporal", "toggle"), ("large", "toggle", "response"), ("toggle", "materials", "temporal"),
                 ("response", "toggle", "edits"), ("toggle", "temporal", "response"), ("response", "large", "toggle"),
                 ("temporal", "toggle", "materials"), ("toggle", "response", "reports")),
    "denoise": (("denoise", "reports"), ("denoise", "edits"), ("spp", "denoise"), ("denoise", "materials")),
    "tables": (("tables",), ("tables",)),
}


def chain(case: int):
    """-> (params, ops) of a random chain: params as the written chains', ops from the runner's vocabulary (UNION_VOCABULARY)"""
    import copy
    rng = np.random.default_rng(case)
    layout, max_w, size, flavour = PLAN[case % len(PLAN)]
    p = dict(layout=layout, flavour=flavour, max_w=max_w, size=size)
    ordinal = [c for c in range(case + 1) if PLAN[c % len(PLAN)][3] == flavour].index(case)
    segments = SEGMENTS[flavour][ordinal % len(SEGMENTS[flavour])]
    n_tiles = -(-size[0] // 8) * -(-size[1] // 8)
    temporal = flavour in ("temporal", "response")
    sh, ops = Shadow(), []
    g = dict(frames=0, diverged=False, temporal=False, stepped=False, response=(False, 4, 2.0, 1.0), seq=0, first=1, kinds={},
             spp=MC.SPP, rng_mode=0, adaptive_denoise=False, owed=False, updates=0, since=0, drawn=0, edited=0)
    chance = lambda q: bool(rng.random() < q)
    seed = lambda: int(rng.integers(0, 2 ** 31))
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]

    def emit(*op):
        if op != CHECK and ops and (g["since"] >= CHECK_EVERY - 1 or (op[0] in ("regroup", "set_world") and g["owed"])):
            emit(*CHECK)
        if op == CHECK and ops[-1] == CHECK:
            return
        ops.append(op)
        sh.calls(op)
        assert sh.sc is None or max(float(np.abs(sh.xyzr()).max()), float(np.abs(sh.cam[0]).max())) <= 0.5 * MC.LIMIT
        name = op[0]
        g["since"] = 0 if name == "check" else g["since"] + 1
        if name == "check":
            g.update(updates=0, owed=False)
        elif name == "regroup":
            g["owed"] = True
        elif name == "render":
            g["frames"] += op[1]
        elif name == "subset":
            assert 0 < len(op[1]) < n_tiles and op[2] < K_TABLE_FIRST and (g["rng_mode"] == 0 or g["spp"] <= COUNTER_BLOCK)
            g["frames"] += op[2]
            g["diverged"] = True
        elif name == "reset":
            g.update(frames=0, diverged=False, first=g["seq"] + 1)
        elif name == "set_world":
            g["stepped"] = False
        elif name == "set_temporal":
            g.update(temporal=op[1], stepped=g["stepped"] and op[1])
        elif name == "temporal_step":
            assert g["temporal"] and g["frames"]
            g["stepped"] = True
        elif name == "temporal_reset":
            g["stepped"] = False
        elif name == "temporal_response":
            g.update(stepped=g["stepped"] and op[1] == g["response"][0], response=op[1:])
        elif name == "query":
            g["seq"] += 1
            g["kinds"][g["seq"]] = op[3]
        elif name in ("adaptive", "budget"):
            assert g["diverged"] and op[-1] in named({"adaptive": "max_rel", "budget": "sum_s"}[name])
        elif name == "spp":
            g["spp"] = op[1]
        elif name == "rng_mode":
            g["rng_mode"] = op[1]
        elif name == "denoise_adaptive":
            g["adaptive_denoise"] = op[1]
        elif name in ("read_denoised", "present") and op[-1] != "temporal":
            assert g["adaptive_denoise"] or not g["diverged"]
        elif name == "read_temporal" or op == ("present", "temporal"):
            assert g["temporal"] and g["stepped"]
        if name == "update":
            g["updates"] += 1
            if sh.camera_stale():
                emit("set_camera", float(rng.uniform(-0.5, 0.5)), float(rng.uniform(11.0, 15.0)), float(rng.uniform(2.0, 3.0)))
            if g["updates"] >= 3:
                emit(*CHECK)

    def room(n, updates=1):                     # the next n ops stand together: no check of the two rules falls among them
        if g["since"] + n > CHECK_EVERY - 1 or g["updates"] + updates >= 3:
            emit(*CHECK)

    def named(kind):                            # the reports of one map kind that a selection or an allocation may name
        oldest = max(g["first"], g["seq"] - NOISE_RING + 1, 1)
        return [s for s in range(oldest, g["seq"] + 1) if g["kinds"][s] == kind]

    def report(kind):
        if not named(kind):
            query(kind)
        return pick(named(kind))

    def tiles(most=4):
        k = int(rng.integers(1, min(most, n_tiles - 1) + 1))
        return tuple(sorted(int(t) for t in rng.choice(n_tiles, k, replace=False)))

    def subset(most=4, frames=None):
        emit("subset", tiles(most), int(rng.integers(1, 3)) if frames is None else frames)

    def update(kind=None):
        g["drawn"] += 1
        emit("update", kind or EDIT_KINDS[(case + g["drawn"]) % len(EDIT_KINDS)], seed())

    def materials(restart=False):
        g["edited"] += 1
        emit("materials", XC.MATERIAL_KINDS[(case + g["edited"]) % len(XC.MATERIAL_KINDS)], seed(), restart)

    def query(kind=None):
        emit("query", pick((0.2, 0.3, 0.5)), 0.02, kind or pick(("max_rel", "sum_s")))

    def camera():
        emit("set_camera", float(rng.uniform(-0.4, 0.4)), float(rng.uniform(11.0, 15.0)), float(rng.uniform(2.0, 3.0)))

    def step():
        if not g["frames"]:
            emit("render", 1)
        emit("temporal_step")

    def diverge():
        if not g["diverged"]:
            subset()

    def numbers():
        return pick((1, 2, 4, 16)), pick((0.5, 1.0, 2.0, 3.0)), pick((0.0, 0.5, 1.0))

    # -- the segments (the situations of the written chains, with drawn tiles, kinds, seeds and numbers)
    def seg_edits():                            # 1: updates between subset frames queued without a wait, then whole frames
        diverge()
        room(5, 2)
        subset()
        update()
        subset()
        update()
        emit("render", int(rng.integers(2, 4)))

    def seg_regroups():                         # 2: the caller's regroup and the policy's, subset frames on both sides
        diverge()
        room(4)
        subset()
        update(pick(("scatter", "jitter")))
        emit("regroup")
        subset()
        update("jitter")
        emit(*CHECK)
        emit("auto_regroup", True, 1.0, 1)
        subset()
        update(pick(("scatter", "jitter")))
        subset()
        emit(*CHECK)
        emit("auto_regroup", False, pick((1.0, 2.0)), pick((1, 2)))

    def seg_materials():                        # 3: material edits between subset frames; the flagged one with a step behind it
        diverge()
        room(5)
        subset()
        materials()
        subset()
        materials()
        subset()
        if g["temporal"]:
            room(3)
            subset()
            materials(True)
            step()

    def seg_two_pictures():                     # 4: another camera and another scene on a diverged accumulation, no reset
        diverge()
        query()
        camera()
        subset()
        emit("render", 1)
        emit("set_world", pick([l for l in ("small", "large-quad", "large-lin") if l != sh.layout]))
        subset()
        emit("render", int(rng.integers(1, 3)))
        query("sum_s")
        emit("budget", int(rng.integers(6, 25)), int(rng.integers(2, 4)), report("sum_s"))

    def seg_temporal():                         # 5: steps behind subset frames, both orders of update and subset, read and presented
        room(2)
        subset()
        step()
        room(3)
        update("jitter")
        subset()
        step()
        room(3)
        subset()
        update(pick(("jitter", "partial")))
        step()
        if g["stepped"]:
            emit("read_temporal")
            emit("present", "temporal")

    def seg_temporal_reset():
        emit("temporal_reset")
        emit(*CHECK)                            # dropped: the read refuses
        emit("refuse", "present-temporal-dropped")
        emit("render", 1)
        step()

    def seg_response():                         # the response on: steps behind subset frames, the numbers alone changed between two
        if not g["response"][0]:
            emit("temporal_response", True, *numbers())
        step()
        room(2)
        subset()
        step()
        emit("get_temporal_response")
        emit("temporal_response", True, *numbers())
        room(3)
        subset()
        update("jitter")
        step()
        if chance(0.5):
            emit("read_temporal")

    def seg_toggle():                           # `enabled` changed between two steps, a check of each dropped history
        if not g["stepped"]:
            step()
        on, *nums = g["response"]
        emit("temporal_response", not on, *nums)
        emit("refuse", "present-temporal-dropped") if chance(0.5) else emit(*CHECK)
        room(2)
        subset()
        step()
        emit("temporal_response", on, *(numbers() if chance(0.5) else nums))
        emit(*CHECK)
        room(2)
        subset()
        step()

    def seg_denoise():                          # 6: the per-tile denoise by mode and blend, behind an update and a material edit
        emit("denoise_adaptive", True)
        diverge()
        mode = (case // 3) % 3
        emit("denoise_variance", mode, int(rng.integers(2, 7)))
        room(3)
        subset()
        update("jitter")
        emit("read_denoised")
        emit("denoise_mix", True, pick((1.0, 2.0)))
        room(2)
        materials()
        emit("read_denoised")
        emit("denoise_variance", (mode + 1) % 3, int(rng.integers(2, 7)))
        emit("read_denoised")
        emit("denoise_mix", False, 1.0)
        subset()
        emit("read_denoised")
        emit("present", "denoised")

    def seg_reports():                          # 7: reports of both kinds on both sides of an edit, the older ones named
        diverge()
        query("max_rel")
        query("sum_s")
        before = g["seq"]
        subset()
        update("jitter")
        query("max_rel")
        query("sum_s")
        emit("adaptive", int(rng.integers(1, 3)), [s for s in named("max_rel") if s <= before][-1])
        emit("budget", int(rng.integers(6, 37)), int(rng.integers(2, 5)), [s for s in named("sum_s") if s <= before][-1])
        emit("refuse", "adaptive-on-sums", named("sum_s")[-1])
        emit("refuse", "budget-on-max-rel", named("max_rel")[-1])

    def seg_refusals():
        diverge()
        emit("refuse", "duplicate-tile")
        if not g["adaptive_denoise"]:
            emit("refuse", "denoise-off")
        emit(*CHECK)

    def seg_tables():                           # 8: the masks forced, then the lists, subset launches under all three generations
        for mode in (3, 2):
            emit("set_camera_masks", mode)
            if mode == 2:
                emit("set_frames_in_flight", 8)
            kinds = ["update", "regroup", "camera"]
            rng.shuffle(kinds)
            subset(2)
            for kind in kinds:
                update(pick(("jitter", "partial"))) if kind == "update" else emit("regroup") if kind == "regroup" else camera()
                subset(2)
            emit("render", int(rng.integers(1, 3)))
            emit(*CHECK)

    def seg_reset():                            # 9: a reset of a diverged, moving chain; the uniform paths; divergence again
        diverge()
        update("jitter")
        subset()
        if not g["adaptive_denoise"]:
            emit("refuse", "denoise-off")
        query()
        old = g["seq"]
        emit(*CHECK)
        emit("reset")
        if g["temporal"]:
            emit("refused", "step-after-reset", seed())
        emit("render", 2)
        emit("read_denoised")
        emit("refuse", "old-report", old)
        query()
        emit(*CHECK)
        subset()

    def seg_spp():                              # 10: the samples change between subset frames; counter mode at 64, 65 refused
        room(3)
        subset(2, 1)
        emit("spp", pick((1, 3, 5)))
        subset(2, 1)
        room(3)
        emit("rng_mode", 1)
        emit("spp", 64)
        subset(1, 1)
        room(3)
        emit("spp", 65)
        emit("refuse", "counter-65")
        emit(*CHECK)
        emit("spp", MC.SPP)
        emit("rng_mode", 0)

    def seg_batched():                          # 11: batched whole frames behind an update, in both forms of a batch
        diverge()
        for form in (2, 3):
            room(3)
            emit("set_frame_batching", form)
            update(pick(("jitter", "partial")))
            emit("render", int(rng.integers(2, 5)))
            subset()

    def seg_large():                            # 12: subset frames, a regroup, the policy, a step and the per-tile denoise together
        emit("set_regroup_block", 4)
        emit("denoise_adaptive", True)
        room(3)
        subset()
        update("jitter")
        subset()
        if g["temporal"]:
            step()
        update("scatter")
        emit("regroup")
        subset()
        if g["temporal"]:
            step()
        emit("read_denoised")
        emit("auto_regroup", True, 1.0, 1)
        update("jitter")
        emit(*CHECK)

    segs = dict(edits=seg_edits, regroups=seg_regroups, materials=seg_materials, two_pictures=seg_two_pictures, temporal=seg_temporal,
                temporal_reset=seg_temporal_reset, response=seg_response, toggle=seg_toggle, denoise=seg_denoise, reports=seg_reports,
                refusals=seg_refusals, tables=seg_tables, reset=seg_reset, spp=seg_spp, batched=seg_batched, large=seg_large)

    # -- the start: a scene, tracking, the per-launch settings as _start has them, the switches that hold for the chain
    in_flight = 4 if flavour == "tables" else None if "batched" in segments else (4, 8, None)[case % 3]
    for op in _start(layout, in_flight, 1 if temporal else 2, temporal):
        emit(*op)
    emit("set_sweep", case % 3)
    if layout != "small":
        emit("set_regroup_block", (4, 0)[(case // 2) % 2])
    elif flavour != "tables" and case % 2:
        emit("set_camera_masks", bool(case % 4 == 1))
    if flavour == "response":
        emit("temporal_response", True, *numbers())
    if temporal:
        step()
    # one refusal of each family by the case number: every kind turns up in the suite
    emit("refuse", tuple(RESPONSE_REFUSALS)[case % len(RESPONSE_REFUSALS)])
    kinds = [k for k in MC.REFUSALS if k != ("step-while-off" if temporal else "step-after-reset") and k != "step-after-reset"]
    emit("refused", kinds[case % len(kinds)], seed())
    if case % 4 == 1:
        emit("refused_materials")
    for name in segments + tuple(n for n in ("materials", "edits", "refusals") if n not in segments):      # (what still fits)
        saved = (len(ops), copy.deepcopy(g), copy.deepcopy(sh), copy.deepcopy(rng.bit_generator.state))
        segs[name]()
        if len(ops) > MAX_OPS - 1:              # (it does not fit: taken back whole, the draws with it)
            del ops[saved[0]:]
            g.clear()
            g.update(saved[1])
            sh.__dict__.clear()
            sh.__dict__.update(saved[2].__dict__)
            rng.bit_generator.state = saved[3]
    emit(*CHECK)
    assert len(ops) <= MAX_OPS and {op[0] for op in ops} <= set(UNION_VOCABULARY)
    return p, ops


def new_model(O, name, cls=None):
    return MC.new_model(O, params_and_ops(name)[0], cls or Model)


def params_and_ops(name):
    """a written chain by its name, a random one by its case number"""
    return chain(name) if isinstance(name, int) else CHAINS[name]


def new_run(name, impl, model, O, stats=None, after=None, device_checks=True):
    label = f"random adaptive chain {name} (python tests/adaptive_chains.py {name})" if isinstance(name, int) else f"adaptive chain {name}"
    return MC.Run(label, params_and_ops(name)[0], impl, model, O, stats, after, device_checks, shadow=Shadow(),
                  compare=compare, extra_check=extra_check)


def run(name, impl, model, O, stats=None, after=None, device_checks=True):
    """chain `name` on impl and model in lock step (motion_chains.Run); raises ChainMismatch at the first difference"""
    r = new_run(name, impl, model, O, stats, after, device_checks)
    for op in params_and_ops(name)[1]:
        r.step(op)
    return r


if __name__ == "__main__":                      # the case's params and ops, one per line, for replay and bug reports (no device)
    for case in (int(a) for a in sys.argv[1:]):
        params, case_ops = chain(case)
        print(f"case {case}: {params}")
        for i, op in enumerate(case_ops):
            print(f"{i:3d} {op!r}")
