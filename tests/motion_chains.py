"""Chains of calls on a scene that moves: mrt_update_spheres, mrt_regroup_spheres, mrt_set_camera, frames and mrt_temporal_step, many
in a row, checked against a host model.

Every single-step test of these calls starts from a freshly built scene.  What only a chain reaches: the host scalars that
mrt_update_spheres keeps valid monotonically (the sweep's reach, the quadratic box slack's kc, the direct records) and the sweep's
origin, frozen at the build, after a scene has drifted fifty scene sizes, shrunk three times or taken a radius of 0; a partial
update through a member_index that regroups have permuted; the camera masks' generations with 4 to 8 frames in flight; a temporal
history across updates, regroups, resets and a mrt_set_world to another sphere count.

chain(case) draws (params, ops) from np.random.default_rng(case); ops are plain tuples:
  ("set_world", layout)            tests/test_gpu_update_spheres.py's scenes, with the forced hierarchy of its HASH_LAYOUTS
  ("update", kind, seed[, k])      UPDATE_KINDS; "drift" moves k scene sizes in ONE mrt_update_spheres (see drift below) and takes
                                   the camera along; "tiny" is two one-sphere updates
  ("regroup",) ("set_regroup_block", 4 | 0) ("set_camera", angle, distance, height)
  ("render", k) ("reset",) ("set_frames_in_flight", n) ("set_frame_batching", 0) ("set_sweep", m)
  ("set_camera_masks", on)         False / True (1: the library's rule); the list chains: 0, 2 (the lists), 3 (the masks)
  ("set_temporal", on) ("temporal_step",) ("temporal_reset",)
  ("temporal_response", enabled, fast_history, clamp_sigma, antilag)     mrt_set_temporal_response (no chain of this module draws
  ("get_temporal_response",)       it: tests/adaptive_chains.py does); the getter is compared where it stands
  ("refused", kind, seed)          one call the header refuses, REFUSALS
  ("check",)
Shadow turns an op into calls -- it follows the geometry and the camera the way the generator did when it drew the op, without
an oracle -- and Run applies every call to the implementation and to the model and compares statuses; a check compares what the
model can say (frames_done, framebuffer, counters, guides, the temporal history and image) bit for bit and, on a real context,
the hierarchy (tests/refit_ref.py), member_index (tests/regroup_ref.py), the candidate sets under both sweeps, the camera masks
(tests/camera_mask_ref.py), the camera-ray sphere lists (tests/camera_list_ref.py) and mrt_debug_check_context.  Behind every
render the launch's table -- none, the masks, the lists -- is held to CameraTables, a host model of the library's decision.

Drift: a drift op carries the number of scene sizes it moves in ONE mrt_update_spheres.  Chain 8 is the long one: fifty-two drifts of
one scene size each, with frames and checks at the positions between, about 120 ops.  The other chains are kept to forty ops;
their drifts jump 1 .. 16 sizes a call, and the host scalars see the same maxima as after that many single steps.

Checks: every chain ends with one, one follows every third update, and one follows every regroup before the grouping changes
again.  In seg_two_regroups it comes straight behind the regroup, so that the regrouped hierarchy is checked before a refit
rewrites it; in seg_regroup_then_partial and seg_masks updates, camera changes and frames come first on purpose -- they are queued
behind the regroup without a wait, which a check would be -- and the check then sees the hierarchy after the later refit
(member_index is held to the ordering computed at the regroup either way).

A HIP error or a stalled wait from ANY call the runner makes on a real context -- the ops' own (Run._both), the read-backs and
diagnostics of a check and of the steps (Run._dev), the creation of the context (new_state) -- is ChainStopped, which the GPU tests
turn into pytest.exit: nothing more is started on the GPU.

Imports: the module needs no device, but it imports the package (which loads the host library) and, for the scenes and ray
batches the issue tells it to share, the gpu-marked modules tests/test_gpu_update_spheres.py and tests/test_gpu_superset.py; those
must stay importable on a machine without a GPU (they are: their imports touch no device), or tests/test_motion_chains_host.py fails.

Hooks for chains with a vocabulary of their own (tests/material_chains.py, tests/adaptive_chains.py): params["size"], an image
other than W x H; Run's shadow, compare and extra_check; Run.rendered(k, listed) for the launches of mrt_render_tiles,
mrt_render_adaptive and mrt_render_budget, which CameraTables.launch judges as it judges a whole frame's; the verdicts of
mrt_set_auto_regroup, read at the next check (or regroup, or scene) and replayed from the positions each update left.  None of them changes what the chains of this module do.

The model is host only.  It holds the spheres, the camera, the (scene, camera) of every frame queued since the last reset, the
guides' staleness, and the temporal state (h0, h1, previous spheres, previous derived camera, dropped / stepped); frames and
counters are the oracle's, guides denoise_ref's, a step and the image temporal_ref's.  Nothing is read back from the library.

The temporal response (mrt_set_temporal_response) is in the model as the header's contract paragraph has it: the setting outlives
mrt_reset, mrt_set_world and mrt_set_camera; a change of `enabled` drops the history, a change of the three numbers alone keeps
it; a dropped history zeroes the H2 the next step reads.  With it on a step is temporal_response_ref's (steps 3 to 4c), whose
fractional lengths the next step, the image and its variance take as they are; a check then holds the fast history H2 too
(mrt_debug_read_temporal_fast), a dropped one's included once a step has brought the pair."""
import ctypes
import itertools
import math

import numpy as np

import camera_list_ref as CL
import camera_mask_ref as CM
import denoise_ref
import myraytracer_amd as M
import refit_ref as R
import regroup_ref as G
import temporal_ref as T
import temporal_response_ref as TR
from common import mismatch_report, to_oracle_spheres
from test_gpu_superset import _rays_for
from test_gpu_update_spheres import DEPTH, H, HASH_LAYOUTS, KEYS, SEED, SPP, W, scene

OK, INVALID_ARG, HIP, NO_SCENE, BAD_SCENE, STATE, STALLED = 0, 1, 3, 4, 5, 7, 9
SUITE_CASES = tuple(range(16))
UPDATE_KINDS = ("jitter", "scatter", "drift", "shrink", "grow", "flip", "tiny", "partial", "ground")
REFUSALS = ("step-after-reset", "step-while-off", "range-past-the-end", "coordinate-too-large", "radius-nan")
VOCABULARY = ("set_world", "update", "regroup", "set_regroup_block", "set_camera", "render", "reset", "set_frames_in_flight",
              "set_frame_batching", "set_sweep", "set_camera_masks", "set_temporal", "temporal_step", "temporal_reset", "refused", "check")
LIMIT = 1.0e7                                  # mrt_update_spheres: |coordinate|, |radius| <= 1e7
DRIFT_DIR = np.array([0.6, 0.1, 0.79]) / np.linalg.norm([0.6, 0.1, 0.79])
GENERATION_CALLS = ("set_world", "update_spheres", "regroup_spheres", "set_camera")
# case -> (layout, flavour).  masks: frame batching off, 4 or 8 frames in flight, generation changes with two frames between them
# and with none; temporal: max_framebuffer_weight 0, a step per frame; world: mrt_set_world to another sphere count while temporal
# reprojection is on; drift: ends fifty scene sizes away, in a few jumps; long drift: the one chain beyond forty ops, fifty-two drifts of
# ONE scene size each with frames and checks at the positions between; shrink: three shrinks in a row and the tiny radii;
# lists: a masks flavour that asks for the camera-ray sphere lists (mrt_debug_set_camera_masks(2)) right behind mrt_set_world and
# whose seg_masks switches between no table, the masks and the lists on one built generation (0, 3, 2 in a seeded order)
PLAN = {0: ("small", "masks"), 1: ("small", "masks"), 2: ("small", "masks drift"), 3: ("small", "masks shrink"),
        4: ("small", "temporal"), 5: ("small", "temporal world"), 6: ("large-quad", "shrink"), 7: ("large-quad", "temporal world"),
        8: ("large-quad", "long drift"), 9: ("large-lin", "temporal world"), 10: ("large-lin", "shrink drift"), 11: ("deep-4200", "mixed"),
        12: ("small", "lists"), 13: ("small", "lists drift"), 14: ("small", "lists shrink"), 15: ("small", "lists temporal")}
DRIFT_STEPS = (1, 3, 8, 8, 16, 16)             # 52 scene sizes


class Refused(Exception):
    def __init__(self, status, where):
        super().__init__(f"{where}: status {status}")
        self.status = status


class ChainMismatch(AssertionError):
    pass


class ChainStopped(RuntimeError):
    """A status that is no comparison failure (a HIP error, a stalled wait): nothing more may run on the GPU."""


# ------------------------------------------------------------------ the geometry an op names

def layout_scene(layout):
    return scene(M, HASH_LAYOUTS[layout][0])


class Shadow:
    """The spheres and the camera as the calls so far have left them (no oracle, no device): what an op means."""

    def __init__(self):
        self.layout = self.sc = self.cam = None
        self.grown = 0

    @property
    def n(self):
        return len(self.sc)

    def xyzr(self):
        return R.xyzr_of(self.sc)

    def centroid(self):
        return self.sc["center"][:self.n - 1].astype(np.float64).mean(0)

    def ground_top(self):
        return float(self.sc["center"][self.n - 1, 1]) + abs(float(self.sc["radius"][self.n - 1]))

    def load(self, layout):
        self.layout, self.sc, self.grown = layout, layout_scene(layout), 0
        c = self.sc["center"][:self.n - 1].astype(np.float64)
        self.ext0 = c.max(0) - c.min(0)
        self.size = float(self.ext0.max())
        self.origin0 = self.centroid()
        self.rmin0 = float(np.abs(self.sc["radius"][:self.n - 1]).min())

    def camera_at(self, angle, distance, height):
        """a look-at camera `height` above the higher of the centroid and the ground's top, looking at the centroid"""
        c = self.centroid()
        f32 = lambda v: tuple(float(np.float32(x)) for x in v)
        return (f32((c[0] + distance * math.sin(angle), max(c[1], self.ground_top()) + height, c[2] + distance * math.cos(angle))), f32(c))

    def camera_stale(self):
        """the camera no longer stands a unit above the ground, or looks more than a quarter of a scene size past the centroid"""
        frm, at = self.cam
        return frm[1] < self.ground_top() + 1.0 or float(np.linalg.norm(np.asarray(at) - self.centroid())) > 0.25 * self.size

    def drifted(self):
        """the centroid's distance from the one the scene was built around, in scene sizes"""
        return float(np.linalg.norm(self.centroid() - self.origin0)) / self.size

    def smallest_clustered_radius(self):
        return float(np.abs(self.sc["radius"][:self.n - 1]).min())

    def motion(self, kind, seed, k=1):
        """-> [(first, (count, 4) float32)]: the updates of ("update", kind, seed, k) from the spheres as they are"""
        rng = np.random.default_rng(seed)
        n, x = self.n, self.xyzr()
        third = (n - 1) // 3
        size = np.float32(self.size)
        if kind == "jitter":                    # 1 % of the scene's size, the ground included
            x[:, :3] += rng.uniform(-0.01, 0.01, (n, 3)).astype(np.float32) * size
            return [(0, x)]
        if kind == "scatter":                   # anywhere in a box twice the build's size around the middle: the groups stop meaning anything
            c = x[:n - 1, :3].astype(np.float64)
            mid = 0.5 * (c.min(0) + c.max(0))
            x[:n - 1, :3] = rng.uniform(mid - self.ext0, mid + self.ext0, (n - 1, 3)).astype(np.float32)
            top = rng.uniform(mid - self.ext0, mid + self.ext0 * [1.0, 0.0, 1.0])      # (the ground's top: the box's lower half)
            x[n - 1, :3] = (top - [0.0, abs(float(x[n - 1, 3])), 0.0]).astype(np.float32)
            return [(0, x)]
        if kind == "drift":
            x[:, :3] = (x[:, :3].astype(np.float64) + k * self.size * DRIFT_DIR).astype(np.float32)
            return [(0, x)]
        if kind == "shrink":                    # always the first third: three in a row reach 1e-3 of the build's radii
            x[:third, 3] *= np.float32(0.1)
            return [(0, x[:third].copy())]
        if kind == "grow":
            x[third:2 * third, 3] *= np.float32(3.0)
            return [(third, x[third:2 * third].copy())]
        if kind == "flip":
            glass = np.nonzero(self.sc["material_ty"][:n - 1] == 3)[0]
            i = int(glass[rng.integers(0, len(glass))])
            x[i, 3] = -x[i, 3]
            return [(i, x[i:i + 1].copy())]
        if kind == "tiny":                      # legal radii that quad_kc_for_radius clamps; two one-sphere updates
            i, j = (int(v) for v in 2 * third + rng.choice(n - 1 - 2 * third, 2, replace=False))
            x[i, 3], x[j, 3] = 0.0, 1e-30
            return [(i, x[i:i + 1].copy()), (j, x[j:j + 1].copy())]
        if kind == "partial":
            form = seed % 3                     # 0: ends at the last sphere, 1: one sphere, 2: anywhere
            count = 1 if form == 1 else int(rng.integers(2, max(3, n // 2)))
            first = n - count if form == 0 else int(rng.integers(0, n - count))
            x[first:first + count, :3] += rng.uniform(-0.05, 0.05, (count, 3)).astype(np.float32) * size
            return [(first, x[first:first + count].copy())]
        if kind == "ground":                    # the direct sphere: a step aside, a little down or up, the radius 1000 <-> 1001 under the same top
            r = abs(float(x[n - 1, 3]))
            r2 = 1001.0 if r == 1000.0 else 1000.0
            step = rng.uniform([-1.0, -0.3, -1.0], [1.0, 0.1, 1.0])
            x[n - 1, :3] = (x[n - 1, :3].astype(np.float64) + step - [0.0, r2 - r, 0.0]).astype(np.float32)
            x[n - 1, 3] = r2
            return [(n - 1, x[n - 1:n].copy())]
        raise KeyError(kind)

    def apply_update(self, first, arr):
        self.sc["center"][first:first + len(arr)] = arr[:, :3]
        self.sc["radius"][first:first + len(arr)] = arr[:, 3]

    def camera_call(self):
        frm, at = self.cam
        return ("set_camera", (M.Camera(1, frm, at, (0.0, 1.0, 0.0), 40.0, 0.0, 10.0),))

    def calls(self, op):
        """the op as [(method, args)] of State / Model, the shadow moved on by what the legal ones do"""
        name, a = op[0], op[1:]
        if name == "set_world":
            self.load(a[0])
            self.cam = self.camera_at(0.0, 13.0, 2.5)
            return [("debug_set_hierarchy", HASH_LAYOUTS[a[0]][1] or (4, 0)), ("set_world", (self.sc.copy(),)), self.camera_call()]
        if name == "update":
            out = []
            for first, arr in self.motion(*a):
                self.apply_update(first, arr)
                out.append(("update_spheres", (first, arr)))
            if a[0] == "grow":
                self.grown += 1
            if a[0] == "drift":
                shift = a[2] * self.size * DRIFT_DIR
                frm, at = self.cam
                f32 = lambda v: tuple(float(np.float32(x)) for x in v)
                self.cam = (f32(np.asarray(frm) + shift), f32(np.asarray(at) + shift))
                out.append(self.camera_call())
            return out
        if name == "set_camera":
            self.cam = self.camera_at(*a)
            return [self.camera_call()]
        if name == "refused":
            kind, seed = a
            x = self.xyzr()
            if kind in ("step-after-reset", "step-while-off"):
                return [("temporal_step", ())]
            if kind == "range-past-the-end":
                return [("update_spheres", (self.n - 2, x[:4].copy()))]
            bad = x[5:9].copy()
            if kind == "coordinate-too-large":
                bad[2, seed % 3] = 1.5e7
            else:
                bad[1, 3] = np.nan
            return [("update_spheres", (5, bad))]
        simple = {"regroup": "regroup_spheres", "set_regroup_block": "debug_set_regroup_block", "render": "render", "reset": "reset",
                  "set_frames_in_flight": "debug_set_frames_in_flight", "set_frame_batching": "debug_set_frame_batching",
                  "set_sweep": "debug_set_sweep", "set_camera_masks": "debug_set_camera_masks", "set_temporal": "set_temporal",
                  "temporal_step": "temporal_step", "temporal_reset": "temporal_reset", "get_temporal_response": "temporal_response"}
        if name == "temporal_response":
            return [("set_temporal_response", dict(enabled=a[0], fast_history=a[1], clamp_sigma=a[2], antilag=a[3]))]
        return [(simple[name], a)] if name != "check" else []


# ------------------------------------------------------------------ the generator

def chain(case: int):
    """-> (params, ops): params = dict(layout, flavour, max_w); ops = the case's list of tuples"""
    rng = np.random.default_rng(case)
    layout, flavour = PLAN[case % len(PLAN)]
    p = dict(layout=layout, flavour=flavour, max_w=0.0 if "temporal" in flavour else 1.0)
    lists = "lists" in flavour
    flavour = flavour.replace("lists", "masks")     # (a lists flavour is the masks flavour of the same name, but for `lists` below)
    temporal, masks = "temporal" in flavour, "masks" in flavour
    sh = Shadow()
    ops = []
    g = dict(frames=0, temporal=False, updates=0, owed=False)
    chance = lambda q: bool(rng.random() < q)
    seed = lambda: int(rng.integers(0, 2 ** 31))

    def emit(*op):
        if op[0] in ("regroup", "set_world") and g["owed"]:
            emit("check")                       # a check follows every regroup before the grouping changes again
        if op == ("check",) and ops[-1] == op:
            return
        ops.append(op)
        sh.calls(op)
        assert sh.sc is None or max(float(np.abs(sh.xyzr()).max()), float(np.abs(sh.cam[0]).max())) <= 0.5 * LIMIT     # the 1e7 rule
        if op[0] == "check":
            g.update(updates=0, owed=False)
        elif op[0] == "regroup":
            g["owed"] = True
        elif op[0] == "render":
            g["frames"] += op[1]
        elif op[0] == "reset":
            g["frames"] = 0
        elif op[0] == "set_temporal":
            g["temporal"] = op[1]
        elif op[0] == "update":
            g["updates"] += 1
            if sh.camera_stale():
                emit("set_camera", float(rng.uniform(-0.5, 0.5)), float(rng.uniform(11.0, 15.0)), float(rng.uniform(2.0, 3.0)))
            if g["updates"] >= 3:
                emit("check")                   # ... and every third update

    def update(kind, k=None):
        if kind == "grow" and sh.grown >= 1:    # (once a scene: a second x 3 would hide the sky)
            kind = "jitter"
        emit("update", kind, seed(), *(() if k is None else (k,)))

    def frame(k=1):
        if g["temporal"] and g["frames"] and chance(0.2):
            emit("reset")                       # (a caller who resets before every step's frames: the history stays)
        emit("render", k)
        if g["temporal"]:
            emit("temporal_step")

    def animate(kinds):
        for kind in kinds:
            update(kind)
            frame(int(rng.integers(1, 4)) if not g["temporal"] else 1)

    # -- the segments a flavour is made of
    def seg_regroup_then_partial():             # a partial update through a permuted member_index, queued right behind the regroup
        update("scatter" if chance(0.6) else "jitter")
        emit("regroup")
        update("partial")
        emit("check")
        frame()

    def seg_two_regroups():                     # update, regroup, update, regroup
        update(str(rng.choice(["scatter", "jitter", "partial"])))
        emit("regroup")
        emit("check")                           # the regrouped hierarchy itself, before a refit rewrites it
        update(str(rng.choice(["scatter", "partial", "flip"])))
        emit("regroup")
        emit("check")
        frame()

    def seg_masks():                            # generation changes of all three kinds, two frames between some and none between others
        if g["updates"]:
            emit("check")                       # (so that no check of the every-third-update rule drains the frames in flight below)
        emit("set_frames_in_flight", int(rng.choice([4, 8])))
        kinds = ["update", "regroup", "camera", "update"]
        rng.shuffle(kinds)
        for i, kind in enumerate(kinds):
            if kind == "update":
                update(str(rng.choice(["jitter", "partial", "flip"])))
            elif kind == "regroup":
                emit("regroup")
            else:
                emit("set_camera", float(rng.uniform(-0.4, 0.4)), float(rng.uniform(11.0, 15.0)), float(rng.uniform(2.0, 3.0)))
            if i % 2 == 0 or i == len(kinds) - 1:
                emit("render", 2 if chance(0.5) else 3)
                if g["temporal"]:               # (lists temporal: a step behind the frames of every generation that got a table)
                    emit("temporal_step")
            elif chance(0.5):
                emit("render", 1)
        if chance(0.5):                         # a built table left unused for a launch, then used again
            if lists:                           # ... no table, the masks and the lists on one built generation, ending on the lists
                modes = [0, 3]
                rng.shuffle(modes)
                for mode in modes + [2]:
                    emit("set_camera_masks", mode)
                    emit("render", 1)
            else:
                emit("set_camera_masks", False)
                emit("render", 1)
                emit("set_camera_masks", True)
                emit("render", 1)
        emit("check")

    def seg_drift(steps):
        for i, k in enumerate(steps):
            update("drift", int(k))
            if i % 2 == 0 or g["temporal"]:
                frame()

    def seg_shrink():
        for _ in range(3):
            update("shrink")
            if chance(0.5):
                frame()
        update("tiny")
        frame()
        emit("check")

    def seg_other_world():                      # another sphere count; with temporal reprojection on this re-creates "previous"
        other = [l for l in ("small", "large-quad", "large-lin") if len(layout_scene(l)) != sh.n]
        emit("set_world", str(rng.choice(other)))
        frame()
        animate(["jitter"])
        emit("check")

    def seg_switches():                         # (by case number: every value turns up somewhere in the suite)
        emit("set_sweep", case % 3)
        if case % 3 != 2 and not masks:         # (the mask chains switch them off for a launch or two, seg_masks)
            emit("set_camera_masks", bool(case % 2))
        if not masks:
            emit("set_frames_in_flight", (0, 1, 4, 8)[case % 4])
        emit("set_regroup_block", (4, 0)[(case // 2) % 2])

    def seg_reset():
        emit("reset")
        if chance(0.5):
            emit("check")
        frame(int(rng.integers(1, 3)) if not g["temporal"] else 1)

    def seg_refusal():
        kinds = [k for k in REFUSALS if k != "step-after-reset" or g["temporal"]]
        kinds = [k for k in kinds if k != "step-while-off" or not g["temporal"]]
        kind = kinds[case % len(kinds)]
        if kind == "step-after-reset":
            emit("reset")
        emit("refused", kind, seed())
        emit("check")                           # the refused call changed nothing
        if kind == "step-after-reset":
            frame()

    def seg_temporal_toggles():
        which = case % 3
        if which == 0:
            emit("temporal_reset")
            emit("check")                       # dropped: the read refuses
        elif which == 1:
            emit("set_temporal", False)
            emit("set_temporal", True)
        else:
            emit("temporal_reset")
        frame()
        animate(["ground"] if chance(0.5) else ["jitter"])

    def seg_pan():                              # the camera turns a little between two steps: "previous camera" is the last step's
        frm, at = sh.cam
        angle = math.atan2(frm[0] - at[0], frm[2] - at[2]) + float(rng.uniform(-0.06, 0.06))
        emit("set_camera", angle, float(np.hypot(frm[0] - at[0], frm[2] - at[2])), 2.5)
        frame()
        animate(["jitter"])
        emit("check")

    emit("set_world", layout)
    if lists:
        emit("set_camera_masks", 2)
    if masks:
        emit("set_frame_batching", 0)
    if temporal:
        emit("set_temporal", True)
    frame(1 if temporal else 2)
    seg_switches()                              # (first: they hold for the chain)
    body = [seg_refusal]
    if masks:
        body += [seg_masks, seg_masks] if flavour == "masks" else [seg_masks]
    if temporal:                                # (the list chains' seg_masks steps too and toggles for longer: two segments less keep them to forty ops)
        body += [seg_temporal_toggles] if lists else [seg_pan, seg_temporal_toggles, seg_regroup_then_partial]
        if flavour == "temporal":
            body.append(lambda: seg_drift([2]))
    if flavour == "long drift":
        body += [lambda: seg_drift([1] * 26), lambda: seg_drift([1] * 26)]
    elif "drift" in flavour:
        steps = list(DRIFT_STEPS)
        rng.shuffle(steps)
        body += [lambda: seg_drift(steps[:3]), lambda: seg_drift(steps[3:])]
    if "shrink" in flavour:
        body.append(seg_shrink)
    if flavour in ("shrink", "long drift", "mixed", "masks"):
        body += [seg_two_regroups] if masks else [seg_two_regroups, seg_reset]
    if flavour in ("shrink", "mixed", "masks drift", "shrink drift") and not (lists and "drift" in flavour):
        body.append(seg_regroup_then_partial)
    if flavour in ("mixed", "long drift", "masks shrink"):
        body.append(lambda: animate(["grow", "scatter", "ground"]))
    body = [body[int(i)] for i in rng.permutation(len(body))]
    if "world" in flavour:                      # (in the later half: both scenes get their share of the chain)
        body.insert(int(rng.integers(len(body) // 2 + 1, len(body) + 1)), seg_other_world)
    for seg in body:
        seg()
    if ops[-1] != ("check",):
        emit("check")
    return p, ops


# ------------------------------------------------------------------ the model

_FRAMES, _GUIDES, _HITS = {}, {}, {}


def _key(a) -> int:
    return hash(np.ascontiguousarray(a).tobytes())


def _cached(cache, key, make, limit=4000):
    if key not in cache:
        if len(cache) > limit:
            cache.clear()
        cache[key] = make()
    return cache[key]


class Model:
    """State's method names for the chain vocabulary; a call the header refuses raises Refused(status).  The methods the seeded
    defects of tests/test_motion_chains_host.py override are the ones with a leading underscore."""

    def __init__(self, O, max_w, w=W, h=H):
        self.O, self.max_w, self.w, self.h = O, max_w, w, h     # (w, h: the image; tests/adaptive_chains.py has chains at 44 x 20)
        self.spheres = None
        self.set_camera(None)
        self.seeds = O.fill_seeds(SEED, w, h)
        self.frames, self.done = [], []         # per frame queued since the reset: (spheres, cam_raw, key); (fb, counters) after it
        self.guides_built = None                # the (scene, camera) the guides were last rebuilt for
        self.guides_stale = True
        self.temporal_on, self.stepped, self.cleared = False, False, True
        self.h0 = self.h1 = self.prev_xyzr = self.prev_cam = None
        self.found = []                         # per step: (first since a drop, pixels that found history, pixels)
        # the temporal response (mrt_set_temporal_response): the setting, the fast history H2, and whether a step with the
        # response on has brought the H2 pair since temporal reprojection was enabled (the diagnostic's refusal is defined then)
        self.response = dict(enabled=False, **{k: (v if k == "fast_history" else float(np.float32(v))) for k, v in TR.R_DEFAULTS.items()})
        self.h2, self.h2_brought = None, False
        self.response_steps = []                # per step with the response on: (pixels the clamp moved, fractional lengths stored)

    # ---- what the seeded defects change
    def _after_update(self):
        self.guides_stale = True

    def _after_set_world(self):
        self._drop_history()

    def _after_reset(self):
        pass

    def _refused_update(self, first, arr):
        pass

    def _queue_frame(self):
        self.frames.append((self.spheres, self.cam_raw, (_key(self.spheres), self.cam_key)))

    # ---- helpers
    def xyzr(self):
        return R.xyzr_of(self.spheres)

    def _drop_history(self):
        self.stepped, self.cleared = False, True

    def _evaluate(self):
        O, W, H = self.O, self.w, self.h
        for f in range(len(self.done), len(self.frames)):
            spheres, cam_raw, key = self.frames[f]
            fb, cnt = self.done[f - 1] if f else (np.zeros((H, W, 4), np.float32), (0, 0, 0))

            def make():
                c = O.Counters()
                out = O.render_frame(W, H, SPP, DEPTH, O.pack_world(to_oracle_spheres(O, spheres)), cam_raw, self.seeds,
                                     O.frame_shuffle(SEED, f), O.frame_weight(f, self.max_w), fb, counters=c)
                return out, tuple(int(c.as_dict()[k]) for k in KEYS)
            out, add = _cached(_FRAMES, (key, f, self.max_w, _key(fb), W, H), make)
            self.done.append((out, tuple(a + b for a, b in zip(cnt, add))))

    def _guides(self, key):
        spheres, cam_raw = key[2], key[3]
        W, H = self.w, self.h

        def make():
            rays = denoise_ref.centre_rays(W, H, cam_raw)
            hit, t, normal, albedo = denoise_ref.expected_guides(self.O, spheres, rays)
            return {"rays": rays, "index": hit.reshape(H, W).astype(np.int32), "t": t.reshape(H, W), "normal": normal.reshape(H, W, 3),
                    "albedo": albedo.reshape(H, W, 3)}
        return _cached(_GUIDES, key[:2] + (W, H), make, 400)

    def _ensure_guides(self):
        if self.guides_stale or self.guides_built is None:
            self.guides_built = (_key(self.spheres), self.cam_key, self.spheres, self.cam_raw)
            self.guides_stale = False
        return self._guides(self.guides_built)

    def _step_guides(self):
        """the guides a temporal step reads, rebuilt first if stale (a hook: tests/adaptive_chains.py names its consumers)"""
        return self._ensure_guides()

    # ---- scene
    def debug_set_hierarchy(self, levels, target):
        pass

    def set_world(self, spheres):
        self.spheres = np.array(spheres, copy=True)
        self.guides_stale = True
        self.prev_xyzr = self.xyzr()            # "previous" is created anew: the scene's own to begin with
        self._after_set_world()

    def update_spheres(self, first, xyzr):
        arr = np.ascontiguousarray(xyzr, np.float32).reshape(-1, 4)
        if self.spheres is None:
            raise Refused(NO_SCENE, "update_spheres")
        status = OK
        if first + len(arr) > len(self.spheres):
            status = INVALID_ARG
        elif not (np.isfinite(arr) & (np.abs(arr) <= LIMIT)).all():
            status = BAD_SCENE
        if status:
            self._refused_update(first, arr)
            raise Refused(status, "update_spheres")
        if len(arr) == 0:
            return
        self._write(first, arr)
        self._after_update()

    def _write(self, first, arr):
        sc = self.spheres.copy()
        sc["center"][first:first + len(arr)] = arr[:, :3]
        sc["radius"][first:first + len(arr)] = arr[:, 3]
        self.spheres = sc

    def regroup_spheres(self):
        if self.spheres is None:
            raise Refused(NO_SCENE, "regroup_spheres")

    def set_camera(self, cam):
        O = self.O
        self.cam = O.pinhole_camera() if cam is None else O.lookat_camera(cam.lookfrom, cam.lookat, cam.vup, cam.vfov_deg,
                                                                            cam.defocus_angle_deg, cam.focus_dist)
        self.cam_raw = O.camera_derive(self.cam)
        self.cam_key = hash(bytes(self.cam_raw))
        self.guides_stale = True

    # ---- frames
    def render(self, frames=1):
        for _ in range(frames):
            if self.spheres is None:
                raise Refused(NO_SCENE, "render")
            self._queue_frame()

    def reset(self):
        self.frames, self.done = [], []
        self._after_reset()

    @property
    def frames_done(self):
        return len(self.frames)

    def read_framebuffer(self):
        self._evaluate()
        return self.done[-1][0].copy() if self.done else np.zeros((self.h, self.w, 4), np.float32)

    def read_counters(self):
        self._evaluate()
        return dict(zip(KEYS, self.done[-1][1] if self.done else (0, 0, 0)))

    def debug_read_guides(self):
        if self.spheres is None:
            raise Refused(NO_SCENE, "debug_read_guides")
        return {k: v.copy() for k, v in self._ensure_guides().items()}

    # ---- switches that change no output
    def debug_set_frames_in_flight(self, slots):
        pass

    def debug_set_frame_batching(self, enabled):
        pass

    def debug_set_sweep(self, mode):
        pass

    def debug_set_camera_masks(self, on):
        pass

    def debug_set_regroup_block(self, clusters):
        pass

    # ---- temporal reprojection
    def set_temporal(self, enabled):
        if not enabled and self.temporal_on:
            self._drop_history()
            self.h2_brought = False             # (the H2 pair is freed with the history's buffers)
        self.temporal_on = bool(enabled)

    # ---- the temporal response: the header's contract paragraph.  mrt_reset, mrt_set_world*, mrt_set_camera keep the setting
    #      (nothing here touches self.response but set_temporal_response itself)
    def set_temporal_response(self, enabled, fast_history=None, clamp_sigma=None, antilag=None, reserved=0):
        new = dict(self.response, enabled=bool(enabled))
        for k, v in (("fast_history", fast_history), ("clamp_sigma", clamp_sigma), ("antilag", antilag)):
            if v is not None:
                new[k] = int(v) if k == "fast_history" else float(np.float32(v))
        cs, al = new["clamp_sigma"], new["antilag"]
        if (not 1 <= new["fast_history"] <= 16 or not (math.isfinite(cs) and cs > 0) or not 0.0 <= al <= 1.0 or reserved != 0
                or enabled not in (0, 1, False, True)):
            raise Refused(INVALID_ARG, "set_temporal_response")
        if new["enabled"] != self.response["enabled"]:
            self._response_enabled_changed()
        self.response = new                     # (only the three numbers: the history stays, the next step takes them)

    def set_temporal_response_raw(self, enabled, fast_history, clamp_sigma, antilag, reserved):
        """the struct as it is, a reserved word included (the package's wrapper cannot write one)"""
        self.set_temporal_response(enabled, fast_history, clamp_sigma, antilag, reserved)

    def temporal_response(self):
        return self.response["enabled"], {k: v for k, v in self.response.items() if k != "enabled"}

    # what the seeded defects of tests/test_adaptive_chains_host.py change
    def _response_enabled_changed(self):
        self._drop_history()                    # "A call that changes `enabled` drops the history, as mrt_temporal_reset does"

    def _h2_after_drop(self):
        return np.zeros((self.h, self.w, 4), np.float32)        # "a dropped history zeroes the H2 the next step reads"

    def _stored_length(self, h0):
        return h0                               # "The stored length may therefore be fractional"

    def _clamp_indices(self, h1):
        return h1                               # 4b: "... and the index bits of H1'_q equal the pixel's own"

    def _response_step(self, cur, g, now, Mx, o):
        rp = {k: v for k, v in self.response.items() if k != "enabled"}
        h2 = self.h2 if self.h2 is not None else np.zeros((self.h, self.w, 4), np.float32)
        o0, o1, o2, info = TR.reproject(cur, g["rays"], g["index"], g["t"], now, self.prev_xyzr, Mx, o, self.h0, self.h1, h2, None, rp)
        out, cinfo = TR.clamp(o0, self._clamp_indices(o1), o2, rp)
        out = self._stored_length(out)
        self.response_steps.append((int(cinfo["moved"].sum()), int((out[..., 3] != np.floor(out[..., 3])).sum())))
        return out, o1, o2, info

    def _temporal_check(self, where, stepped):
        if not self.temporal_on:
            raise Refused(STATE, where)
        if self.spheres is None:
            raise Refused(NO_SCENE, where)
        if stepped and not self.stepped:
            raise Refused(STATE, where)

    def temporal_step(self):
        self._temporal_check("temporal_step", False)
        if self.frames_done == 0:
            raise Refused(STATE, "temporal_step")
        g = self._step_guides()
        first = self.cleared
        if self.cleared:                        # every length 0: no tap of this step counts, whatever "previous" holds
            self.h0 = np.zeros((self.h, self.w, 4), np.float32)
            self.h1 = np.zeros((self.h, self.w, 4), np.float32)
            self.prev_cam = self.cam_raw
            if self.response["enabled"]:
                self.h2 = self._h2_after_drop()
            self.cleared = False
        Mx, o = T.camera_matrix(self.prev_cam)
        now = self.xyzr()
        if self.response["enabled"]:            # steps 3 and 4 with the fast history, then 4b and 4c
            self.h0, self.h1, self.h2, info = self._response_step(self.read_framebuffer(), g, now, Mx, o)
            self.h2_brought = True
        else:
            self.h0, self.h1, info = T.step(self.read_framebuffer(), g["rays"], g["index"], g["t"], now, self.prev_xyzr, Mx, o, self.h0, self.h1)
        self.prev_xyzr, self.prev_cam, self.stepped = now, self.cam_raw, True
        self.found.append((first, int(info["found"].sum()), info["found"].size))

    def temporal_reset(self):
        if not self.temporal_on:
            raise Refused(STATE, "temporal_reset")
        self._drop_history()

    def read_temporal(self):
        self._temporal_check("read_temporal", True)
        return T.image(self.h0, self.h1, self.read_framebuffer()[..., 3], self._guides(self.guides_built))

    def debug_read_temporal(self, n_spheres):
        self._temporal_check("debug_read_temporal", True)
        return {"h0": self.h0.copy(), "h1": self.h1.copy(), "prev_xyzr": self.prev_xyzr.copy()}

    def debug_read_temporal_fast(self):
        """the H2 the next step reads: a dropped history's reads as zeroes (the runner asks only once a step has brought the pair)"""
        self._temporal_check("debug_read_temporal_fast", False)
        if not self.response["enabled"] or not self.h2_brought:
            raise Refused(STATE, "debug_read_temporal_fast")
        h2 = self._h2_after_drop() if self.cleared else self.h2
        return np.zeros((self.h, self.w, 4), np.float32) if h2 is None else h2.copy()


def new_model(O, params, cls=None):
    return (cls or Model)(O, params["max_w"], *params.get("size", ()))      # ("size": a chain's own image, (w, h); else W x H)


def new_state(params):
    """a context for a chain; a HIP error or a stalled wait while it is made is ChainStopped, as in the runner"""
    try:
        w, h = params.get("size", (W, H))
        st = M.State(M.Args(w, h, SPP, DEPTH, params["max_w"]), seed=SEED)
        st.set_wait_timeout(60.0)               # (a stalled wait stops the case with the wait's name long before the suite's own limit)
        st.debug_set_boxes(2)                   # the walk's box tests on (large scenes), as tests/test_gpu_update_spheres.py has them
    except M.MrtError as e:
        if e.status in (HIP, STALLED):
            raise ChainStopped(f"creating a context: {e}")
        raise
    return st


# ------------------------------------------------------------------ which launches get a camera-ray table

class CameraTables:
    """Host model of the library's decision which render launches run with a camera-ray table, and with which of the two
    (frames.cpp, the comment above camera_masks), from the calls alone:

    * mrt_set_world, mrt_update_spheres, mrt_regroup_spheres and mrt_set_camera begin a new generation: what was built is stale.
    * Every frame launch, with or without a table, is "the previous frame" of the next one: a generation has survived a frame
      when the launch before this one was made under it.
    * The switch (mrt_debug_set_camera_masks): 0 no table, 2 the lists, 3 the masks, 1 the library's rule, which reads the
      device (pixels per lane the chip holds): `lists` is None then, open.
    * The tables apply to the small layout and to launches whose texel is the pixel's own (no queue-layer batch).
    * A launch the tables apply to gets one when its slot has built for the generation; else the slot builds first -- at once
      when some slot has built for the generation, or the generation has survived a frame, or the launch's samples per pixel
      (per frame x frames per lane) reach the threshold of the table it gets (96 the lists, 512 the masks) -- and else runs
      without.

    The slot (frame sequence number modulo the frames in flight) decides who builds, not whether the launch gets a table: a
    slot follows "some slot has built" at once.  That is what makes the outcome independent of how many frames the library's
    controller keeps in flight, which follows measured times; the model keeps the slots' records all the same, and the seeded
    defects of tests/test_motion_chains_host.py show that the comparison notices a rule that reads them wrongly."""
    LISTS_ALWAYS_SPP, MASKS_ALWAYS_SPP = 96, 512

    def __init__(self):
        self.mode = 1
        self.gen = 0                            # the calls that made a table stale so far
        self.frame_gen = None                   # the generation the previous frame was launched under
        self.slot_gen = {}                      # slot -> the generation it last built for
        self.built_gen = None                   # the generation some slot has built
        self.seq = 0                            # frames launched

    # ---- what the seeded defects change
    def stale_after(self, call):
        return call in GENERATION_CALLS

    def slot_has_built(self, slot):
        return self.slot_gen.get(slot) == self.gen

    # ----
    def call(self, name):
        if self.stale_after(name):
            self.gen += 1

    def launch(self, applies, slots, spp_lane):
        """one frame launch -> (in_force, lists); lists None: open (mode 1)"""
        slot = self.seq % max(slots, 1)
        self.seq += 1
        survived = self.frame_gen == self.gen
        self.frame_gen = self.gen
        if self.mode == 0 or not applies:
            return False, False
        lists = {1: None, 2: True, 3: False}[self.mode]
        if not self.slot_has_built(slot):
            if self.built_gen != self.gen and not survived:
                if lists is None and self.LISTS_ALWAYS_SPP <= spp_lane < self.MASKS_ALWAYS_SPP:
                    raise NotImplementedError("mode 1 between the two thresholds: the build depends on the device's rule")
                if spp_lane < (self.LISTS_ALWAYS_SPP if lists else self.MASKS_ALWAYS_SPP):
                    return False, False
            self.slot_gen[slot] = self.gen
            self.built_gen = self.gen
        return True, lists


# ------------------------------------------------------------------ applying and comparing

def _raw_response(st, enabled, fast_history, clamp_sigma, antilag, reserved):
    """mrt_set_temporal_response on a real context with the struct written out, a reserved word included"""
    p = M._lib.MrtTemporalResponse()
    st._L.mrt_temporal_response_default(ctypes.byref(p))
    p.enabled, p.fast_history, p.clamp_sigma, p.antilag = int(enabled), fast_history, clamp_sigma, antilag
    p.reserved[len(p.reserved) - 1] = reserved
    st._check(st._L.mrt_set_temporal_response(st._ctx, ctypes.byref(p)), "mrt_set_temporal_response")


def _call(obj, name, args):
    try:
        if name == "set_temporal_response_raw" and not hasattr(obj, name):
            return OK, _raw_response(obj, *args)
        v = getattr(obj, name)
        if isinstance(args, dict):              # (keyword arguments: mrt_set_temporal_response's wrapper takes its numbers by name)
            return OK, v(**args)
        return OK, (v(*args) if callable(v) else v)
    except (Refused, M.MrtError) as e:
        return e.status, None


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:                   # bit for bit; a NaN equals a NaN
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def _describe(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape / type {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    if a.dtype == np.float32 and a.ndim == 3 and a.shape[-1] == 4:
        return mismatch_report(a, b)
    neq = np.argwhere(~((a == b) | ((a != a) & (b != b))))
    return f"{len(neq)} of {a.size} differ; first at {tuple(neq[0])}: {a[tuple(neq[0])]!r} against {b[tuple(neq[0])]!r}"


def _last_error(impl):
    try:
        return impl._L.mrt_last_error(impl._ctx).decode()
    except Exception:
        return ""


def check_rays(spheres, cam_raw, W=W, H=H):
    """the rays of a check: about 2,000 random, grazing and on-surface rays around the spheres as they are, and the camera's own
    (every texel's four corner jitters and six random ones, as tests/camera_mask_cases.py samples them); -> (rays, index of the first camera ray, the camera rays' texels)"""
    rays = _rays_for(np.random.default_rng(7), spheres, 500, 900, 600)
    n_tex = CM.local_texels(W, H)
    px, py = CM.texel_pixels(n_tex, W)
    tex = np.nonzero(py < H)[0]
    cam_rays, ray_tex = CM.camera_rays(cam_raw, W, H, tex, px[tex], py[tex], np.random.default_rng(17), 6)
    return np.concatenate([rays, cam_rays], 0), len(rays), ray_tex


def reference_hits(O, spheres, rays):
    """oracle.world_hit_batch of the rays against the spheres: (winner, t, discriminant >= 0, required)"""
    return _cached(_HITS, (_key(spheres), _key(rays)),
                   lambda: O.world_hit_batch(O.pack_world(to_oracle_spheres(O, spheres)), rays), 200)


class Run:
    """One chain on one implementation and one model, op by op.  after(i, op, run): called behind every op that compared equal."""

    def __init__(self, label, params, impl, model, O, stats=None, after=None, device_checks=True, tables=None, shadow=None,
                 compare=None, extra_check=None):
        """The hooks of the chains that bring a vocabulary of their own (tests/adaptive_chains.py): shadow, the Shadow that knows
        their ops; compare(name, got, want) -> None or what differs, asked behind every call that both sides accepted, for the
        calls whose value is an observable; extra_check(run), called in every check behind the comparisons below and ahead of
        the device's."""
        self.label, self.p, self.impl, self.model, self.O = label, params, impl, model, O
        self.tables = (tables or CameraTables)()        # the prediction of every render launch's table
        self.batching, self.tables_lost = 1, False      # mrt_debug_set_frame_batching: automatic until a chain switches it off
        self.device_checks = device_checks      # (off: what the model can say alone -- the liveness test's view of a real context)
        self.stats, self.after = stats if stats is not None else {}, after
        self.sh = shadow or Shadow()
        self.compare, self.extra_check = compare, extra_check
        self.spp = SPP                          # samples per frame and launch (mrt_set_samples_per_frame)
        self.auto_regroup, self.auto_seen = False, 0    # mrt_set_auto_regroup: the policy is on; the regroups it has let run
        self.auto_pending = []                  # ... the positions left by the updates whose verdict has not been read yet
        self.device = getattr(impl, "_ctx", None) is not None
        self.sweep, self.fif, self.gen = 0, 0, 0
        self.midx = self.real = self.n_pool = None
        self.ops = []

    def _bump(self, k, by=1):
        k = (self.sh.layout, k)                 # (per layout: a chain may change its scene)
        self.stats[k] = self.stats.get(k, 0) + by

    def _fail(self, what):
        raise ChainMismatch(f"{self.label}, op {len(self.ops) - 1} {self.ops[-1]!r}: {what}\nops so far: {self.ops!r}")

    def _dev(self, name, *args, **kw):
        """a call on the real context alone (the read-backs and diagnostics of a check): its value.  EVERY call this runner makes
        on an implementation goes through here or through _both: MRT_ERR_HIP or MRT_ERR_STALLED from any of them is ChainStopped,
        never a comparison failure; any other refusal of a diagnostic is a mismatch."""
        try:
            return getattr(self.impl, name)(*args, **kw)
        except M.MrtError as e:
            where = f"{self.label}, op {len(self.ops) - 1} {self.ops[-1]!r}: {name}: status {e.status}: {_last_error(self.impl)}"
            if e.status in (HIP, STALLED):
                raise ChainStopped(f"{where}\nops so far: {self.ops!r}")
            self._fail(f"{name} refused: status {e.status} ({_last_error(self.impl)})")

    def _both(self, name, args=()):
        """the call on both; -> (status, the implementation's value, the model's)"""
        si, got = _call(self.impl, name, args)
        sm, want = _call(self.model, name, args)
        if si in (HIP, STALLED):
            raise ChainStopped(f"{self.label}, op {len(self.ops) - 1} {self.ops[-1]!r}: {name}: status {si}: {_last_error(self.impl)}\n"
                               f"ops so far: {self.ops!r}")
        if si != sm:
            self._fail(f"{name}: status {si} against the model's {sm} ({_last_error(self.impl)})")
        return si, got, want

    def step(self, op):
        self.ops.append(op)
        calls = self.sh.calls(op)
        if op[0] == "render" and self.batching == 0 and self.sh.layout == "small":
            # frame batching off: mrt_render(k) is k launches, queued without a wait.  The runner makes them one call each, which
            # queues the same launches, so that EVERY launch's table is compared with the prediction and not the last one's alone
            calls = [("render", (1,))] * op[1]
        if op[0] == "subset" and self.batching == 0 and self.sh.layout == "small":
            calls = [("render_tiles", (op[1], 1))] * op[2]      # (the same for the launches of mrt_render_tiles(tiles, k))
        for name, args in calls:
            if name in ("regroup_spheres", "set_world", "set_auto_regroup"):     # (they need, or end, the ordering as it is)
                self._resolve_auto_regroups()
            status, got, want = self._both(name, args)
            if status == OK and self.compare is not None:
                bad = self.compare(name, got, want)
                if bad:
                    self._fail(f"{name}: {bad}")
            if name == "temporal_response" and status == OK and got != want:
                self._fail(f"temporal_response: {got} against the model's {want}")
            if name == "set_samples_per_frame" and status == OK:
                self.spp = int(args[0])
            if name == "set_auto_regroup" and status == OK:
                self.auto_regroup = bool(args[0])
            if status == OK and name == "set_world":
                self.auto_seen = 0              # (the policy's statistics restart with the scene)
            if status == OK and name == "render_tiles":
                self.rendered(args[1], len(args[0]))
            if status == OK and name == "render_adaptive" and want[1]:
                self.rendered(args[0], want[1])
            if status == OK and name == "render_budget":
                levels = self.model.last_levels  # the mrt_render_tiles calls the allocation was rendered through; the device reports
                for i, (listed, run_length) in enumerate(levels):       # the last launch of the last one
                    self.rendered(run_length, listed, last=i == len(levels) - 1)
            if status == OK and name in GENERATION_CALLS and not (name == "update_spheres" and len(args[1]) == 0):
                self.gen += 1
                self.tables.call(name)
                self._bump("generation changes")
            if status == OK and name == "set_world" and self.device:
                h = self._dev("debug_read_hierarchy")
                self.midx, self.real, self.n_pool = h["midx"], G.real_slots(h), self._dev("debug_regroup_info")["n_pool"]
            if status == OK and name == "regroup_spheres":
                self._bump("regroups")
                if self.device:                 # the ordering tests/regroup_ref.py gives for the geometry at this regroup
                    self.midx = G.regroup(self.midx, self.real, self.n_pool, self.model.xyzr()[:, :3])
            if status == OK and name == "update_spheres" and self.auto_regroup and self.device and len(args[1]):
                # the policy decides on the device and the host never learns the verdict: the positions this update leaves are
                # kept, and the verdicts are read where the runner waits anyway (_resolve_auto_regroups), so that what follows
                # the update still queues behind the frames in flight
                self.auto_pending.append(self.model.xyzr()[:, :3].copy())
            if name == "debug_set_sweep":
                self.sweep = args[0]
            if name == "debug_set_frames_in_flight":
                self.fif = args[0]
            if name == "debug_set_camera_masks" and status == OK:
                self.tables.mode = int(args[0])
            if name == "debug_set_frame_batching":
                self.batching = int(args[0])
            if status == OK and name == "render":
                self.rendered(args[0])
        if op[0] == "check":
            self.check()
            self._bump("checks")
        self._bump("ops")
        self.stats["largest drift"] = max(self.stats.get("largest drift", 0.0), self.sh.drifted())
        self.stats["smallest radius"] = min(self.stats.get("smallest radius", math.inf), self.sh.smallest_clustered_radius())
        if self.after is not None:
            self.after(len(self.ops) - 1, op, self)

    def _resolve_auto_regroups(self):
        """The policy's verdicts on the updates since the last look, read once (mrt_read_regroup_stats waits): how many regroups
        the gate let run, from the statistics; at which of the updates, from the device's member_index -- the ordering is
        replayed (tests/regroup_ref.py, the positions each update left) for every choice of that many updates in order, and the
        one that gives the device's ordering is taken.  None does: the first choice stands, and the check reports member_index."""
        if not self.auto_pending:
            return
        pending, self.auto_pending = self.auto_pending, []
        fired = self._dev("read_regroup_stats")["regroups"] - self.auto_seen
        self.auto_seen += fired
        if not 0 <= fired <= len(pending):
            self._fail(f"the policy reports {fired} regroups behind {len(pending)} updates")
        if fired == 0:
            return
        got = self._dev("debug_read_hierarchy")["midx"]
        replays = []
        for which in itertools.combinations(range(len(pending)), fired):
            midx = self.midx
            for i in which:
                midx = G.regroup(midx, self.real, self.n_pool, pending[i])
            replays.append(midx)
        match = [r for r in replays if np.array_equal(r, got)]
        self.midx = match[0] if match else replays[0]
        self._bump("auto regroups", fired)

    def rendered(self, k, listed=None, last=True):
        """render(k) went through: CameraTables' prediction of its last launch against what the implementation reports.
        listed: the frames were mrt_render_tiles' over that many tiles -- subset launches unless every tile is listed, held to the
        same rule (frames.cpp: the launch covers the list, the table the shard; a subset frame counts as a frame the generation
        survived); the statistics keep them apart ("subset ... launches")."""
        small = self.sh.layout == "small"
        subset = listed is not None and listed < (-(-self.model.w // 8)) * (-(-self.model.h // 8))
        if k > 1 and self.batching != 0 and small:      # (one launch of several frames, in a form the library chooses: the prediction
            self.tables_lost = True             # ends there, for the chain.  On the other layouts no launch gets a table, however
        if self.tables_lost:                    # many launches the frames take)
            return
        for _ in range(k):                      # (0 frames in flight: the library's choice, two or more -- see CameraTables on the slots)
            want = self.tables.launch(small, self.fif or 2, self.spp)
        if not small or not last:               # (last False: more launches of the same call follow)
            return
        pre = "subset " if subset else ""
        self.stats.setdefault(pre + "predicted launches", []).append((self.gen, want[0], want[1], self.fif))
        if not hasattr(self.impl, "debug_read_camera_masks"):
            return
        info = self._dev("debug_read_camera_masks", table=False)       # (host only: no wait)
        self.stats.setdefault(pre + "mask launches", []).append((self.gen, info["in_force"], self.fif))
        self.stats.setdefault(pre + "list launches", []).append((self.gen, info["lists"], self.fif))
        if info["in_force"] != want[0] or (want[1] is not None and info["lists"] != want[1]):
            self._fail(f"the last launch of render({k}) ran with (a table, the lists) = {(info['in_force'], info['lists'])}, the calls say "
                       f"{want} (switch {self.tables.mode}, generation {self.gen}, {self.fif} frames in flight)")

    def check(self):
        m = self.model
        self._resolve_auto_regroups()
        for name in ("frames_done", "read_framebuffer", "read_counters"):
            _, got, want = self._both(name)
            if name == "read_counters":
                got, want = {k: got[k] for k in KEYS}, {k: want[k] for k in KEYS}
                if got != want:
                    self._fail(f"counters {got} against {want}")
            elif name == "frames_done":
                if got != want:
                    self._fail(f"frames_done {got} against {want}")
            elif not _same(got, want):
                self._fail("framebuffer: " + _describe(got, want))
        status, got, want = self._both("debug_read_guides")
        if status != OK and not (status == STATE and getattr(getattr(m, "acc", None), "diverged", False)):
            self._fail(f"debug_read_guides: both refuse with status {status}")     # (the one refusal a check may meet: a diverged
        for k in ("rays", "index", "t", "normal", "albedo") if status == OK else ():        # accumulation without the per-tile denoise)
            if not _same(got[k], want[k]):
                self._fail(f"guide {k}: " + _describe(got[k], want[k]))
        if m.temporal_on:
            status, got, want = self._both("read_temporal")         # dropped: both refuse with MRT_ERR_STATE
            if status == OK:
                if not _same(got, want):
                    self._fail("temporal image: " + _describe(got, want))
                _, got, want = self._both("debug_read_temporal", (len(m.spheres),))
                for k in ("h0", "h1", "prev_xyzr"):
                    if not _same(got[k], want[k]):
                        self._fail(f"temporal {k}: " + _describe(got[k], want[k]))
            # the fast history the next step reads, stepped or dropped (a dropped one reads as zeroes): asked wherever a step
            # with the response on has brought the H2 pair, which is where the diagnostic's answer is defined
            if m.response["enabled"] and m.h2_brought and m.spheres is not None:
                status, got, want = self._both("debug_read_temporal_fast")
                if status != OK:
                    self._fail(f"debug_read_temporal_fast: both refuse with status {status}")
                if not _same(got, want):
                    self._fail("temporal h2: " + _describe(got, want))
                self.stats["h2 checks"] = self.stats.get("h2 checks", 0) + 1
                self.stats["h2 checks of a dropped history"] = self.stats.get("h2 checks of a dropped history", 0) + bool(m.cleared)
        if self.extra_check is not None:
            self.extra_check(self)
        if self.device and self.device_checks:
            self.check_device()

    def check_device(self):
        m, O = self.model, self.O
        xyzr = m.xyzr()
        h = self._dev("debug_read_hierarchy")
        full = dict(h)
        if h["axes"] != (1.0, 1.0, 1.0):        # (the checker's operand and reach are statements about D = I)
            del h["mfma"], h["reach"]
        try:
            R.check(h, xyzr)
        except AssertionError as e:
            self._fail(f"hierarchy: {e}")
        bad = np.nonzero(h["midx"] != self.midx)[0]
        if len(bad):
            self._fail(f"member_index: {len(bad)} slots differ from the reference's grouping; first: slot {bad[0]} holds {h['midx'][bad[0]]}, want {self.midx[bad[0]]}")
        rays, first_cam, ray_tex = check_rays(m.spheres, m.cam_raw, m.w, m.h)
        a2 = (rays[:, 3:].astype(np.float64) ** 2).sum(1)
        if not (np.abs(a2 - 1.0) < 5e-6).all():
            self._fail(f"{int((np.abs(a2 - 1.0) >= 5e-6).sum())} rays are not of unit length")
        ref_hit, ref_t, ref_set, required = reference_hits(O, m.spheres, rays)
        for sweep in (1, 2):
            self._dev("debug_set_sweep", sweep)
            hit, t, cand = self._dev("debug_world_hit", rays, len(m.spheres))
            missing, extra = required & ~cand, cand & ~ref_set
            if missing.any():
                self._fail(f"sweep {sweep}: {int(missing.sum())} (ray, sphere) pairs with a discriminant >= 0 never reached the root tests; "
                           f"first ray {int(np.nonzero(missing.any(1))[0][0])}, sphere {int(np.nonzero(missing.any(0))[0][0])}")
            if extra.any():
                self._fail(f"sweep {sweep}: {int(extra.sum())} pairs reached the root tests with a negative discriminant")
            if not np.array_equal(hit, ref_hit):
                self._fail(f"sweep {sweep}: winners differ on {int((hit != ref_hit).sum())} rays")
            if not np.array_equal(t.view(np.uint32)[hit >= 0], ref_t.view(np.uint32)[hit >= 0]):
                self._fail(f"sweep {sweep}: t differs")
        self._dev("debug_set_sweep", self.sweep)
        if self.sh.layout == "small":
            info = self._dev("debug_read_camera_masks")
            if info["built"]:                   # built for the current generation: it covers what the current camera's rays require
                cluster_of = CM.cluster_of_sphere(full["midx"], len(full["top"]), full["direct_first"], full["nodes"][:full["n_members"]],
                                                  len(m.spheres))
                ri, si = CM.missing_pairs(info["masks"], ray_tex, required[first_cam:], cluster_of)
                self._bump("mask tables checked")
                if len(ri):
                    self._fail(f"camera masks: {len(ri)} required (ray, sphere) pairs lie in a cluster the table's entry does not set")
                self.check_lists(full, ray_tex, required[first_cam:])
        why = self._dev("debug_check_context")
        if why is not None:
            self._fail(f"the context is not sound: {why}")

    def check_lists(self, full, ray_tex, required):
        """the sphere lists of the build the masks came from: tests/camera_list_ref.py's for the hierarchy as the device holds it
        and the model's camera, and on them every (ray, sphere) pair the oracle requires of the check's camera rays"""
        m = self.model
        members, n_top, direct_first = full["nodes"][:full["n_members"]], len(full["top"]), full["direct_first"]
        n_slots = min(4 * n_top, direct_first, len(members))
        words = self._dev("debug_read_camera_lists")
        ref = CL.camera_lists_ref(members, n_top, direct_first, m.cam_raw, m.w, m.h)
        try:
            got, over = CL.unpack(words, n_slots)
        except AssertionError as e:
            self._fail(f"camera lists: an entry is malformed (entry, its slots or count): {e}")
        self._bump("list tables checked")
        if got.shape != ref.shape:
            self._fail(f"camera lists: {got.shape} entries x slots against the reference's {ref.shape}")
        want_over = ref.sum(1) > CL.CAP
        if not np.array_equal(over, want_over):
            bad = np.nonzero(over != want_over)[0]
            self._fail(f"camera lists: the overflow flags of {len(bad)} entries differ from the reference's; first: entry {bad[0]}")
        if not np.array_equal(got[~over], ref[~over]):
            bad = np.argwhere(got != ref)
            bad = bad[~over[bad[:, 0]]]
            self._fail(f"camera lists: {len(bad)} (entry, slot) answers differ from the reference's; first: entry {bad[0][0]}, slot {bad[0][1]}: "
                       f"{got[tuple(bad[0])]} against {ref[tuple(bad[0])]}")
        ri, si = CL.missing_pairs(got, over, ray_tex, required, CL.slot_of_sphere(full["midx"], n_slots, members, len(m.spheres)))
        if len(ri):
            self._fail(f"camera lists: {len(ri)} required (ray, sphere) pairs are not on the list of the ray's entry")


def run(case, impl, model, O, stats=None, after=None, device_checks=True, tables=None):
    """Applies chain `case` to impl and model in lock step; raises ChainMismatch at the first difference."""
    p, ops = chain(case)
    r = Run(f"chain {case}", p, impl, model, O, stats, after, device_checks, tables)
    for op in ops:
        r.step(op)
    return r
