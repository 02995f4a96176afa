"""Chains that mix mrt_update_materials with the calls of tests/motion_chains.py: updates, regroups, camera changes, resets, frames
and temporal steps, about thirty ops each, checked against the host model.

The runner is motion_chains' own: its Run engine, its checks (framebuffer, counters, guides, the temporal history and image, and
on a real context the hierarchy, member_index, the candidate sets, the camera tables and the context's soundness) and its
CameraTables -- whose GENERATION_CALLS do not name update_materials, so every render launch of the small layout is also held to
"a material edit leaves the camera tables built".  motion_chains.run draws its ops from a case number; the chains here are
written out (CHAINS), so run() below feeds them to motion_chains.Run, with a Shadow that knows the one new op:

  ("materials", kind, seed, restart)   MATERIAL_KINDS, from the spheres as they are; restart: MRT_MATERIALS_RESTART_HISTORY
  ("refused_materials",)               a range past the end: MRT_ERR_INVALID_ARG, nothing changed

The model (Model, passed through motion_chains.new_model(..., cls=Model)) writes the material fields of its sphere list, marks
the guides stale and takes no history action without the flag; with it, the radius of "previous" becomes a NaN for the range,
which is all the flag does on the device -- temporal_ref's step then finds no history there, and its snapshot restores it."""
import numpy as np

import motion_chains as MC
import myraytracer_amd as M

F = np.float32
MATERIAL_KINDS = ("recolour", "types", "partial", "ground", "glass-one")


class Shadow(MC.Shadow):
    def materials(self, kind, seed):
        """-> (first, MATERIAL_DTYPE array): the edit `kind` of the spheres as they are"""
        rng = np.random.default_rng(seed)
        n = self.n
        sc = self.sc.copy()
        first, count = 0, n
        if kind == "partial":
            count = int(rng.integers(2, n // 2))
            first = int(rng.integers(0, n - count))
        elif kind == "ground":
            first, count = n - 1, 1
        elif kind == "glass-one":                # "make this one glass"
            first, count = int(rng.integers(0, n - 1)), 1
        idx = np.arange(first, first + count)
        if kind == "types":                      # L -> M -> D -> L, and one sphere that absorbs
            ty = sc["material_ty"][idx]
            sc["material_ty"][idx] = np.where(ty == 1, 2, np.where(ty == 2, 3, 1))
            sc["material_ty"][int(rng.integers(0, n - 1))] = 7
        elif kind == "glass-one":
            sc["material_ty"][idx] = 3
        elif kind == "ground":
            sc["material_ty"][idx] = 2 if sc["material_ty"][n - 1] == 1 else 1
        ty = sc["material_ty"][idx]
        sc["albedo"][idx] = rng.uniform(0.05, 0.95, (count, 3)).astype(F)
        sc["param"][idx] = np.where(ty == 2, rng.uniform(0.0, 0.5, count), np.where(ty == 3, rng.uniform(1.2, 2.0, count), 0.0)).astype(F)
        return first, M.materials_of(sc[first:first + count])

    def calls(self, op):
        if op[0] == "materials":
            _, kind, seed, restart = op
            first, arr = self.materials(kind, seed)
            for k in M.MATERIAL_DTYPE.names:
                self.sc[k][first:first + len(arr)] = arr[k]
            return [("update_materials", (first, arr, restart))]
        if op[0] == "refused_materials":
            return [("update_materials", (self.n - 2, M.materials_of(self.sc[:4]), False))]
        return super().calls(op)


class Model(MC.Model):
    """motion_chains.Model with update_materials; what the seeded defects of tests/test_material_chains_host.py change is
    _after_materials"""

    def update_materials(self, first, materials, restart_history=False):
        arr = M.materials_of(materials)
        if self.spheres is None:
            raise MC.Refused(MC.NO_SCENE, "update_materials")
        if first + len(arr) > len(self.spheres):
            raise MC.Refused(MC.INVALID_ARG, "update_materials")
        if len(arr) == 0:
            return
        sc = self.spheres.copy()
        for k in M.MATERIAL_DTYPE.names:
            sc[k][first:first + len(arr)] = arr[k]
        self.spheres = sc
        self._after_materials(first, len(arr), restart_history)

    def _after_materials(self, first, count, restart_history):
        self.guides_stale = True
        if restart_history:
            prev = self.prev_xyzr.copy()
            prev[first:first + count, 3] = np.nan
            self.prev_xyzr = prev


def _mat(kind, seed, restart=False):
    return ("materials", kind, seed, restart)


_CAM = lambda a, d=13.0, h=2.5: ("set_camera", a, d, h)
_STEP = [("render", 1), ("temporal_step",)]

CHAINS = {
    # frames in flight, frame batching off: every launch's camera table is predicted from the calls, and an edit is no generation
    "small-masks": (dict(layout="small", flavour="materials masks", max_w=1.0), [
        ("set_world", "small"), ("set_frame_batching", 0), ("render", 2), _mat("recolour", 1), ("render", 2),
        ("set_frames_in_flight", 4), ("update", "jitter", 11), _mat("types", 2), ("render", 3), ("check",),
        ("regroup",), _mat("partial", 3), ("update", "partial", 14), ("render", 2), ("check",),
        _CAM(0.2), _mat("ground", 4), ("render", 1), _mat("glass-one", 5), ("render", 2), ("reset",), _mat("partial", 6),
        ("render", 2), ("check",), ("refused_materials",), ("check",), ("update", "scatter", 15), ("regroup",),
        _mat("recolour", 7), ("render", 2), ("check",)]),
    # a history across edits with and without the flag, a check between a flagged edit and its step, a reset, a dropped history
    "small-temporal": (dict(layout="small", flavour="materials temporal", max_w=0.0), [
        ("set_world", "small"), _CAM(0.0, 5.0, 1.5), ("set_temporal", True), *_STEP, _mat("recolour", 21), *_STEP, ("check",),
        _mat("partial", 22, True), *_STEP, ("check",), ("update", "jitter", 31), ("regroup",), _mat("types", 23, True), *_STEP, ("check",),
        _CAM(0.04, 5.0, 1.5), *_STEP, ("reset",), _mat("ground", 24), *_STEP, ("check",),
        _mat("glass-one", 25, True), ("check",), *_STEP, ("check",),
        ("temporal_reset",), _mat("recolour", 26, True), *_STEP, *_STEP, ("check",)]),
    # the large layout: boxes, three levels, regroups in small blocks, a partial move through a permuted member_index
    "large-temporal": (dict(layout="large-quad", flavour="materials temporal", max_w=0.0), [
        ("set_world", "large-quad"), _CAM(0.0, 6.0, 2.0), ("set_regroup_block", 4), ("set_temporal", True), *_STEP,
        _mat("types", 41), *_STEP, ("update", "scatter", 51), ("regroup",), _mat("partial", 42, True), ("update", "partial", 52),
        *_STEP, ("check",), _mat("recolour", 43, True), ("update", "jitter", 53), *_STEP, ("check",),
        ("refused_materials",), ("reset",), _mat("ground", 44, True), *_STEP, _mat("glass-one", 45), ("regroup",), *_STEP,
        ("check",)]),
}
NAMES = tuple(CHAINS)


def new_model(O, name, cls=None):
    return MC.new_model(O, CHAINS[name][0], cls or Model)


def run(name, impl, model, O, stats=None, after=None, device_checks=True):
    """chain `name` on impl and model in lock step (motion_chains.Run); raises ChainMismatch at the first difference"""
    p, ops = CHAINS[name]
    r = MC.Run(f"material chain {name}", p, impl, model, O, stats, after, device_checks)
    r.sh = Shadow()
    for op in ops:
        r.step(op)
    return r
