"""Host-side mirror of the reference's interface for the render path, over the C ABI.

Names follow raytracer/src/lib.rs: `Args` (lib.rs:18-37), the scene description
`Lambertian` / `Metal` / `Sphere` / `World` (the fn-local `api` module, lib.rs:611-639;
`Dielectric` is the extension), and `State` with `redraw()` (lib.rs:206-308).  The
reference's toolchain (Rust) is not in this image, so this mirror is Python over ctypes;
INTEGRATION.md shows the Rust binding of the same ABI.
"""
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import MrtArgs, MrtCamera, MrtCameraRaw, MrtCounters, MrtLocals, MrtMaterial, MrtSphere, MrtWorld

LAMBERTIAN, METAL, DIELECTRIC = 1, 2, 3          # raw::MaterialTy, lib.rs:644-648 (+ extension)
SPHERE_DTYPE = np.dtype([("center", "<f4", 3), ("radius", "<f4"), ("material_ty", "<i4"),
                         ("albedo", "<f4", 3), ("param", "<f4")])
assert SPHERE_DTYPE.itemsize == C.sizeof(MrtSphere) == 36
MATERIAL_DTYPE = np.dtype([("material_ty", "<i4"), ("albedo", "<f4", 3), ("param", "<f4")])     # mrt_material
assert MATERIAL_DTYPE.itemsize == C.sizeof(MrtMaterial) == 20


class MrtError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        name = _lib.load().mrt_status_string(status).decode()
        super().__init__(f"{where}: {name}" + (f" ({detail})" if detail else ""))


@dataclass
class Args:
    """raytracer::Args (lib.rs:18-37), same defaults."""
    width: int = 0
    height: int = 0
    samples_per_frame: int = 1
    ray_depth: int = 50
    max_framebuffer_weight: float = 1.0

    def resolved(self) -> "Args":
        """The size rule of App::resumed (lib.rs:113-134)."""
        a = MrtArgs(self.width, self.height, self.samples_per_frame, self.ray_depth, self.max_framebuffer_weight)
        _lib.load().mrt_args_resolve_size(C.byref(a))
        return Args(a.width, a.height, a.samples_per_frame, a.ray_depth, a.max_framebuffer_weight)

    def _c(self) -> MrtArgs:
        return MrtArgs(self.width, self.height, self.samples_per_frame, self.ray_depth, self.max_framebuffer_weight)


@dataclass
class Lambertian:          # api::Lambertian, lib.rs:613-616
    albedo: Tuple[float, float, float]


@dataclass
class Metal:               # api::Metal, lib.rs:618-622
    albedo: Tuple[float, float, float]
    fuzz: float


@dataclass
class Dielectric:          # extension (material type 3)
    ior: float


@dataclass
class Sphere:              # api::Sphere, lib.rs:630-635
    center: Tuple[float, float, float]
    radius: float
    material: object


@dataclass
class World:               # api::World, lib.rs:637-639
    spheres: List[Sphere] = field(default_factory=list)

    def to_array(self) -> np.ndarray:
        out = np.zeros(len(self.spheres), SPHERE_DTYPE)
        for i, s in enumerate(self.spheres):
            m = s.material
            if isinstance(m, Lambertian):
                out[i] = (s.center, s.radius, LAMBERTIAN, m.albedo, 0.0)
            elif isinstance(m, Metal):
                out[i] = (s.center, s.radius, METAL, m.albedo, m.fuzz)
            elif isinstance(m, Dielectric):
                out[i] = (s.center, s.radius, DIELECTRIC, (1.0, 1.0, 1.0), m.ior)
            else:
                raise TypeError(f"unknown material {m!r}")
        return out


@dataclass
class Camera:
    """mode 0 = the reference's fixed pinhole (shader.wgsl:360-381); mode 1 = look-at thin lens."""
    mode: int = 0
    lookfrom: Sequence[float] = (0.0, 0.0, 0.0)
    lookat: Sequence[float] = (0.0, 0.0, -1.0)
    vup: Sequence[float] = (0.0, 1.0, 0.0)
    vfov_deg: float = 90.0
    defocus_angle_deg: float = 0.0
    focus_dist: float = 1.0

    def _c(self) -> MrtCamera:
        c = MrtCamera()
        c.mode = self.mode
        c.lookfrom[:] = list(self.lookfrom)
        c.lookat[:] = list(self.lookat)
        c.vup[:] = list(self.vup)
        c.vfov_deg, c.defocus_angle_deg, c.focus_dist = self.vfov_deg, self.defocus_angle_deg, self.focus_dist
        return c

    @staticmethod
    def _from_c(c: MrtCamera) -> "Camera":
        return Camera(c.mode, tuple(c.lookfrom), tuple(c.lookat), tuple(c.vup), c.vfov_deg,
                      c.defocus_angle_deg, c.focus_dist)


# ------------------------------------------------------------------ host-only helpers

def pack_world(spheres: np.ndarray):
    """lib.rs:722-799 through mrt_pack_world -> (MrtWorld, vec4[n,4], f32[n], i32[n])."""
    L = _lib.load()
    spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
    n = len(spheres)
    vec4 = np.zeros((2 * n + 1, 4), np.float32)
    f32 = np.zeros(2 * n + 1, np.float32)
    i32 = np.zeros(2 * n + 1, np.int32)
    w = MrtWorld()
    nv, nf, ni = C.c_size_t(), C.c_size_t(), C.c_size_t()
    st = L.mrt_pack_world(spheres.ctypes.data, n, C.byref(w), vec4.ctypes.data, 2 * n + 1, C.byref(nv),
                          f32.ctypes.data, 2 * n + 1, C.byref(nf), i32.ctypes.data, 2 * n + 1, C.byref(ni))
    if st:
        raise MrtError(st, "mrt_pack_world")
    return w, vec4[:nv.value].copy(), f32[:nf.value].copy(), i32[:ni.value].copy()


def materials_of(materials) -> np.ndarray:
    """A contiguous MATERIAL_DTYPE array from one, or from the material fields of a SPHERE_DTYPE array."""
    arr = np.asarray(materials)
    if arr.dtype == SPHERE_DTYPE:
        out = np.zeros(arr.shape, MATERIAL_DTYPE)
        for k in MATERIAL_DTYPE.names:
            out[k] = arr[k]
        arr = out
    elif arr.dtype != MATERIAL_DTYPE:
        raise TypeError(f"materials must be a MATERIAL_DTYPE or SPHERE_DTYPE array, got {arr.dtype}")
    if arr.ndim != 1:
        raise ValueError(f"materials must be one-dimensional, got {arr.shape}")
    return np.ascontiguousarray(arr)


def material_shade(material) -> np.ndarray:
    """mrt_debug_material_shade (host only): floats 4..7 of the shade record of a sphere with this material (one MATERIAL_DTYPE
    record) -- the derivation mrt_set_world_raw and mrt_update_materials share."""
    m = materials_of(np.asarray(material).reshape(1))
    out = np.zeros(4, np.float32)
    st = _lib.load().mrt_debug_material_shade(C.cast(m.ctypes.data, C.POINTER(MrtMaterial)), out.ctypes.data_as(C.POINTER(C.c_float)))
    if st:
        raise MrtError(st, "mrt_debug_material_shade")
    return out


def camera_derive(cam: Camera) -> MrtCameraRaw:
    raw = MrtCameraRaw()
    st = _lib.load().mrt_camera_derive(C.byref(cam._c()), C.byref(raw))
    if st:
        raise MrtError(st, "mrt_camera_derive")
    return raw


def frame_weight(frames_done: int, max_w: float) -> float:
    return float(_lib.load().mrt_frame_weight(frames_done, max_w))


def frame_shuffle(seed: int, frame: int) -> List[int]:
    out = (C.c_uint32 * 4)()
    _lib.load().mrt_frame_shuffle(seed, frame, out)
    return [int(x) for x in out]


def pixel_seed(seed: int, pixel_index: int) -> List[int]:
    out = (C.c_uint32 * 4)()
    _lib.load().mrt_pixel_seed(seed, pixel_index, out)
    return [int(x) for x in out]


def scene_default() -> np.ndarray:
    """The shipped 4-sphere scene (lib.rs:687-720)."""
    out = np.zeros(4, SPHERE_DTYPE)
    n = _lib.load().mrt_scene_default(out.ctypes.data, 4)
    assert n == 4
    return out


def scene_cover(scene_seed: int = 1, dielectric: bool = False):
    out = np.zeros(512, SPHERE_DTYPE)
    cam = MrtCamera()
    n = _lib.load().mrt_scene_cover(scene_seed, int(dielectric), out.ctypes.data, len(out), C.byref(cam))
    if n < 0 or n > len(out):
        raise MrtError(-n if n < 0 else 6, "mrt_scene_cover")
    return out[:n].copy(), Camera._from_c(cam)


def scene_stress(scene_seed: int = 1, n_side: int = 100):
    out = np.zeros(n_side * n_side + 1, SPHERE_DTYPE)
    cam = MrtCamera()
    n = _lib.load().mrt_scene_stress(scene_seed, n_side, out.ctypes.data, len(out), C.byref(cam))
    if n < 0 or n > len(out):
        raise MrtError(-n if n < 0 else 6, "mrt_scene_stress")
    return out[:n].copy(), Camera._from_c(cam)


def save_scene(path: str, spheres, cam: Optional[Camera] = None):
    """Write a scene file (format: include/myraytracer_amd.h, mrt_scene_save).  cam=None writes no camera line."""
    arr = spheres.to_array() if isinstance(spheres, World) else np.ascontiguousarray(spheres, SPHERE_DTYPE)
    c = cam._c() if cam is not None else None
    st = _lib.load().mrt_scene_save(os.fsencode(path), arr.ctypes.data, len(arr), C.byref(c) if c is not None else None)
    if st != 0:
        raise MrtError(st, "mrt_scene_save", _lib.load().mrt_last_error(None).decode())


def load_scene(path: str):
    """Read a scene file -> (spheres, camera or None if the file has no camera line)."""
    L = _lib.load()
    cam, has = MrtCamera(), C.c_int(0)
    n = L.mrt_scene_load(os.fsencode(path), None, 0, C.byref(cam), C.byref(has))
    if n < 0:
        raise MrtError(-n, "mrt_scene_load", L.mrt_last_error(None).decode())
    out = np.zeros(n, SPHERE_DTYPE)
    n2 = L.mrt_scene_load(os.fsencode(path), out.ctypes.data, len(out), C.byref(cam), C.byref(has))
    if n2 != n:
        raise MrtError(-n2 if n2 < 0 else 6, "mrt_scene_load")
    return out, (Camera._from_c(cam) if has.value else None)


def write_image(path: str, rgba: np.ndarray):
    """rgba: (H, W, 4) f32, row 0 = bottom.  .ppm / .png -> 8-bit sRGB (what the reference's surface shows), anything else -> PFM."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w, _ = rgba.shape
    L = _lib.load()
    fn = L.mrt_write_ppm if path.endswith(".ppm") else L.mrt_write_png if path.endswith(".png") else L.mrt_write_pfm
    st = fn(path.encode(), rgba.ctypes.data, w, h)
    if st:
        raise MrtError(st, "write_image", path)


def width_policy(op: int, workload: Sequence[int], state: Sequence[int], util: float = 0.0, rate: float = 0.0):
    """The launch-width controller's policy (csrc/width_policy.h) on synthetic input; host only.  workload = (n_tiles, n_waves,
    max_slots, spp, n_members, counter); state = (div, mult, prev_div, prev_mult, low_windows, settled, prev_rate).  Returns
    the new state (op 0: start, op 1: a window closed) or the launch share (op 2, util = frames still running)."""
    import struct
    L = _lib.load()
    w = (C.c_uint32 * 6)(*[int(x) for x in workload])
    st = list(state) if state is not None else [0, 1, 0, 1, 0, 0, 0.0]
    bits = struct.unpack("<I", struct.pack("<f", float(st[6])))[0]
    sv = (C.c_uint32 * 7)(*[int(x) for x in st[:6]], bits)
    rc = L.mrt_debug_width_policy(op, w, sv, float(util), float(rate))
    if rc:
        raise MrtError(rc, "mrt_debug_width_policy")
    if op == 2:
        return int(sv[0])
    return [int(sv[i]) for i in range(6)] + [struct.unpack("<f", struct.pack("<I", sv[6]))[0]]


WIDTH_DECISION_FIELDS = ("div", "mult", "settled", "frames_in_flight", "frames_running", "launch_div", "window_open", "window_closed",
                         "memo_entries")


def width_replay(workload: Sequence[int], calls: Sequence[dict], hint: Optional[Tuple[int, int]] = None, probe_slots: int = 0):
    """mrt_debug_width_replay: a fresh launch-width controller (csrc/width_policy.h, WidthController) through synthetic frame
    calls; host only.  workload = (n_tiles, n_waves, max_slots, spp, n_members, counter[, n_spheres]); hint = (div, mult) or
    None; probe_slots = what the stream-concurrency probe would report (0: all 16).  Every call is a dict: now (seconds,
    required), running (earlier frames found queued or running, default 0), intervals = (n, sum_ms) of device start-to-start
    times or None, samples = [(frame, hits, slots), ...] that have landed, invalidate (a setter was called before this call),
    and -- from this call on -- workload / hint where they change.  Returns one dict per call: WIDTH_DECISION_FIELDS, util, rate."""
    L = _lib.load()
    n = len(calls)
    words = np.zeros((n, 13), np.uint32)
    times = np.zeros((n, 2), np.float64)
    samples = []
    for i, call in enumerate(calls):
        workload = call.get("workload", workload)
        hint = call["hint"] if "hint" in call else hint
        n_int, sum_ms = call.get("intervals") or (0, 0.0)
        landed = call.get("samples", ())
        w = tuple(workload) + (0,) * (7 - len(workload))
        words[i] = [*w, *(hint or (0, 0)), int(bool(call.get("invalidate"))), call.get("running", 0), n_int, len(landed)]
        times[i] = [call["now"], sum_ms]
        samples += [tuple(s) for s in landed]
    flat = np.ascontiguousarray(np.array(samples, np.uint64).reshape(-1, 3))
    out = np.zeros((n, len(WIDTH_DECISION_FIELDS)), np.uint32)
    measured = np.zeros((n, 2), np.float64)
    rc = L.mrt_debug_width_replay(int(probe_slots), n, words.ctypes.data, times.ctypes.data, flat.ctypes.data if len(samples) else None,
                                  len(samples), out.ctypes.data, measured.ctypes.data)
    if rc:
        raise MrtError(rc, "mrt_debug_width_replay")
    return [dict(zip(WIDTH_DECISION_FIELDS, map(int, out[i])), util=float(measured[i, 0]), rate=float(measured[i, 1])) for i in range(n)]


# ------------------------------------------------------------------ State

class State:
    """The in-scope part of raytracer's `State` (lib.rs:206-308) on one MI355X.

    State(args, seed) ~ State::new; set_world ~ Object::new's upload; redraw() ~
    State::redraw (raytrace pass + swap + weight/shuffle update).
    """

    def __init__(self, args: Args, seed: int = 1, device: int = 0, shard: Optional[Tuple[int, int]] = None,
                 stream: Optional[int] = None):
        self._L = _lib.load()
        self._ctx = C.c_void_p()
        self.args = args.resolved()
        st = self._L.mrt_create(C.byref(args._c()), seed, device, C.byref(self._ctx))
        if st:
            raise MrtError(st, "mrt_create", self._L.mrt_last_error(None).decode())
        if shard is not None:
            self._check(self._L.mrt_set_shard(self._ctx, shard[0], shard[1]), "mrt_set_shard")
        if stream is not None:
            self._check(self._L.mrt_set_stream(self._ctx, stream), "mrt_set_stream")

    def _check(self, st, where):
        if st:
            raise MrtError(st, where, self._L.mrt_last_error(self._ctx).decode())

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.mrt_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- scene
    def set_world(self, world):
        arr = world.to_array() if isinstance(world, World) else np.ascontiguousarray(world, SPHERE_DTYPE)
        self._check(self._L.mrt_set_world(self._ctx, arr.ctypes.data, len(arr)), "mrt_set_world")

    def set_world_raw(self, w, vec4: np.ndarray, f32: np.ndarray, i32: np.ndarray):
        """w: an MrtWorld (80 bytes) or any buffer holding the reference's 64-byte raw::World."""
        wbuf = bytes(w) if not isinstance(w, (bytes, bytearray)) else bytes(w)
        vec4 = np.ascontiguousarray(vec4, np.float32).reshape(-1, 4)
        f32 = np.ascontiguousarray(f32, np.float32)
        i32 = np.ascontiguousarray(i32, np.int32)
        self._check(self._L.mrt_set_world_raw(self._ctx, wbuf, len(wbuf), vec4.ctypes.data, len(vec4), f32.ctypes.data,
                                              len(f32), i32.ctypes.data, len(i32)), "mrt_set_world_raw")

    def update_spheres(self, first: int, xyzr):
        """mrt_update_spheres: new (cx, cy, cz, radius) for spheres first .. first + len(xyzr) - 1 of the current scene -- any
        (count, 4) array; materials and the hierarchy's grouping stay, the derived arrays are refitted on the device in stream
        order and nothing waits for the frames in flight."""
        arr = np.ascontiguousarray(xyzr, np.float32)
        if arr.ndim != 2 or arr.shape[1] != 4:
            raise ValueError(f"update_spheres: xyzr must be (count, 4), got {arr.shape}")
        self._check(self._L.mrt_update_spheres(self._ctx, first, len(arr), arr.ctypes.data if len(arr) else None), "mrt_update_spheres")

    def update_materials(self, first: int, materials, restart_history: bool = False):
        """mrt_update_materials: new materials for spheres first .. first + len(materials) - 1 of the current scene -- a
        MATERIAL_DTYPE array, or a SPHERE_DTYPE array whose material fields are taken; geometry, grouping and the hierarchy stay,
        nothing is refitted and nothing waits for the frames in flight.  restart_history: the next temporal_step finds no history
        for the pixels that show these spheres."""
        arr = materials_of(materials)
        flags = _lib.MATERIALS_RESTART_HISTORY if restart_history else 0
        self._check(self._L.mrt_update_materials(self._ctx, first, len(arr), arr.ctypes.data if len(arr) else None, flags), "mrt_update_materials")

    def regroup_spheres(self):
        """mrt_regroup_spheres: the hierarchy's grouping made anew on the device from the spheres as they are now (after
        update_spheres calls have moved them), refitted in stream order; images do not change, member_tests do."""
        self._check(self._L.mrt_regroup_spheres(self._ctx), "mrt_regroup_spheres")

    def set_auto_regroup(self, enabled: bool = True, ratio: Optional[float] = None, check_every: Optional[int] = None):
        """mrt_set_auto_regroup: have update_spheres judge the hierarchy on the device at every check_every-th call and regroup
        when the sum of R^2 over its nodes exceeds `ratio` x its value after the last regroup; None keeps the current number.
        Off by default; images never depend on it."""
        p = _lib.MrtAutoRegroup()
        self._check(self._L.mrt_get_auto_regroup(self._ctx, C.byref(p)), "mrt_get_auto_regroup")
        p.enabled = int(bool(enabled))
        if ratio is not None:
            p.ratio = ratio
        if check_every is not None:
            p.check_every = check_every
        self._check(self._L.mrt_set_auto_regroup(self._ctx, C.byref(p)), "mrt_set_auto_regroup")

    def get_auto_regroup(self) -> dict:
        """enabled, ratio, check_every (mrt_get_auto_regroup)"""
        p = _lib.MrtAutoRegroup()
        self._check(self._L.mrt_get_auto_regroup(self._ctx, C.byref(p)), "mrt_get_auto_regroup")
        return dict(enabled=bool(p.enabled), ratio=float(p.ratio), check_every=int(p.check_every))

    def read_regroup_stats(self) -> dict:
        """the auto-regroup policy's state on the device: checks, regroups, q_ref, q_last, q_level (one float64 per level), pending
        (mrt_read_regroup_stats; waits for the context's stream)"""
        s = _lib.MrtRegroupStats()
        self._check(self._L.mrt_read_regroup_stats(self._ctx, C.byref(s)), "mrt_read_regroup_stats")
        return dict(checks=int(s.checks), regroups=int(s.regroups), q_ref=float(s.q_ref), q_last=float(s.q_last),
                    q_level=[float(v) for v in s.q_level[:s.levels]], levels=int(s.levels), pending=bool(s.pending))

    def debug_regroup_info(self) -> dict:
        """n_pool, the block capacity in force, and the global / in-LDS depths of the last regroup (mrt_debug_regroup_info)"""
        out = (C.c_uint32 * 4)()
        self._check(self._L.mrt_debug_regroup_info(self._ctx, out), "mrt_debug_regroup_info")
        return dict(n_pool=int(out[0]), block=int(out[1]), global_depths=int(out[2]), lds_depths=int(out[3]))

    def debug_set_camera_masks(self, on: bool):
        """the camera-ray cluster masks and sphere lists off / on for the launches that follow (mrt_debug_set_camera_masks); 2: the lists
        wherever the tables apply, 3: the masks; images do not change"""
        self._check(self._L.mrt_debug_set_camera_masks(self._ctx, int(on)), "mrt_debug_set_camera_masks")

    def debug_read_camera_masks(self, table: bool = True) -> dict:
        """entries, words per entry, whether the last launch ran with the masks and whether the table is built for the current
        scene / camera / shard; with `table` the (entries, 4) uint32 array itself (mrt_debug_read_camera_masks)"""
        info = (C.c_uint32 * 4)()
        self._check(self._L.mrt_debug_read_camera_masks(self._ctx, info, None, 0), "mrt_debug_read_camera_masks")
        out = dict(entries=int(info[0]), words=int(info[1]), in_force=bool(info[2]), built=bool(info[3]), masks=None, lists=info[2] == 2)
        if table and out["entries"]:
            m = np.zeros((out["entries"], 4), np.uint32)
            self._check(self._L.mrt_debug_read_camera_masks(self._ctx, info, m.ctypes.data, m.size), "mrt_debug_read_camera_masks")
            out["masks"] = m
        return out

    def debug_read_camera_lists(self) -> np.ndarray:
        """the camera-ray sphere lists built with the masks: (entries, 4) uint32, word 0 the count (0xFFFFFFFF: overflowed), words
        1 .. 3 the member slots, 10 bits each (mrt_debug_read_camera_lists); no entries where the masks do not apply"""
        info = (C.c_uint32 * 4)()
        self._check(self._L.mrt_debug_read_camera_lists(self._ctx, info, None, 0), "mrt_debug_read_camera_lists")
        m = np.zeros((int(info[0]), 4), np.uint32)
        if len(m):
            self._check(self._L.mrt_debug_read_camera_lists(self._ctx, info, m.ctypes.data, m.size), "mrt_debug_read_camera_lists")
        return m

    def debug_set_regroup_block(self, clusters: int):
        self._check(self._L.mrt_debug_set_regroup_block(self._ctx, clusters), "mrt_debug_set_regroup_block")

    def debug_read_hierarchy(self) -> dict:
        """The scene's hierarchy and the four copies of the spheres' geometry as the device holds them, plus the host-side
        scalars the kernels get as arguments (mrt_debug_read_hierarchy)."""
        info = (C.c_uint32 * 16)()
        scal = (C.c_double * 8)()
        direct = np.zeros((4, 4), np.float32)
        direct_index = np.zeros(4, np.uint32)
        nul = [None] * 10
        self._check(self._L.mrt_debug_read_hierarchy(self._ctx, info, scal, direct.ctypes.data, direct_index.ctypes.data, *nul),
                    "mrt_debug_read_hierarchy")
        levels, n_top, n_nodes, n_members, n_direct, direct_first = (int(v) for v in info[:6])
        n_boxes, n = int(info[10]), int(info[12])
        top, nodes = np.zeros((n_top, 4), np.float32), np.zeros((n_nodes, 4), np.float32)
        midx = np.zeros(n_members, np.uint32)
        boxes, boxes_open = np.zeros((n_boxes, 6), np.float32), np.zeros((n_boxes, 6), np.float32)
        mfma = np.zeros(n_top // 32 * 512, np.uint16)
        spheres, shade = np.zeros((n, 4), np.float32), np.zeros((n, 8), np.float32)
        centres, radii = np.zeros((n, 4), np.float32), np.zeros(n, np.float32)
        arrays = [top, nodes, midx, boxes, boxes_open, mfma, spheres, shade, centres, radii]
        self._check(self._L.mrt_debug_read_hierarchy(self._ctx, info, scal, direct.ctypes.data, direct_index.ctypes.data,
                                                     *[a.ctypes.data if a.size else None for a in arrays]), "mrt_debug_read_hierarchy")
        return dict(levels=levels, top=top, nodes=nodes, midx=midx, mfma=mfma, n_direct=n_direct, direct_first=direct_first,
                    level_base=[int(info[6 + k]) for k in range(4)], n_members=n_members, boxes=boxes, boxes_open=boxes_open,
                    box_quad=bool(info[11]), box_kc=np.float32(scal[0]), origin=np.array(scal[1:4], np.float64),
                    axes=tuple(float(v) for v in scal[4:7]), reach=float(scal[7]), direct=direct, direct_index=direct_index,
                    box_cluster_first=int(info[13]), box_cluster_parent_first=int(info[14]), mfma_scene_ok=bool(info[15]),
                    spheres=spheres, shade=shade, centres=centres, radii=radii)

    def set_camera(self, cam: Camera):
        self._check(self._L.mrt_set_camera(self._ctx, C.byref(cam._c())), "mrt_set_camera")

    def set_seeds(self, seeds: np.ndarray):
        seeds = np.ascontiguousarray(seeds, np.uint32)
        self._check(self._L.mrt_set_seeds(self._ctx, seeds.ctypes.data, seeds.size), "mrt_set_seeds")

    def read_seeds(self) -> np.ndarray:
        rows, w = self.shard_info()[2:]
        out = np.empty((rows, w, 4), np.uint32)
        self._check(self._L.mrt_read_seeds(self._ctx, out.ctypes.data, out.size), "mrt_read_seeds")
        return out

    # -- frame loop
    def redraw(self):
        self._check(self._L.mrt_redraw(self._ctx), "mrt_redraw")

    def render(self, frames: int = 1):
        self._check(self._L.mrt_render(self._ctx, frames), "mrt_render")

    def sync(self):
        self._check(self._L.mrt_sync(self._ctx), "mrt_sync")

    def reset(self):
        self._check(self._L.mrt_reset(self._ctx), "mrt_reset")

    @property
    def locals(self) -> MrtLocals:
        out = MrtLocals()
        self._check(self._L.mrt_get_locals(self._ctx, C.byref(out)), "mrt_get_locals")
        return out

    def set_rng_shuffle(self, shuffle: Sequence[int]):
        self._check(self._L.mrt_set_rng_shuffle(self._ctx, (C.c_uint32 * 4)(*shuffle)), "mrt_set_rng_shuffle")

    def set_rng_mode(self, mode: int):
        """0 = the reference's per-pixel stream, 1 = per-sample counter-based states (extension)."""
        self._check(self._L.mrt_set_rng_mode(self._ctx, mode), "mrt_set_rng_mode")

    def set_draw_counting(self, enabled: bool):
        """False: launches without the per-lane RNG draw counter (counters()['rng_draws'] stops advancing); same images."""
        self._check(self._L.mrt_set_draw_counting(self._ctx, int(enabled)), "mrt_set_draw_counting")

    def set_samples_per_frame(self, spp: int):
        self._check(self._L.mrt_set_samples_per_frame(self._ctx, spp), "mrt_set_samples_per_frame")

    @property
    def frames_done(self) -> int:
        return int(self._L.mrt_frames_done(self._ctx))

    # -- output
    def shard_info(self) -> Tuple[int, int, int, int]:
        r, w, rows, width = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self._L.mrt_shard_info(self._ctx, C.byref(r), C.byref(w), C.byref(rows), C.byref(width)),
                    "mrt_shard_info")
        return r.value, w.value, rows.value, width.value

    def set_shard(self, rank: int, world: int):
        """mrt_set_shard: this context renders the 8-row bands b with b % world == rank; only while frames_done == 0."""
        self._check(self._L.mrt_set_shard(self._ctx, rank, world), "mrt_set_shard")

    def framebuffer_device_ptr(self) -> int:
        return int(self._L.mrt_framebuffer_device_ptr(self._ctx) or 0)

    def read_framebuffer(self) -> np.ndarray:
        """(H, W, 4) f32, row 0 = bottom (world == 1) or this shard's packed (local_rows, W, 4)."""
        _, world, rows, width = self.shard_info()
        shape = (self.args.height, width, 4) if world == 1 else (rows, width, 4)
        out = np.empty(shape, np.float32)
        self._check(self._L.mrt_read_framebuffer(self._ctx, out.ctypes.data, out.size), "mrt_read_framebuffer")
        return out

    def read_counters(self) -> dict:
        c = MrtCounters()
        self._check(self._L.mrt_read_counters(self._ctx, C.byref(c)), "mrt_read_counters")
        return {"samples": int(c.samples), "world_hit_calls": int(c.world_hit_calls), "rng_draws": int(c.rng_draws),
                "lane_slots": int(c.lane_slots), "member_tests": int(c.member_tests),
                "sweep_records": int(c.sweep_records)}

    def kernel_ms_history(self, n: int = 64) -> list:
        """GPU time (ms, HIP events on the launch stream) of the render kernel of the last <= n redraws."""
        buf = (C.c_float * n)()
        got = C.c_size_t()
        self._check(self._L.mrt_kernel_ms_history(self._ctx, buf, n, C.byref(got)), "mrt_kernel_ms_history")
        return [float(buf[i]) for i in range(got.value)]

    def debug_set_hierarchy(self, max_levels: int, top_target: int):
        """Tuning / test hook: depth rule of the bounding-sphere hierarchy built by the next set_world()."""
        self._check(self._L.mrt_debug_set_hierarchy(self._ctx, max_levels, top_target), "mrt_debug_set_hierarchy")

    def debug_set_sweep(self, mode: int):
        """Tuning / test hook: 0 = automatic, 1 = SGPR-fed VALU sweep, 2 = matrix-core sweep (same image either way)."""
        self._check(self._L.mrt_debug_set_sweep(self._ctx, mode), "mrt_debug_set_sweep")

    def debug_set_sweep_axes(self, axis=None):
        """Tuning / test hook: the matrix-core sweep of the scene of the next set_world() runs in the space scaled by axis (three
        of 1, 2, 4) instead of the one chosen for the scene; None returns to the choice.  Same image either way."""
        arr = (C.c_float * 3)(*axis) if axis is not None else None
        self._check(self._L.mrt_debug_set_sweep_axes(self._ctx, arr), "mrt_debug_set_sweep_axes")

    def debug_sweep_axes(self):
        """The axis scales of the space the current scene's matrix-core sweep runs in ((1, 1, 1): the world's)."""
        arr = (C.c_float * 3)()
        self._check(self._L.mrt_debug_sweep_axes(self._ctx, arr), "mrt_debug_sweep_axes")
        return tuple(float(v) for v in arr)

    def debug_sweep_variant(self) -> int:
        """1 = SGPR-fed VALU sweep, 2 = matrix-core sweep, for the next redraw (0 before a scene is set)."""
        return int(self._L.mrt_debug_sweep_variant(self._ctx))

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        self._check(self._L.mrt_last_kernel_ms(self._ctx, C.byref(ms)), "mrt_last_kernel_ms")
        return float(ms.value)

    def debug_read_pixel_costs(self) -> np.ndarray:
        """(rows, W) u32: bounce-loop trips (= world_hit calls when ray_depth > 0) of every pixel in the last frame;
        full image when unsharded, else this shard's packed rows."""
        _, world, rows, width = self.shard_info()
        packed = np.empty((rows, width), np.uint32)
        self._check(self._L.mrt_debug_read_pixel_costs(self._ctx, packed.ctypes.data, packed.size), "mrt_debug_read_pixel_costs")
        return packed[:self.args.height] if world == 1 else packed

    def debug_world_hit(self, rays: np.ndarray, n_spheres: int):
        """One world_hit per ray (rays: (n, 6) f32 = origin, unit direction) through the render kernel's sweep + walk.
        Returns (hit index (n,) i32 [-1 = miss], t (n,) f32, candidates (n, n_spheres) bool = spheres that reached the root
        tests)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n, words = len(rays), max(1, (n_spheres + 31) // 32)
        hit = np.empty((n, 2), np.int32)
        cand = np.zeros((n, words), np.uint32)
        self._check(self._L.mrt_debug_world_hit(self._ctx, rays.ctypes.data, n, hit.ctypes.data, cand.ctypes.data, words),
                    "mrt_debug_world_hit")
        bits = np.unpackbits(cand.view(np.uint8), axis=1, bitorder="little")[:, :n_spheres].astype(bool)
        return hit[:, 0].copy(), hit[:, 1].copy().view(np.float32), bits

    def debug_world_hit_stats(self):
        """(rays traced, member tests) of the last debug_world_hit: member tests = 4 per cluster item of the walk + one per direct
        sphere and usable ray (mrt_debug_world_hit_stats)"""
        out = (C.c_uint64 * 2)()
        self._check(self._L.mrt_debug_world_hit_stats(self._ctx, out), "mrt_debug_world_hit_stats")
        return int(out[0]), int(out[1])

    def debug_last_launch(self):
        """(main, pilot or None): template-argument bits of the last render launch -- 1 COUNT, 2 PILOT, 4 CTR, 8 SMALL, 16 MFMA,
        32 quadratic box slack (large scenes), 64 the camera-ray sphere lists (SC = 3)."""
        out = (C.c_uint32 * 2)()
        self._check(self._L.mrt_debug_last_launch(self._ctx, out), "mrt_debug_last_launch")
        return int(out[0]), (None if out[1] == 0xFFFFFFFF else int(out[1]))

    def set_wait_timeout(self, seconds: float):
        """Deadline of every wait for the GPU inside the library (0 = none): a longer wait raises MrtError(MRT_ERR_STALLED)."""
        self._check(self._L.mrt_set_wait_timeout(self._ctx, float(seconds)), "mrt_set_wait_timeout")

    def get_schedule(self) -> dict:
        """The launch schedule: a frame runs on 1 / div of the persistent waves, max(2, div) x mult frames are in flight."""
        out = (C.c_uint32 * 6)()
        self._check(self._L.mrt_get_schedule(self._ctx, out), "mrt_get_schedule")
        return {"div": int(out[0]), "mult": int(out[1]), "settled": bool(out[2]), "frames_in_flight": int(out[3]),
                "last_launch_div": int(out[4]), "max_concurrent_frames": int(out[5])}

    def set_schedule_hint(self, div: int, mult: int = 1):
        """Pin the launch schedule (what an earlier run settled at); (0, 0) = measure again.  The images do not change."""
        self._check(self._L.mrt_set_schedule_hint(self._ctx, div, mult), "mrt_set_schedule_hint")

    def debug_stream_concurrency(self, streams: int = 8) -> float:
        out = C.c_float()
        self._check(self._L.mrt_debug_stream_concurrency(self._ctx, streams, C.byref(out)), "mrt_debug_stream_concurrency")
        return float(out.value)

    def debug_check_context(self) -> Optional[str]:
        """Host only: None if no call the context accepts could touch a buffer, stream or event that is not there, else the
        first finding (mrt_debug_check_context)."""
        why = C.create_string_buffer(512)
        return why.value.decode() if self._L.mrt_debug_check_context(self._ctx, why, len(why)) else None

    def debug_set_frames_in_flight(self, slots: int):
        """How many frames may be in flight, each on a side stream of its own (1..8; 0 = automatic)."""
        self._check(self._L.mrt_debug_set_frames_in_flight(self._ctx, slots), "mrt_debug_set_frames_in_flight")

    _HOLD_STREAMS = {"context": _lib.HOLD_CONTEXT, "slot": _lib.HOLD_SLOT, "present": _lib.HOLD_PRESENT, "noise": _lib.HOLD_NOISE}

    def debug_hold(self, which: str, index: int = 0, ticks: int = 1_000_000, max_polls: int = 1 << 20):
        """mrt_debug_hold: one kernel on the "context" stream, the side stream of frame "slot" `index`, the "present" or the
        "noise" stream that ends after `ticks` of the 100 MHz clock or `max_polls` polls, whichever comes first; what is queued
        behind it on that stream starts late.  Creates nothing: MrtError (MRT_ERR_STATE) where the stream does not exist yet."""
        self._check(self._L.mrt_debug_hold(self._ctx, self._HOLD_STREAMS[which], index, ticks, max_polls), "mrt_debug_hold")

    def debug_hold_stamps(self):
        """(start tick, end tick, polls given) of the most recent debug_hold, once it has ended (after sync())"""
        out = (C.c_uint64 * 3)()
        self._check(self._L.mrt_debug_hold_stamps(self._ctx, out), "mrt_debug_hold_stamps")
        return int(out[0]), int(out[1]), int(out[2])

    def debug_set_schedule(self, pilot_spp: int, waves_per_cu: int):
        """Before the first redraw: samples per pixel of the pilot launch, persistent waves per CU (0 = automatic)."""
        self._check(self._L.mrt_debug_set_schedule(self._ctx, pilot_spp, waves_per_cu), "mrt_debug_set_schedule")

    def debug_sort_tiles(self, cost, tiles=None) -> np.ndarray:
        """The tile-queue sort a frame runs, on caller-supplied costs (u32, at most the context's tile count of them): the whole
        range (tiles None) or the listed tile ids, as a subset frame's list.  Returns the queue, heaviest first.  Synchronous;
        the slot's own estimate is invalid afterwards (mrt_debug_sort_tiles)."""
        cost = np.ascontiguousarray(cost, np.uint32).ravel()
        lst = None if tiles is None else np.ascontiguousarray(tiles, np.uint32).ravel()
        n = len(cost) if lst is None else len(lst)
        out = np.empty(n, np.uint32)
        self._check(self._L.mrt_debug_sort_tiles(self._ctx, cost.ctypes.data, len(cost), None if lst is None else lst.ctypes.data, n,
                                                 out.ctypes.data), "mrt_debug_sort_tiles")
        return out

    def debug_read_tile_schedule(self):
        """(costs (n_tiles,) u32 as the last slot's finalize or per-tile blend left them, the queue order (entries,) u32 its most
        recent render launch was given, {"kind": one of _lib.TILE_ORDER_KINDS, "entries", "pilot", "slot"}).  Waits for the
        frames in flight."""
        _, _, rows, width = self.shard_info()
        tiles = ((width + 7) // 8) * (rows // 8)
        n, info = C.c_uint32(), (C.c_uint32 * 4)()
        cost, order = np.empty(tiles, np.uint32), np.empty(tiles, np.uint32)
        self._check(self._L.mrt_debug_read_tile_schedule(self._ctx, cost.ctypes.data, order.ctypes.data, tiles, C.byref(n), info),
                    "mrt_debug_read_tile_schedule")
        assert n.value == tiles
        return cost, order[:info[1]].copy(), {"kind": _lib.TILE_ORDER_KINDS[info[0]], "entries": int(info[1]), "pilot": bool(info[2]),
                                              "slot": int(info[3])}

    def debug_set_tile_sort(self, enabled: bool):
        """A/B switch: False queues tiles in index order instead of heaviest-first (same image)."""
        self._check(self._L.mrt_debug_set_tile_sort(self._ctx, int(enabled)), "mrt_debug_set_tile_sort")

    def debug_set_boxes(self, mode):
        """A/B switch (large scenes, whose walk tests every node's axis-aligned box): 0 / False = the boxes are opened wide and
        never reject, 1 / 2 / True = the real boxes (default); the image is the same."""
        self._check(self._L.mrt_debug_set_boxes(self._ctx, 2 if mode is True else int(mode)), "mrt_debug_set_boxes")

    def debug_arith(self, mode: int, bits_range: Sequence[int], count: int = 0, seed: int = 1):
        """mrt_debug_arith: (tested, mismatches, smallest mismatching operand) of the kernel's unscaled sqrt (mode 0, every
        bit pattern of bits_range[0..1]) / division (mode 1 / 2, `count` random pairs) against hipcc's own."""
        out = (C.c_uint64 * 3)()
        r = (C.c_uint32 * 4)(*(list(bits_range) + [0, 0, 0, 0])[:4])
        self._check(self._L.mrt_debug_arith(self._ctx, mode, r, count, seed, out), "mrt_debug_arith")
        return int(out[0]), int(out[1]), int(out[2])

    def debug_arith_pairs(self, x: np.ndarray, y: np.ndarray) -> np.ndarray:
        """mrt_debug_arith_pairs: (n, 6) u32 = bits of x / y, unscaled quotient, sqrtf(x), unscaled root, and the two guards."""
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32)
        assert x.shape == y.shape and x.ndim == 1
        out = np.zeros((len(x), 6), np.uint32)
        self._check(self._L.mrt_debug_arith_pairs(self._ctx, x.ctypes.data, y.ctypes.data, len(x), out.ctypes.data), "mrt_debug_arith_pairs")
        return out

    def debug_set_frame_batching(self, enabled):
        """A/B switch: False / 0 makes render(frames) launch every frame on its own; True / 1 automatic; 2 / 3 force the
        batch's form (2: a lane keeps its pixel for all frames of the batch, 3: frames as layers of the tile queue)."""
        self._check(self._L.mrt_debug_set_frame_batching(self._ctx, int(enabled)), "mrt_debug_set_frame_batching")

    def last_set_world_ms(self) -> float:
        """Host wall time of the last scene upload (hierarchy build + copies); one-off per scene."""
        ms = C.c_float()
        self._check(self._L.mrt_debug_last_set_world_ms(self._ctx, C.byref(ms)), "mrt_debug_last_set_world_ms")
        return float(ms.value)

    # -- multi-GPU (one process per GPU): RCCL gather on a caller-supplied ncclComm_t
    def gather_rccl(self, nccl_comm: int, root: int = 0):
        self._check(self._L.mrt_gather_rccl(self._ctx, nccl_comm, root), "mrt_gather_rccl")

    def debug_set_gather_per_band(self, enabled: bool):
        """On the root: mrt_gather uses the cross-device form of its copies (one peer copy per band) on one device too."""
        self._check(self._L.mrt_debug_set_gather_per_band(self._ctx, int(enabled)), "mrt_debug_set_gather_per_band")

    def gathered_device_ptr(self) -> int:
        return int(self._L.mrt_gathered_device_ptr(self._ctx) or 0)

    def read_gathered(self) -> np.ndarray:
        """(H, W, 4) f32, row 0 = bottom: the full frame assembled on this (root) State by the last gather."""
        out = np.empty((self.args.height, self.args.width, 4), np.float32)
        self._check(self._L.mrt_read_gathered(self._ctx, out.ctypes.data, out.size), "mrt_read_gathered")
        return out

    # -- the noise estimate across shards (include/myraytracer_amd.h, "the noise estimate across shards"): S travels with the
    #    gather and the root denoises the gathered frame
    def set_gather_noise(self, enabled: bool):
        """mrt_set_gather_noise: from the next gather on, S travels with the colour (gather(): the root's setting decides;
        gather_rccl(): every rank's own, and all must agree).  A change drops the gathered S until the next gather."""
        self._check(self._L.mrt_set_gather_noise(self._ctx, int(enabled)), "mrt_set_gather_noise")

    def read_gathered_noise(self) -> np.ndarray:
        """(H, W) f32, row 0 = bottom: the full-frame S assembled on this (root) State by the last gather."""
        out = np.empty((self.args.height, self.args.width), np.float32)
        self._check(self._L.mrt_read_gathered_noise(self._ctx, out.ctypes.data, out.size), "mrt_read_gathered_noise")
        return out

    def read_gathered_denoised(self) -> np.ndarray:
        """(H, W, 4) f32, row 0 = bottom: the last gathered frame, denoised on this (root) State with the gather's snapshot of
        K and the frame count and the guides of this State's current camera and scene."""
        out = np.empty((self.args.height, self.args.width, 4), np.float32)
        self._check(self._L.mrt_read_gathered_denoised(self._ctx, out.ctypes.data, out.size), "mrt_read_gathered_denoised")
        return out

    def debug_read_gathered_guides(self) -> dict:
        """debug_read_guides' dict of the guides read_gathered_denoised filters with: the full image's, on a root that is a
        shard too."""
        h, w = self.args.height, self.args.width
        g = {"rays": np.empty((h, w, 6), np.float32), "index": np.empty((h, w), np.int32), "t": np.empty((h, w), np.float32),
             "normal": np.empty((h, w, 3), np.float32), "albedo": np.empty((h, w, 3), np.float32)}
        self._check(self._L.mrt_debug_read_gathered_guides(self._ctx, g["rays"].ctypes.data, g["index"].ctypes.data, g["t"].ctypes.data,
                                                           g["normal"].ctypes.data, g["albedo"].ctypes.data, h * w),
                    "mrt_debug_read_gathered_guides")
        return g

    # -- present pass (the reference's pass 2, lib.rs:270-297 / sample_framebuffer.wgsl): 8-bit sRGB images, read back without
    #    waiting for the frames in flight; and the linear floats themselves, as binary16 or as the source's float32 bits
    _PRESENT_FORMATS = {"rgba8": _lib.PRESENT_RGBA8_SRGB, "bgra8": _lib.PRESENT_BGRA8_SRGB,
                        "rgba16f": _lib.PRESENT_RGBA16F_LINEAR, "rgba32f": _lib.PRESENT_RGBA32F_LINEAR}
    _PRESENT_DTYPES = {_lib.PRESENT_RGBA16F_LINEAR: np.float16, _lib.PRESENT_RGBA32F_LINEAR: np.float32}

    def present(self, fmt: str = "rgba8", flip: bool = True, gathered: bool = False, denoise: bool = False, temporal: bool = False,
                gathered_denoised: bool = False, view: bool = False):
        """mrt_present: queue the most recent frame's image: 8-bit sRGB ("rgba8" / "bgra8") or linear ("rgba16f": binary16,
        _lib.half_bits of every channel; "rgba32f": the source's float32 bits).  flip = rows top-down; gathered = the
        root's full frame of the last gather; denoise = the denoised frame, read_denoised's image; temporal = the temporal image,
        read_temporal's; gathered_denoised = the last gathered frame denoised on the root, read_gathered_denoised's image, a
        source of its own: with flip only; view = the current diagnostic view (set_view), read_view's image, with flip only.
        Asynchronous."""
        if fmt not in self._PRESENT_FORMATS:
            raise ValueError(f"present: format {fmt!r} ({', '.join(self._PRESENT_FORMATS)})")
        flags = ((_lib.PRESENT_FLIP_Y if flip else 0) | (_lib.PRESENT_GATHERED if gathered else 0) |
                 (_lib.PRESENT_DENOISED if denoise else 0) | (_lib.PRESENT_TEMPORAL if temporal else 0) |
                 (_lib.PRESENT_GATHERED_DENOISED if gathered_denoised else 0) | (_lib.PRESENT_VIEW if view else 0))
        self._check(self._L.mrt_present(self._ctx, self._PRESENT_FORMATS[fmt], flags), "mrt_present")

    def acquire_presented(self, newest: bool = True, wait: bool = True, copy: bool = True):
        """mrt_present_acquire: ([rows, width, 4] of the image's format -- uint8, float16 for "rgba16f", float32 for "rgba32f" --
        and the info dict) or None if no image has finished (wait=False) or none is
        queued.  newest: the most recent finished image (older ones are dropped), else the oldest.  copy=False returns a view
        of the library's pinned buffer, valid until release_presented() / the next acquire / reset / close."""
        px = C.POINTER(C.c_uint8)()
        info = _lib.MrtPresentInfo()
        mode = _lib.ACQUIRE_NEWEST if newest else _lib.ACQUIRE_OLDEST
        self._check(self._L.mrt_present_acquire(self._ctx, mode, int(wait), C.byref(px), C.byref(info)), "mrt_present_acquire")
        if not px:
            return None
        dtype = self._PRESENT_DTYPES.get(info.format, np.uint8)
        img = np.ctypeslib.as_array(px, shape=(info.rows, info.row_bytes)).view(dtype).reshape(info.rows, info.width, 4)
        d ={k: int(getattr(info, k)) for k, _ in _lib.MrtPresentInfo._fields_}
        return (img.copy() if copy else img), d

    def release_presented(self):
        self._check(self._L.mrt_present_release(self._ctx), "mrt_present_release")

    def set_present_ring(self, depth: int):
        """Pin the ring of presented images to `depth` entries (2..18); 0 = automatic (frames in flight + 2)."""
        self._check(self._L.mrt_set_present_ring(self._ctx, depth), "mrt_set_present_ring")

    def debug_set_present_copy(self, mode: int):
        """Where the present's device-to-host copy runs: 0 = a stream of its own, 1 = the context's stream (default)."""
        self._check(self._L.mrt_debug_set_present_copy(self._ctx, mode), "mrt_debug_set_present_copy")

    def debug_present_encode(self, rgba: np.ndarray, fmt: str = "rgba8", flip: bool = False) -> np.ndarray:
        """The present kernel on caller-supplied texels: float32 [rows, width, 4] -> uint8 [rows, width, 4], synchronously."""
        rgba = np.ascontiguousarray(rgba, np.float32)
        rows, width, _ = rgba.shape
        out = np.empty((rows, width, 4), np.uint8)
        self._check(self._L.mrt_debug_present_encode(self._ctx, rgba.ctypes.data, width, rows, self._PRESENT_FORMATS[fmt],
                                                     _lib.PRESENT_FLIP_Y if flip else 0, out.ctypes.data),
                    "mrt_debug_present_encode")
        return out

    # -- noise estimate (include/myraytracer_amd.h, "noise estimate"): the per-texel luminance variance of the accumulation and
    #    an image-level report, computed on the device and read back without waiting for the frames in flight
    def set_noise_tracking(self, enabled: bool):
        """Turn noise tracking on / off; only while frames_done == 0 (after creation or reset()).  Survives reset()."""
        self._check(self._L.mrt_set_noise_tracking(self._ctx, int(enabled)), "mrt_set_noise_tracking")

    def noise_query(self, threshold: float = 0.02, floor: float = 0.01, tile_map: str = "max_rel", budget: Optional[int] = None,
                    max_frames: int = 8):
        """Queue the noise report of the most recent frame (asynchronous).  threshold: the relative standard error above which a
        pixel counts as noisy; floor: the luminance below which the relative error is taken against the floor instead.
        tile_map: what the report's tile map holds -- "max_rel", the tile's largest relative error (render_adaptive selects from
        it), or "sum_s", the tile's summed S (render_budget allocates from it); the report's scalar fields are the same.
        budget=N: a "sum_s" query that also allocates N tile-frames, at most max_frames a tile, on the device right behind the
        reduction (mrt_noise_query_budget): budget_plan() reads the plan, render_planned() renders it."""
        if budget is not None:                             # (always a "sum_s" query, whatever tile_map says)
            self._check(self._L.mrt_noise_query_budget(self._ctx, threshold, floor, budget, max_frames), "mrt_noise_query_budget")
            return
        if tile_map not in _lib.TILE_MAP_KINDS:
            raise ValueError(f"noise_query: unknown tile_map {tile_map!r} ({', '.join(_lib.TILE_MAP_KINDS)})")
        if tile_map == "max_rel":
            self._check(self._L.mrt_noise_query(self._ctx, threshold, floor), "mrt_noise_query")
        else:
            self._check(self._L.mrt_noise_query_map(self._ctx, threshold, floor, _lib.TILE_MAP_KINDS.index(tile_map)), "mrt_noise_query_map")

    def noise_result(self, wait: bool = True) -> Optional[dict]:
        """The newest finished report as a dict, or None if none has finished (wait=False) or none was queued.  wait=True waits
        (bounded) for the newest queued report, never for frames queued after it."""
        r = _lib.MrtNoiseReport()
        self._check(self._L.mrt_noise_result(self._ctx, int(wait), C.byref(r)), "mrt_noise_result")
        return noise_report_dict(r) if r.seq else None

    def read_noise(self) -> np.ndarray:
        """S, the per-texel luminance variance of the accumulation: (H, W) f32 (world == 1, row 0 = bottom) or this shard's
        packed (local_rows, W).  Waits for the frames in flight, as read_framebuffer does."""
        _, world, rows, width = self.shard_info()
        out = np.empty((self.args.height if world == 1 else rows, width), np.float32)
        self._check(self._L.mrt_read_noise(self._ctx, out.ctypes.data, out.size), "mrt_read_noise")
        return out

    def read_noise_tiles(self) -> np.ndarray:
        """The latest query's tile map -- the per-8x8-tile maximum of the relative error, or the tile's summed S after
        noise_query(tile_map="sum_s") --: (tile rows, tiles_x) f32, numbered as the framebuffer's bands (a shard's packed bands).
        Waits for that query only."""
        tx, tr = C.c_uint32(), C.c_uint32()
        self._L.mrt_read_noise_tiles(self._ctx, None, 0, C.byref(tx), C.byref(tr))     # (the shape; the status comes below)
        out = np.empty((tr.value, tx.value), np.float32)
        self._check(self._L.mrt_read_noise_tiles(self._ctx, out.ctypes.data, out.size, C.byref(tx), C.byref(tr)),
                    "mrt_read_noise_tiles")
        return out

    def render_until(self, target_rel_rmse: float, max_frames: int, check_every: int = 16, threshold: float = 0.02,
                     floor: float = 0.01, adaptive: bool = False, budget: Optional[int] = None,
                     plan: str = "host") -> Tuple[int, dict]:
        """Render chunks of check_every frames until a noise report's rel_rmse <= target_rel_rmse or frames_done reaches
        max_frames; returns (frames_done, report).  Keeps the pipeline full by lagging one check: chunk k + 1 is queued before
        report k is waited for, so the stop overshoots the first report that meets the target by at most check_every frames
        (the one lagged chunk); the report returned is that one (report['frames_done'] <= frames_done).  With seeded input
        the stopping frame is deterministic.  At max_frames, the report is that of the final image.  Turns tracking on if it
        is off and frames_done == 0.

        adaptive=True: every chunk after the first is render_adaptive over the tiles that the report queued one chunk
        earlier counts as noisy (that report has been waited for already, so a chunk stays in flight), and the loop also
        stops at a report with above == 0 (no tile left above `threshold`).  frames_done counts subset frames as frames.

        budget=N (not with adaptive=True): every chunk after the first is render_budget(N, min(check_every, 32), report): N
        tile-frames allocated from the summed-S map of the report queued one chunk earlier -- the same lag -- so the queries
        are noise_query(tile_map="sum_s").  The loop also stops when a chunk finds nothing worth a frame.

        plan="device" (with budget=N): the queries are noise_query(budget=N, max_frames=min(check_every, 32)), which allocate on
        the device behind the reduction, and every chunk after the first is render_planned(report) -- the same one-check lag.
        A plan is a target (n at its query + k), so the frames of the chunk queued between a plan's query and its rendering
        count towards it; a chunk that finds its plan met already queues nothing and the loop goes on, and it stops when a plan
        as allocated is empty.  A last chunk with fewer frames left than the plans' max_frames is render_budget's."""
        if check_every < 1 or max_frames < 0:
            raise ValueError("render_until: check_every >= 1, max_frames >= 0")
        if budget is not None and (adaptive or budget < 1):
            raise ValueError("render_until: budget >= 1, and not together with adaptive=True")
        if plan not in ("host", "device") or (plan == "device" and budget is None):
            raise ValueError('render_until: plan is "host" or "device", and "device" needs a budget')
        if self.frames_done == 0:
            self.set_noise_tracking(True)
        tile_map = "max_rel" if budget is None else "sum_s"
        plan_frames = min(check_every, 32)

        def chunk(select_from=None):
            """whether the chunk had anything to queue"""
            n = min(check_every, max_frames - self.frames_done)
            if n > 0:
                if select_from is None:
                    self.render(n)
                elif budget is not None and plan == "device" and n >= plan_frames:
                    return self.render_planned(select_from)["planned_tile_frames"] != 0
                elif budget is not None:
                    return self.render_budget(budget, min(n, 32), select_from)["tile_frames"] != 0
                else:
                    self.render_adaptive(n, select_from)
            return True

        def query():
            if plan == "device":
                self.noise_query(threshold, floor, budget=budget, max_frames=plan_frames)
            else:
                self.noise_query(threshold, floor, tile_map)

        chunk()
        query()
        earlier = None                                     # adaptive, budget: the report one chunk before the newest
        while True:
            lagged = adaptive or budget is not None
            spent = chunk(earlier["seq"] if lagged and earlier is not None else None)   # the lagged chunk
            rep = self.noise_result(wait=True)             # the newest queued: the check before that chunk
            if rep["rel_rmse"] <= target_rel_rmse:
                return self.frames_done, rep
            if rep["frames_done"] >= max_frames:
                return self.frames_done, rep
            if adaptive and rep["above"] == 0:
                return self.frames_done, rep
            if not spent:
                return self.frames_done, rep
            earlier = rep
            query()

    # -- adaptive sampling (include/myraytracer_amd.h, "adaptive sampling"): frames over a list of 8x8 tiles, each tile blended
    #    at its own frame count
    def render_tiles(self, tiles, frames: int = 1):
        """Queue `frames` subset frames over the listed tile ids (tile = band * tiles_x + column, row 0 at the bottom)."""
        t = np.ascontiguousarray(np.asarray(tiles).ravel(), np.uint32)
        self._check(self._L.mrt_render_tiles(self._ctx, t.ctypes.data if t.size else None, t.size, frames), "mrt_render_tiles")

    def render_adaptive(self, frames: int = 1, report_seq: int = 0) -> Tuple[int, int]:
        """Subset frames over the tiles whose entry in noise report `report_seq` (0: the newest finished one, every tile if none
        has finished) is above its threshold; returns (the report used, 0 for none; the tiles selected).  Nothing is queued when
        no tile is selected."""
        used, sel = C.c_uint64(), C.c_uint32()
        self._check(self._L.mrt_render_adaptive(self._ctx, frames, report_seq, C.byref(used), C.byref(sel)), "mrt_render_adaptive")
        return int(used.value), int(sel.value)

    def render_budget(self, budget: int, max_frames: int = 8, report_seq: int = 0) -> dict:
        """Spend `budget` tile-frames (one subset frame over one 8x8 tile each) where the model s_t * K(n_t) says they lower the
        image's summed variance most, at most max_frames (1 .. 32) per tile: allocated from the summed-S map of noise report
        `report_seq` (0: the newest finished report queued with tile_map="sum_s"; none: nothing is queued and used_seq is 0) and
        rendered level by level through render_tiles.  Returns {used_seq, tile_frames, tiles, frames, var_before, var_after, k}
        with k the frames given to every tile, (tile rows, tiles_x) uint32."""
        r = _lib.MrtBudgetResult()
        tx, tr = C.c_uint32(), C.c_uint32()
        self._L.mrt_read_tile_frames(self._ctx, None, 0, C.byref(tx), C.byref(tr))     # (the shape)
        k = np.zeros((tr.value, tx.value), np.uint32)
        self._check(self._L.mrt_render_budget(self._ctx, budget, max_frames, report_seq, C.byref(r), k.ctypes.data, k.size),
                    "mrt_render_budget")
        return dict(budget_result_dict(r), k=k)

    def _tile_shape(self):
        tx, tr = C.c_uint32(), C.c_uint32()
        self._L.mrt_read_tile_frames(self._ctx, None, 0, C.byref(tx), C.byref(tr))     # (the shape)
        return tr.value, tx.value

    def budget_plan(self, report_seq: int = 0) -> dict:
        """The plan that noise_query(budget=N) allocated on the device with report `report_seq` (0: the newest finished report
        that carries one, without waiting; none: used_seq is 0), as allocated: render_budget's dict, k the frames planned for
        every tile.  Reads back k and the 64-byte result once that query has finished; waits for that query only."""
        r = _lib.MrtBudgetResult()
        k = np.zeros(self._tile_shape(), np.uint32)
        self._check(self._L.mrt_read_budget_plan(self._ctx, report_seq, k.ctypes.data, k.size, C.byref(r)), "mrt_read_budget_plan")
        return dict(budget_result_dict(r), k=k)

    def render_planned(self, report_seq: int = 0) -> dict:
        """Render the plan of report `report_seq` (budget_plan's rule) level by level through render_tiles.  The plan is a target:
        tile t should reach its frame count at the query + k_t, so frames queued since the query count towards it and k, with
        tile_frames, tiles and frames, is what this call queued (the plan's own k while nothing was queued in between);
        var_before and var_after stay the plan's.  planned_tile_frames: the plan's tile_frames as allocated."""
        r, p = _lib.MrtBudgetResult(), _lib.MrtBudgetResult()
        k = np.zeros(self._tile_shape(), np.uint32)
        self._check(self._L.mrt_render_planned(self._ctx, report_seq, C.byref(r), k.ctypes.data, k.size), "mrt_render_planned")
        if r.used_seq:
            self._check(self._L.mrt_read_budget_plan(self._ctx, r.used_seq, None, 0, C.byref(p)), "mrt_read_budget_plan")
        return dict(budget_result_dict(r), k=k, planned_tile_frames=int(p.tile_frames))

    @staticmethod
    def budget_allocate(s, n, max_framebuffer_weight: float, budget: int, max_frames: int = 8) -> Tuple[np.ndarray, dict]:
        """mrt_budget_allocate (host only): (k, result) for the summed-S map `s` and the frame counts `n` of the same shape; k
        has that shape too."""
        s = np.ascontiguousarray(s, np.float32)
        n = np.ascontiguousarray(n, np.uint32)
        if s.shape != n.shape:
            raise ValueError("budget_allocate: s and n differ in shape")
        k = np.zeros(s.shape, np.uint32)
        r = _lib.MrtBudgetResult()
        st = _lib.load().mrt_budget_allocate(s.ctypes.data, n.ctypes.data, s.size, max_framebuffer_weight, budget, max_frames,
                                             k.ctypes.data, C.byref(r))
        if st != 0:
            raise MrtError(st, "mrt_budget_allocate", "")
        return k, budget_result_dict(r)

    def debug_budget_plan(self, s, n, budget: int, max_frames: int = 8) -> Tuple[np.ndarray, dict]:
        """mrt_debug_budget_plan: the device's allocation (noise_query(budget=N)'s kernels) on the summed-S values `s` and the
        frame counts `n` (an array of s's shape, or an int: that count for every tile), synchronously: (k in s's shape, result).
        K is this context's table, so budget_allocate(s, n, the context's max_framebuffer_weight, ...) is the yardstick."""
        s = np.ascontiguousarray(s, np.float32)
        uniform = np.ndim(n) == 0
        if not uniform:
            n = np.ascontiguousarray(n, np.uint32)
            if s.shape != n.shape:
                raise ValueError("debug_budget_plan: s and n differ in shape")
        k = np.zeros(s.shape, np.uint32)
        r = _lib.MrtBudgetResult()
        self._check(self._L.mrt_debug_budget_plan(self._ctx, s.ctypes.data, None if uniform else n.ctypes.data, int(n) if uniform else 0,
                                                  s.size, budget, max_frames, k.ctypes.data, C.byref(r)), "mrt_debug_budget_plan")
        return k, budget_result_dict(r)

    def tile_frames(self) -> np.ndarray:
        """Every tile's frame count n_t: (tile rows, tiles_x) uint32.  Waits for the frames in flight, as read_framebuffer does."""
        tx, tr = C.c_uint32(), C.c_uint32()
        self._L.mrt_read_tile_frames(self._ctx, None, 0, C.byref(tx), C.byref(tr))     # (the shape; the status comes below)
        out = np.empty((tr.value, tx.value), np.uint32)
        self._check(self._L.mrt_read_tile_frames(self._ctx, out.ctypes.data, out.size, C.byref(tx), C.byref(tr)),
                    "mrt_read_tile_frames")
        return out

    def debug_noise_reduce(self, S: np.ndarray, rgba: np.ndarray, K: float, threshold: float = 0.02, floor: float = 0.01):
        """The noise reduction on caller-supplied buffers (S: (rows, W) f32, rgba: (rows, W, 4) f32), synchronously:
        (report dict, tile map (ceil(rows / 8), ceil(W / 8)) f32)."""
        S = np.ascontiguousarray(S, np.float32)
        rgba = np.ascontiguousarray(rgba, np.float32)
        rows, width = S.shape
        assert rgba.shape == (rows, width, 4)
        tiles = np.empty(((rows + 7) // 8, (width + 7) // 8), np.float32)
        r = _lib.MrtNoiseReport()
        self._check(self._L.mrt_debug_noise_reduce(self._ctx, S.ctypes.data, rgba.ctypes.data, width, rows, K, threshold, floor,
                                                   C.byref(r), tiles.ctypes.data), "mrt_debug_noise_reduce")
        return noise_report_dict(r), tiles

    # -- denoiser (include/myraytracer_amd.h, "denoiser"): an edge-aware a-trous filter guided by S and by first-hit guides
    def set_denoise_params(self, **kw):
        """Change the named fields of the denoise parameters (iterations, sigma_l, normal_exp, sigma_z, sigma_a); the others keep
        their current values."""
        p = _lib.MrtDenoiseParams()
        self._check(self._L.mrt_get_denoise_params(self._ctx, C.byref(p)), "mrt_get_denoise_params")
        for k, v in kw.items():
            if k not in DENOISE_FIELDS:
                raise ValueError(f"set_denoise_params: unknown field {k!r} ({', '.join(DENOISE_FIELDS)})")
            setattr(p, k, v)
        self._check(self._L.mrt_set_denoise_params(self._ctx, C.byref(p)), "mrt_set_denoise_params")

    def denoise_params(self) -> dict:
        p = _lib.MrtDenoiseParams()
        self._check(self._L.mrt_get_denoise_params(self._ctx, C.byref(p)), "mrt_get_denoise_params")
        return denoise_params_dict(p)

    def set_denoise_variance(self, mode, spatial_frames: int = 3):
        """Where the luminance stop's variance comes from: "accumulated" (0, the default: S * K of the one pixel), "prefiltered"
        (1: its 3 x 3 mean) or "spatial-early" (2: a spatial estimate while frames_done < spatial_frames, prefiltered from then on)."""
        if isinstance(mode, str):
            if mode not in DENOISE_VARIANCE_MODES:
                raise ValueError(f"set_denoise_variance: unknown mode {mode!r} ({', '.join(DENOISE_VARIANCE_MODES)})")
            mode = DENOISE_VARIANCE_MODES.index(mode)
        self._check(self._L.mrt_set_denoise_variance(self._ctx, mode, spatial_frames), "mrt_set_denoise_variance")

    def denoise_variance(self) -> tuple:
        """(mode name, spatial_frames)."""
        mode, frames = C.c_uint32(), C.c_uint32()
        self._check(self._L.mrt_get_denoise_variance(self._ctx, C.byref(mode), C.byref(frames)), "mrt_get_denoise_variance")
        return DENOISE_VARIANCE_MODES[mode.value], int(frames.value)

    def set_denoise_adaptive(self, enabled: bool):
        """Whether an adaptive accumulation (render_tiles / render_adaptive since the last reset) is denoised, with K and the
        variance estimate chosen per tile, or refused (the default)."""
        self._check(self._L.mrt_set_denoise_adaptive(self._ctx, int(bool(enabled))), "mrt_set_denoise_adaptive")

    def denoise_adaptive(self) -> bool:
        on = C.c_int()
        self._check(self._L.mrt_get_denoise_adaptive(self._ctx, C.byref(on)), "mrt_get_denoise_adaptive")
        return bool(on.value)

    def set_denoise_mix(self, enabled: bool, gain: Optional[float] = None):
        """The blend of the filtered with the accumulated image behind every denoise of an accumulation (off by default); gain
        None keeps the State's (0.25 .. 16; the default is denoise_mix_default()'s)."""
        p = _lib.MrtDenoiseMix()
        self._check(self._L.mrt_get_denoise_mix(self._ctx, C.byref(p)), "mrt_get_denoise_mix")
        p.enabled = int(bool(enabled))
        if gain is not None:
            p.gain = gain
        self._check(self._L.mrt_set_denoise_mix(self._ctx, C.byref(p)), "mrt_set_denoise_mix")

    def denoise_mix(self) -> Tuple[bool, float]:
        """(enabled, gain) as set_denoise_mix left them."""
        p = _lib.MrtDenoiseMix()
        self._check(self._L.mrt_get_denoise_mix(self._ctx, C.byref(p)), "mrt_get_denoise_mix")
        return bool(p.enabled), float(p.gain)

    def debug_load_accumulation(self, rgba=None, S=None, tile_frames=None):
        """Overwrite what read_framebuffer (rgba (H, W, 4) f32), read_noise (S (H, W) f32) and tile_frames (one u32 per tile;
        makes the accumulation adaptive) read; None leaves a part as it is.  World 1 only."""
        h, w = self.args.height, self.args.width
        rgba = None if rgba is None else np.ascontiguousarray(rgba, np.float32)
        S = None if S is None else np.ascontiguousarray(S, np.float32)
        tf = None if tile_frames is None else np.ascontiguousarray(tile_frames, np.uint32).reshape(-1)
        assert rgba is None or rgba.shape == (h, w, 4)
        assert S is None or S.shape == (h, w)
        assert tf is None or tf.size == ((w + 7) // 8) * ((h + 7) // 8)
        self._check(self._L.mrt_debug_load_accumulation(self._ctx, None if rgba is None else rgba.ctypes.data,
                                                        None if S is None else S.ctypes.data, None if tf is None else tf.ctypes.data),
                    "mrt_debug_load_accumulation")

    def read_denoised(self) -> np.ndarray:
        """The most recent frame, denoised: (H, W, 4) f32, row 0 = bottom.  Needs noise tracking and world == 1; waits for the
        frames in flight, as read_framebuffer does."""
        out = np.empty((self.args.height, self.args.width, 4), np.float32)
        self._check(self._L.mrt_read_denoised(self._ctx, out.ctypes.data, out.size), "mrt_read_denoised")
        return out

    # -- diagnostic views (include/myraytracer_amd.h, "diagnostic views"): the noise estimate, the per-tile frame counts and the
    #    first-hit guides as an image, through read_view() or present(view=True)
    def set_view(self, kind: str = "noise_rel", ramp: str = "heat", lo: float = 0.0, hi: float = 0.1, rel_floor: Optional[float] = None):
        """mrt_set_view: what read_view() and present(view=True) show.  kind: "noise_se", "noise_rel", "tile_frames", "depth"
        (scalars, mapped from lo..hi through ramp "grey" -- unclamped -- or "heat"), "normal", "albedo", "sphere".  rel_floor
        None keeps the State's (the default is render_until's floor)."""
        if kind not in _lib.VIEW_KINDS or ramp not in _lib.VIEW_RAMPS:
            raise ValueError(f"set_view: kind {kind!r} ({', '.join(_lib.VIEW_KINDS)}), ramp {ramp!r} ({', '.join(_lib.VIEW_RAMPS)})")
        p = _lib.MrtView()
        self._check(self._L.mrt_get_view(self._ctx, C.byref(p)), "mrt_get_view")
        p.kind, p.ramp, p.lo, p.hi = _lib.VIEW_KINDS[kind], _lib.VIEW_RAMPS[ramp], lo, hi
        if rel_floor is not None:
            p.rel_floor = rel_floor
        self._check(self._L.mrt_set_view(self._ctx, C.byref(p)), "mrt_set_view")

    def view(self) -> dict:
        """The view as set_view left it: kind and ramp by name, lo, hi, rel_floor."""
        p = _lib.MrtView()
        self._check(self._L.mrt_get_view(self._ctx, C.byref(p)), "mrt_get_view")
        return view_dict(p)

    def read_view(self) -> np.ndarray:
        """The current view of the most recent frame: (H, W, 4) f32, row 0 = bottom.  World 1 only; the noise kinds need noise
        tracking; waits for the frames in flight, as read_denoised does."""
        out = np.empty((self.args.height, self.args.width, 4), np.float32)
        self._check(self._L.mrt_read_view(self._ctx, out.ctypes.data, out.size), "mrt_read_view")
        return out

    def debug_read_guides(self) -> dict:
        """The denoiser's guides (rebuilt first if stale), row 0 = bottom: rays (H, W, 6), index (H, W) i32, t (H, W),
        normal (H, W, 3), albedo (H, W, 3)."""
        h, w = self.args.height, self.args.width
        g = {"rays": np.empty((h, w, 6), np.float32), "index": np.empty((h, w), np.int32), "t": np.empty((h, w), np.float32),
             "normal": np.empty((h, w, 3), np.float32), "albedo": np.empty((h, w, 3), np.float32)}
        self._check(self._L.mrt_debug_read_guides(self._ctx, g["rays"].ctypes.data, g["index"].ctypes.data, g["t"].ctypes.data,
                                                  g["normal"].ctypes.data, g["albedo"].ctypes.data, h * w), "mrt_debug_read_guides")
        return g

    def debug_denoise(self, rgba: np.ndarray, S: np.ndarray, K: float, guides: dict, params: Optional[dict] = None,
                      variance: int = 0) -> np.ndarray:
        """The filter on caller-supplied buffers, synchronously: rgba (rows, W, 4) f32, S (rows, W) f32, guides as
        debug_read_guides returns them (index, t, normal, albedo); params: fields over the State's parameters; variance: 0
        accumulated (mrt_debug_denoise), 1 prefiltered, 2 prefiltered with the spatial initial variance (K ignored)."""
        rgba = np.ascontiguousarray(rgba, np.float32)
        S = np.ascontiguousarray(S, np.float32)
        rows, width = S.shape
        assert rgba.shape == (rows, width, 4)
        g = pack_guides(guides)
        assert g.shape == (rows, width, 8)
        p = _lib.MrtDenoiseParams()
        self._check(self._L.mrt_get_denoise_params(self._ctx, C.byref(p)), "mrt_get_denoise_params")
        for k, v in (params or {}).items():
            setattr(p, k, v)
        out = np.empty_like(rgba)
        if variance == 0:
            self._check(self._L.mrt_debug_denoise(self._ctx, rgba.ctypes.data, S.ctypes.data, K, g.ctypes.data, width, rows, C.byref(p),
                                                  out.ctypes.data), "mrt_debug_denoise")
        else:
            self._check(self._L.mrt_debug_denoise_variance(self._ctx, rgba.ctypes.data, S.ctypes.data, K, g.ctypes.data, width, rows,
                                                           C.byref(p), variance, out.ctypes.data), "mrt_debug_denoise_variance")
        return out

    def debug_denoise_mix(self, rgba: np.ndarray, S: np.ndarray, K: float, guides: dict, params: Optional[dict] = None,
                          variance: int = 0, enabled: bool = True, gain: Optional[float] = None) -> np.ndarray:
        """debug_denoise with the blend (mrt_debug_denoise_mix): gain None is the default's; with the blend on K is read in
        every variance."""
        rgba = np.ascontiguousarray(rgba, np.float32)
        S = np.ascontiguousarray(S, np.float32)
        rows, width = S.shape
        assert rgba.shape == (rows, width, 4)
        g = pack_guides(guides)
        assert g.shape == (rows, width, 8)
        p = _lib.MrtDenoiseParams()
        self._check(self._L.mrt_get_denoise_params(self._ctx, C.byref(p)), "mrt_get_denoise_params")
        for k, v in (params or {}).items():
            setattr(p, k, v)
        m = _lib.MrtDenoiseMix()
        self._L.mrt_denoise_mix_default(C.byref(m))
        m.enabled = int(bool(enabled))
        if gain is not None:
            m.gain = gain
        out = np.empty_like(rgba)
        self._check(self._L.mrt_debug_denoise_mix(self._ctx, rgba.ctypes.data, S.ctypes.data, K, g.ctypes.data, width, rows, C.byref(p),
                                                  variance, C.byref(m), out.ctypes.data), "mrt_debug_denoise_mix")
        return out

    # -- temporal reprojection (include/myraytracer_amd.h, "temporal reprojection"): a per-pixel history that follows the spheres'
    #    and the camera's motion, for a moving scene rendered with max_framebuffer_weight 0
    def set_temporal(self, enabled: bool, **params):
        """Turn temporal reprojection on / off; params: max_history, spatial_len, depth_tol over the current ones."""
        p = _lib.MrtTemporalParams()
        self._check(self._L.mrt_get_temporal(self._ctx, None, C.byref(p)), "mrt_get_temporal")
        for k, v in params.items():
            if k not in TEMPORAL_FIELDS:
                raise ValueError(f"set_temporal: unknown field {k!r} ({', '.join(TEMPORAL_FIELDS)})")
            setattr(p, k, v)
        self._check(self._L.mrt_set_temporal(self._ctx, int(enabled), C.byref(p)), "mrt_set_temporal")

    def temporal(self) -> Tuple[bool, dict]:
        """(enabled, parameters)."""
        on, p = C.c_int(), _lib.MrtTemporalParams()
        self._check(self._L.mrt_get_temporal(self._ctx, C.byref(on), C.byref(p)), "mrt_get_temporal")
        return bool(on.value), temporal_params_dict(p)

    def temporal_step(self):
        """Integrate the newest frame into the history (asynchronous)."""
        self._check(self._L.mrt_temporal_step(self._ctx), "mrt_temporal_step")

    def temporal_reset(self):
        self._check(self._L.mrt_temporal_reset(self._ctx), "mrt_temporal_reset")

    def read_temporal(self) -> np.ndarray:
        """The temporal image: (H, W, 4) f32, row 0 = bottom; waits for the frames in flight, as read_framebuffer does."""
        out = np.empty((self.args.height, self.args.width, 4), np.float32)
        self._check(self._L.mrt_read_temporal(self._ctx, out.ctypes.data, out.size), "mrt_read_temporal")
        return out

    def debug_read_temporal(self, n_spheres: int) -> dict:
        """The history the next step reads: h0 (H, W, 4) = (r, g, b, len), h1 (H, W, 4) = (m1, m2, t, index bits), and the
        previous spheres prev_xyzr (n_spheres, 4)."""
        h, w = self.args.height, self.args.width
        d = {"h0": np.empty((h, w, 4), np.float32), "h1": np.empty((h, w, 4), np.float32),
             "prev_xyzr": np.empty((n_spheres, 4), np.float32)}
        self._check(self._L.mrt_debug_read_temporal(self._ctx, d["h0"].ctypes.data, d["h1"].ctypes.data, d["prev_xyzr"].ctypes.data,
                                                    max(h * w, n_spheres)), "mrt_debug_read_temporal")
        return d

    def debug_load_temporal(self, h0=None, h1=None, prev_xyzr=None, prev_cam: Optional[MrtCameraRaw] = None):
        """Overwrite the history the next step reads, the previous spheres and / or the previous derived camera."""
        h0 = None if h0 is None else np.ascontiguousarray(h0, np.float32)
        h1 = None if h1 is None else np.ascontiguousarray(h1, np.float32)
        px = None if prev_xyzr is None else np.ascontiguousarray(prev_xyzr, np.float32).reshape(-1, 4)
        for a in (h0, h1):
            assert a is None or a.shape == (self.args.height, self.args.width, 4)
        self._check(self._L.mrt_debug_load_temporal(self._ctx, None if h0 is None else h0.ctypes.data, None if h1 is None else h1.ctypes.data,
                                                    None if px is None else px.ctypes.data, 0 if px is None else len(px),
                                                    None if prev_cam is None else C.byref(prev_cam)), "mrt_debug_load_temporal")

    # -- the temporal response ("temporal reprojection", steps 4b and 4c): a fast-history clamp and an anti-lag rule for what moves
    #    behind the first hit
    def set_temporal_response(self, enabled: bool, **numbers):
        """Turn the response on / off; numbers: fast_history, clamp_sigma, antilag over the current ones.  A change of `enabled`
        drops the history."""
        p = _lib.MrtTemporalResponse()
        self._check(self._L.mrt_get_temporal_response(self._ctx, C.byref(p)), "mrt_get_temporal_response")
        for k, v in numbers.items():
            if k not in RESPONSE_FIELDS:
                raise ValueError(f"set_temporal_response: unknown field {k!r} ({', '.join(RESPONSE_FIELDS)})")
            setattr(p, k, v)
        p.enabled = int(bool(enabled))
        self._check(self._L.mrt_set_temporal_response(self._ctx, C.byref(p)), "mrt_set_temporal_response")

    def temporal_response(self) -> Tuple[bool, dict]:
        """(enabled, numbers)."""
        p = _lib.MrtTemporalResponse()
        self._check(self._L.mrt_get_temporal_response(self._ctx, C.byref(p)), "mrt_get_temporal_response")
        return bool(p.enabled), temporal_response_dict(p)

    def debug_read_temporal_fast(self) -> np.ndarray:
        """The fast history the next step reads: h2 (H, W, 4) = (fr, fg, fb, valid)."""
        out = np.empty((self.args.height, self.args.width, 4), np.float32)
        self._check(self._L.mrt_debug_read_temporal_fast(self._ctx, out.ctypes.data, out.shape[0] * out.shape[1]), "mrt_debug_read_temporal_fast")
        return out

    def debug_load_temporal_fast(self, h2):
        """Overwrite the fast history the next step reads."""
        h2 = np.ascontiguousarray(h2, np.float32)
        assert h2.shape == (self.args.height, self.args.width, 4)
        self._check(self._L.mrt_debug_load_temporal_fast(self._ctx, h2.ctypes.data), "mrt_debug_load_temporal_fast")


TEMPORAL_FIELDS = ("max_history", "spatial_len", "depth_tol")
RESPONSE_FIELDS = ("fast_history", "clamp_sigma", "antilag")


def temporal_params_dict(p) -> dict:
    return {k: (float(getattr(p, k)) if k == "depth_tol" else int(getattr(p, k))) for k in TEMPORAL_FIELDS}


def temporal_params_default() -> dict:
    """mrt_temporal_params_default as a dict (host only)."""
    p = _lib.MrtTemporalParams()
    _lib.load().mrt_temporal_params_default(C.byref(p))
    return temporal_params_dict(p)


DENOISE_FIELDS = ("iterations", "sigma_l", "normal_exp", "sigma_z", "sigma_a")
DENOISE_VARIANCE_MODES = ("accumulated", "prefiltered", "spatial-early")          # MRT_DENOISE_VAR_*


def denoise_params_dict(p) -> dict:
    return {k: (float(getattr(p, k)) if k.startswith("sigma") else int(getattr(p, k))) for k in DENOISE_FIELDS}


def denoise_params_default() -> dict:
    """mrt_denoise_params_default as a dict (host only)."""
    p = _lib.MrtDenoiseParams()
    _lib.load().mrt_denoise_params_default(C.byref(p))
    return denoise_params_dict(p)


def view_dict(p) -> dict:
    kinds = {v: k for k, v in _lib.VIEW_KINDS.items()}
    ramps = {v: k for k, v in _lib.VIEW_RAMPS.items()}
    return {"kind": kinds[p.kind], "ramp": ramps[p.ramp], "lo": float(p.lo), "hi": float(p.hi), "rel_floor": float(p.rel_floor)}


def view_default() -> dict:
    p = _lib.MrtView()
    _lib.load().mrt_view_default(C.byref(p))
    return view_dict(p)


def denoise_mix_default() -> dict:
    """mrt_denoise_mix_default as a dict (host only; enabled is 0)."""
    p = _lib.MrtDenoiseMix()
    _lib.load().mrt_denoise_mix_default(C.byref(p))
    return {"enabled": int(p.enabled), "gain": float(p.gain)}


def pack_guides(guides: dict) -> np.ndarray:
    """{index, t, normal, albedo} -> (rows, W, 8) f32 {normal, t, albedo, index bits}: the layout mrt_debug_denoise reads."""
    idx = np.ascontiguousarray(guides["index"], np.int32)
    g = np.empty(idx.shape + (8,), np.float32)
    g[..., 0:3] = guides["normal"]
    g[..., 3] = guides["t"]
    g[..., 4:7] = guides["albedo"]
    g[..., 7] = idx.view(np.float32)
    return g


def noise_report_dict(r) -> dict:
    d = {k: getattr(r, k) for k, _ in _lib.MrtNoiseReport._fields_ if not k.startswith("reserved")}
    for k in ("seq", "frames_done", "pixels", "non_finite", "above"):
        d[k] = int(d[k])
    for k in ("threshold", "floor", "noise_factor", "sum_var", "sum_lum", "rmse", "rel_rmse", "max_se"):
        d[k] = float(d[k])
    return d


def budget_result_dict(r) -> dict:
    d = {k: int(getattr(r, k)) for k in ("used_seq", "tile_frames", "tiles", "frames")}
    d.update(var_before=float(r.var_before), var_after=float(r.var_after))
    return d


def noise_factor(frames_done: int, max_w: float) -> float:
    """K after frames_done uninterrupted frames with mrt_frame_weight's weights (+inf for fewer than 2)."""
    return float(_lib.load().mrt_noise_factor(frames_done, max_w))


def gather(states: Sequence[State], root: int = 0):
    """mrt_gather: one process, len(states) contexts (states[i] = shard i of n); the full frame lands on states[root]."""
    L = _lib.load()
    arr = (C.c_void_p * len(states))(*[s._ctx for s in states])
    st = L.mrt_gather(arr, len(states), root)
    if st:
        ctx = states[root]._ctx if 0 <= root < len(states) else None
        raise MrtError(st, "mrt_gather", (L.mrt_last_error(ctx) or b"").decode())


def srgb8_thresholds() -> np.ndarray:
    """The present pass's table (host): t[k], k = 1..255, the smallest float32 v with mrt_srgb8(v) >= k; t[0] = -inf."""
    out = np.empty(256, np.float32)
    st = _lib.load().mrt_debug_srgb8_thresholds(out.ctypes.data_as(C.POINTER(C.c_float)))
    if st:
        raise MrtError(st, "mrt_debug_srgb8_thresholds")
    return out


def shard_global_row(local_row: int, rank: int, world: int) -> int:
    return int(_lib.load().mrt_shard_global_row(local_row, rank, world))


def shard_local_rows(height: int, world: int) -> int:
    return int(_lib.load().mrt_shard_local_rows(height, world))


def unshard_rows(gathered: np.ndarray, height: int) -> np.ndarray:
    """Host un-permute (mrt_unshard_rows): [world, local_rows, W, 4] rank-major -> [height, W, 4]."""
    gathered = np.ascontiguousarray(gathered, np.float32)
    world, lrows, width, _ = gathered.shape
    assert lrows == shard_local_rows(height, world)
    out = np.zeros((height, width, 4), np.float32)
    st = _lib.load().mrt_unshard_rows(gathered.ctypes.data, world, width, height, out.ctypes.data)
    if st:
        raise MrtError(st, "mrt_unshard_rows")
    return out


def temporal_response_dict(p) -> dict:
    return {k: (int(getattr(p, k)) if k == "fast_history" else float(getattr(p, k))) for k in RESPONSE_FIELDS}


def temporal_response_default() -> dict:
    """mrt_temporal_response_default's numbers as a dict (host only; enabled is 0)."""
    p = _lib.MrtTemporalResponse()
    _lib.load().mrt_temporal_response_default(C.byref(p))
    return temporal_response_dict(p)
