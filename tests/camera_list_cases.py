"""The cases the camera-list tests share (tests/test_camera_list_host.py on the CPU, tests/test_gpu_camera_list.py on the GPU): scene,
camera, image shape, the host's hierarchy and the reference's lists, computed once per case; with `rays` also sampled camera rays
of every texel and the oracle's `required` set."""
import numpy as np

import camera_list_ref as L
import camera_mask_ref as R
from common import to_oracle_spheres

_cache = {}
OVERFLOW_SHAPE = (24, 16)
OVERFLOW_PIXEL = (12, 8)                        # its axis carries the column of spheres
OVERFLOW_ENTRY = (OVERFLOW_PIXEL[1] * OVERFLOW_SHAPE[0] + OVERFLOW_PIXEL[0]) >> 3


def overflow_scene(M):
    """Pinhole at the origin, 24x16: twelve tiny spheres behind one another on the axis through the middle of pixel (12, 8), each
    well inside that pixel's patch (angular radius 0.01 of a pixel side of 0.125), so that the pixel's entry -- and no other --
    holds twelve members, more than the cap of 8; a ground sphere (direct) and a few spheres elsewhere."""
    W, H = OVERFLOW_SHAPE
    ps = 2.0 / H
    axis = np.array([((OVERFLOW_PIXEL[0] + 0.5) - 0.5 * W) * ps + 0.5 * ps, ((OVERFLOW_PIXEL[1] + 0.5) - 0.5 * H) * ps + 0.5 * ps, -1.0])
    s = 2.0 + 0.5 * np.arange(12)
    others = np.array([[-0.9, 0.0, -2.0, 0.3], [0.9, -0.2, -2.5, 0.25], [-0.3, 0.5, -3.0, 0.2], [0.5, 0.6, -4.0, 0.35]])
    sc = np.zeros(1 + len(s) + len(others), M.SPHERE_DTYPE)
    sc["center"][0] = (0.0, -100.5, -1.0)
    sc["radius"][0] = 100.0
    sc["center"][1:1 + len(s)] = (s[:, None] * axis[None]).astype(np.float32)
    sc["radius"][1:1 + len(s)] = (0.01 * s).astype(np.float32)
    sc["center"][1 + len(s):] = others[:, :3]
    sc["radius"][1 + len(s):] = others[:, 3]
    sc["material_ty"] = 1
    sc["albedo"] = 0.5
    sc["albedo"][1:1 + len(s)] = (0.9, 0.2, 0.2)
    return sc


def scene_of(M, name):
    """(spheres, Camera or None)"""
    if name == "cover-glass":                   # the cover scene with glass under its own thin-lens camera
        return M.scene_cover(1, True)
    if name == "cover-pinhole":                 # ... and with the lens closed
        sc, cam = M.scene_cover(1, True)
        cam.defocus_angle_deg = 0.0
        return sc, cam
    if name == "default":                       # the reference's 4-sphere scene under its pinhole at the origin
        return M.scene_default(), None
    if name == "overflow":
        return overflow_scene(M), None
    raise KeyError(name)


def case(M, O, name, W, H, rays=False, per_texel=6):
    key = (name, W, H, rays)
    if key in _cache:
        return _cache[key]
    sc, cam = scene_of(M, name)
    raw = M.camera_derive(cam) if cam is not None else None
    members, index, n_top, direct_first = R.host_hierarchy(M, sc)
    n_slots = min(4 * n_top, direct_first, len(members))
    out = dict(name=name, sc=sc, cam=cam, raw=raw, W=W, H=H, members=members, index=index, n_top=n_top, direct_first=direct_first,
               n_slots=n_slots, lists=L.camera_lists_ref(members, n_top, direct_first, raw, W, H),
               slot_of=L.slot_of_sphere(index, n_slots, members, len(sc)))
    if rays:
        n_tex = R.local_texels(W, H)
        px, py = R.texel_pixels(n_tex, W)
        tex = np.nonzero(py < H)[0]
        r, ray_tex = R.camera_rays(raw, W, H, tex, px[tex], py[tex], np.random.default_rng(29), per_texel)
        _, _, _, required = O.world_hit_batch(O.pack_world(to_oracle_spheres(O, sc)), r)
        out.update(rays=r, ray_tex=ray_tex, required=required)
    _cache[key] = out
    return out
