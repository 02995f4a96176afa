"""The cases the camera-mask tests share (tests/test_camera_mask_host.py on the CPU, tests/test_gpu_camera_mask.py on the GPU): scene,
camera and image shape, and per case the sampled camera rays with the oracle's `required` set, computed once."""
import math

import numpy as np

import camera_mask_ref as R
from common import to_oracle_spheres

CASES = ("cover-glass", "wide-lens", "default-pinhole", "inside-a-cluster", "21x13", "corner-grazers")
_cache = {}


def scene_of(M, name):
    """(spheres, Camera or None, W, H)"""
    sc, cam = M.scene_cover(1, True)
    if name == "cover-glass":
        return sc, cam, 64, 36
    if name == "wide-lens":                     # lens radius 0.5 = tan(angle / 2) focus
        cam.defocus_angle_deg = math.degrees(2.0 * math.atan(0.5 / cam.focus_dist))
        return sc, cam, 64, 36
    if name == "default-pinhole":
        return M.scene_default(), None, 64, 36
    if name == "inside-a-cluster":              # the camera at the middle of a cluster's members, looking along the ground
        members, index, n_top, direct_first = R.host_hierarchy(M, sc)
        real = np.isfinite(members[: 4 * n_top, 3]).reshape(n_top, 4)
        m = int(np.nonzero(real.sum(1) >= 3)[0][len(np.nonzero(real.sum(1) >= 3)[0]) // 2])
        c = members[4 * m: 4 * m + 4][real[m], :3].astype(np.float64).mean(0)
        cam.lookfrom = (float(c[0]), float(c[1]) + 0.05, float(c[2]))
        cam.lookat = (0.0, 0.3, 0.0)
        cam.focus_dist = 3.0
        return sc, cam, 64, 36
    if name == "21x13":
        return sc, cam, 21, 13
    if name == "corner-grazers":
        # Pinhole, 64x36: small spheres that only the ray through the outer corner of an entry's first texel (jitter 0, 0) grazes
        # -- 0.002 deep, from the side away from the entry -- so that a patch radius 10 % short loses them: at depth 5 the corner
        # lies 0.196 h beyond such a patch, the spheres' own rounding allowance is 0.001.
        W, H, depth, r, deep = 64, 36, 5.0, 0.05, 0.002
        ps = 2.0 / H
        ent = np.arange(3, (W * H) // 8, 7)
        px, py = (8 * ent) % W, (8 * ent) // W
        d = np.stack([((px + 0.5) - 0.5 * W) * ps, ((py + 0.5) - 0.5 * H) * ps, -np.ones(len(ent))], 1)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        out = np.array([-1.0, -1.0, 0.0]) / math.sqrt(2.0)
        perp = out[None] - (d @ out)[:, None] * d
        perp /= np.linalg.norm(perp, axis=1, keepdims=True)
        sc = np.zeros(len(ent), M.SPHERE_DTYPE)
        sc["center"] = (depth * d + (r - deep) * perp).astype(np.float32)
        sc["radius"] = r
        sc["material_ty"] = 1
        sc["albedo"] = 0.5
        return sc, None, W, H
    raise KeyError(name)


def case(M, O, name, per_texel=6):
    """dict: scene, camera, shape, hierarchy, the sampled rays (every texel of the image), their texels and `required`"""
    if name in _cache:
        return _cache[name]
    sc, cam, W, H = scene_of(M, name)
    raw = M.camera_derive(cam) if cam is not None else None
    members, index, n_top, direct_first = R.host_hierarchy(M, sc)
    n_tex = R.local_texels(W, H)
    px, py = R.texel_pixels(n_tex, W)
    tex = np.nonzero(py < H)[0]
    rays, ray_tex = R.camera_rays(raw, W, H, tex, px[tex], py[tex], np.random.default_rng(17), per_texel)
    a2 = (rays[:, 3:].astype(np.float64) ** 2).sum(1)
    assert (np.abs(a2 - 1.0) < 5e-6).all()
    packed = O.pack_world(to_oracle_spheres(O, sc))
    _, _, _, required = O.world_hit_batch(packed, rays)
    out = dict(name=name, sc=sc, cam=cam, raw=raw, W=W, H=H, members=members, index=index, n_top=n_top, direct_first=direct_first,
               rays=rays, ray_tex=ray_tex, required=required,
               cluster_of=R.cluster_of_sphere(index, n_top, direct_first, members, len(sc)))
    _cache[name] = out
    return out
