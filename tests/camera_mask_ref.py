"""Reference of the camera-ray cluster masks (myraytracer_amd/csrc/cam_mask.hip), restated in numpy float64, and the camera rays
the render kernel generates, drawn with its own float32 arithmetic (kernels.hip: new_sample_head / new_sample_lens).

An entry covers 8 consecutive texels of the shard's row-major texel order; bit 31 - i of word w is top record 32 w + i.  A bit
must be set whenever any camera ray of any texel of the entry could have a reference discriminant >= 0 against a member of
that cluster (members 4 m .. 4 m + 3 of level 0), unless the member lies entirely behind the ray's origin.

The bound: a ray runs from O + off, |off| <= rho, through O + p, |p - pc| <= h (pc the centre of the texel's patch of the focal
plane, h its half diagonal); at the affine parameter s >= 0 it is within |1 - s| rho + s h of the axis point O + s pc.  A member
(centre C, radius r) is touched if for some s >= 0 the axis point is within R + |1 - s| rho + s h of C, with R = sqrt(r^2 + E) +
kappa, E = 28 x 2^-23 (|O - C| + rho)^2 the reference's own rounding (twice hierarchy.cpp's 14 eps |oc|^2 / a), and rho, h and the
positions widened by MARGIN relative: rho (1 + MARGIN), h (1 + MARGIN) + MARGIN |pc|, kappa = MARGIN (|O| + rho).
rho_scale / h_scale shrink rho / h for the mutation check of tests/test_camera_mask_host.py."""
import ctypes as C

import numpy as np

MARGIN = 1.0e-5
ROUND = 28.0 * 2.0 ** -23
BAND_ROWS = 8
MAX_RECORDS = 128


def host_hierarchy(M, spheres):
    """(level-0 member records [n_members, 4] float32, member_index, n_top, direct_first) as mrt_set_world builds them"""
    from myraytracer_amd import _lib
    L = _lib.load()
    sc = np.ascontiguousarray(spheres, M.SPHERE_DTYPE)
    info = (C.c_uint32 * 10)()
    assert L.mrt_debug_build_hierarchy(sc.ctypes.data, len(sc), 4, 0, None, 0, None, 0, None, 0, None, 0, None, info) == 0
    nodes = np.zeros((info[2], 4), np.float32)
    index = np.zeros(info[3], np.uint32)
    assert L.mrt_debug_build_hierarchy(sc.ctypes.data, len(sc), 4, 0, None, 0, nodes.ctypes.data, len(nodes), index.ctypes.data, len(index),
                                       None, 0, None, info) == 0
    assert info[0] == 1 and info[6] == 0, "a small scene has one level, level 0 first"
    return nodes[:info[3]], index, int(info[1]), int(info[5])


def camera_arrays(raw):
    """(O, su, sv, fw, ru, rv, defocus) as float32 arrays; raw = None or mode 0: the reference's pinhole at the origin"""
    if raw is None or raw.mode == 0:
        z = np.zeros(3, np.float32)
        return z, np.array([1, 0, 0], np.float32), np.array([0, 1, 0], np.float32), np.array([0, 0, 1], np.float32), z, z, False
    f = lambda a: np.array(list(a), np.float32)
    return f(raw.origin), f(raw.su), f(raw.sv), f(raw.fw), f(raw.ru), f(raw.rv), bool(raw.defocus)


def texel_pixels(n_texels, W, rank=0, world=1):
    """(px, global row py) of the shard's texels 0 .. n_texels - 1"""
    t = np.arange(n_texels, dtype=np.int64)
    lrow, px = t // W, t % W
    py = ((lrow // BAND_ROWS) * world + rank) * BAND_ROWS + lrow % BAND_ROWS
    return px, py


def local_texels(W, H, world=1):
    bands = (H + BAND_ROWS - 1) // BAND_ROWS
    return ((bands + world - 1) // world) * BAND_ROWS * W


def _touches(q, Q2, R, pc, P2, hp, rho):
    """q, Q2, R: [members]; pc [texels, 3], P2, hp: [texels] -> bool [texels, members]"""
    D = pc @ q.T
    a1, a2 = R + rho, R - rho
    b1, b2 = (hp - rho)[:, None], (hp + rho)[:, None]
    C1 = Q2 - a1 * a1
    A1, B1 = P2[:, None] - b1 * b1, D - a1 * b1
    hit = (C1 <= 0.0) | (A1 + 2.0 * B1 + C1 <= 0.0)
    hit |= (A1 > 0.0) & (B1 < 0.0) & (-B1 < A1) & (C1 * A1 <= B1 * B1)
    A2, B2, C2 = P2[:, None] - b2 * b2, D - a2 * b2, Q2 - a2 * a2
    hit |= (A2 <= 0.0) | ((-B2 > A2) & (C2 * A2 <= B2 * B2))
    return hit


def camera_masks_ref(members, n_top, direct_first, raw, W, H, rank=0, world=1, rho_scale=1.0, h_scale=1.0, only=None):
    """(entries, 4) uint32: the masks of shard `rank` of `world` of a W x H image; only: these entries alone (in that order)"""
    assert n_top <= MAX_RECORDS
    O, su, sv, fw, ru, rv, defocus = (np.asarray(a, np.float64) if not isinstance(a, bool) else a for a in camera_arrays(raw))
    rho = 0.0
    if defocus:
        rho = np.sqrt(max(ru @ ru, rv @ rv) + abs(ru @ rv)) * (1.0 + MARGIN) * rho_scale
    kappa = MARGIN * (np.linalg.norm(O) + rho)
    n_slots = min(4 * n_top, direct_first, len(members))
    m = np.asarray(members[:n_slots], np.float64)
    r2 = -m[:, 3]
    real = np.isfinite(r2) & (r2 >= 0.0)
    q = O[None] - m[:, :3]
    q[~real] = 0.0
    Q2 = (q * q).sum(1)
    oc = np.sqrt(Q2) + rho
    R = np.where(real, np.sqrt(np.where(real, r2, 0.0) + ROUND * oc * oc) + kappa, -1.0)
    n_tex = local_texels(W, H, world)
    entries = (n_tex + 7) // 8
    ids = np.arange(entries) if only is None else np.asarray(only, np.int64)
    entries = len(ids)
    tex = (8 * ids[:, None] + np.arange(8)[None]).reshape(-1)
    px, py = texel_pixels(8 * ((n_tex + 7) // 8), W, rank, world)
    px, py = px[tex], py[tex]
    valid = (tex < n_tex) & (py < H)
    ps = float(np.float32(2.0) / np.float32(H))
    half = 0.5 * ps
    vx = ((px + 0.5) - 0.5 * W) * ps + half
    vy = ((py + 0.5) - 0.5 * H) * ps + half
    pc = vx[:, None] * su[None] + vy[:, None] * sv[None] - fw[None]
    P2 = (pc * pc).sum(1)
    h = np.sqrt(half * half * (su @ su + sv @ sv + 2.0 * abs(su @ sv))) * h_scale
    hp = h * (1.0 + MARGIN) + MARGIN * np.sqrt(P2)
    hit = _touches(q, Q2, R, pc, P2, hp, rho) & real[None] & valid[:, None]          # [texels, slots]
    pad = np.zeros((hit.shape[0], 4 * MAX_RECORDS), bool)
    pad[:, :n_slots] = hit
    per_cluster = pad.reshape(entries, 8, MAX_RECORDS, 4).any(axis=(1, 3))             # [entries, 128]
    bits = per_cluster.reshape(entries, 4, 32).astype(np.uint64) << (31 - np.arange(32, dtype=np.uint64))
    return bits.sum(2).astype(np.uint32)


def mask_bits(masks):
    """[entries, 128] bool from the (entries, 4) words"""
    m = np.asarray(masks, np.uint32)
    return ((m[:, :, None] >> (31 - np.arange(32, dtype=np.uint32))) & 1).astype(bool).reshape(len(m), 128)


def cluster_of_sphere(index, n_top, direct_first, members, n_spheres):
    """cluster (top record) of every sphere that sits in the hierarchy, -1 for the direct spheres"""
    out = np.full(n_spheres, -1, np.int64)
    n_slots = min(4 * n_top, direct_first)
    for slot in range(n_slots):
        if np.isfinite(members[slot, 3]):
            out[index[slot]] = slot // 4
    return out


def _f32(x):
    return np.asarray(x, np.float32)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def camera_rays(raw, W, H, texels, px, py, rng, per_texel=6):
    """Camera rays of the given texels in the kernel's float32 arithmetic: per texel the four corner jitters (0 and the largest
    float below 1) with lens points on the rim, and random jitters / lens points.  -> (rays [n, 6] float32, texel of each)"""
    O, su, sv, fw, ru, rv, defocus = camera_arrays(raw)
    mode1 = raw is not None and raw.mode != 0
    top = np.float32(1.0 - 2.0 ** -24)
    n = len(texels)
    u = np.concatenate([np.tile(_f32([0, top, 0, top]), n), _f32(rng.integers(0, 2 ** 24, n * per_texel) * 2.0 ** -24)])
    v = np.concatenate([np.tile(_f32([0, 0, top, top]), n), _f32(rng.integers(0, 2 ** 24, n * per_texel) * 2.0 ** -24)])
    which = np.concatenate([np.repeat(np.arange(n), 4), np.repeat(np.arange(n), per_texel)])
    one, halfc = np.float32(1.0), np.float32(0.5)
    ps = np.float32(2.0) / np.float32(H)
    base_x = ((_f32(px[which]) + halfc) - halfc * np.float32(W)) * ps
    base_y = ((_f32(py[which]) + halfc) - halfc * np.float32(H)) * ps
    vx, vy = base_x + u * ps, base_y + v * ps
    k = len(which)
    if not mode1:
        o = np.zeros((k, 3), np.float32)
        nd = np.stack([vx, vy, np.full(k, -1.0, np.float32)], 1)
    else:
        p = (vx[:, None] * su[None] + vy[:, None] * sv[None]) - fw[None]
        o = np.repeat(O[None], k, 0)
        nd = p
        if defocus:
            # the kernel accepts a point of [-1, 1)^2 with fma(ly, ly, lx * lx) <= 1: rim points (snapped inside) and random ones
            ang = rng.uniform(0, 2 * np.pi, k)
            rad = np.where(rng.random(k) < 0.5, 1.0, np.sqrt(rng.random(k)))
            lx, ly = _f32(rad * np.cos(ang)), _f32(rad * np.sin(ang))
            for _ in range(4):
                out = _fma(ly, ly, lx * lx) > one
                lx = np.where(out, lx * np.float32(1.0 - 2.0 ** -23), lx)
                ly = np.where(out, ly * np.float32(1.0 - 2.0 ** -23), ly)
            assert not (_fma(ly, ly, lx * lx) > one).any()
            off = lx[:, None] * ru[None] + ly[:, None] * rv[None]
            o = o + off
            nd = p - off
    dd = _fma(nd[:, 2], nd[:, 2], _fma(nd[:, 1], nd[:, 1], nd[:, 0] * nd[:, 0]))
    d = nd / np.sqrt(dd)[:, None]
    return np.concatenate([o, d], 1).astype(np.float32), np.asarray(texels)[which]


def missing_pairs(masks, rays_texel, required, cluster_of):
    """(ray, sphere) pairs the oracle requires whose cluster is not set in the ray's entry"""
    bits = mask_bits(masks)
    ri, si = np.nonzero(required)
    cl = cluster_of[si]
    keep = cl >= 0
    ri, si, cl = ri[keep], si[keep], cl[keep]
    miss = ~bits[rays_texel[ri] >> 3, cl]
    return ri[miss], si[miss]
