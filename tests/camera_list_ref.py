"""Reference of the camera-ray sphere lists (myraytracer_amd/csrc/cam_mask.hip, the second table of the mask build), in numpy
float64: per entry of 8 consecutive texels of the shard's row-major order, the level-0 member slots whose bundle test
(camera_mask_ref._touches, the masks' own bound) passes for any valid texel of the entry.  The cluster bit of the masks is the OR of
its four members' answers.

The device's entry is 4 words: word 0 = the number of slots, at most CAP, or OVERFLOW for an entry with more; words 1 .. 3 = the
slot ids ascending, 10 bits each, id k at bits 10 k .. 10 k + 9 of the 96 bits (word 1 lowest)."""
import numpy as np

import camera_mask_ref as R

CAP = 8
OVERFLOW = 0xFFFFFFFF


def camera_lists_ref(members, n_top, direct_first, raw, W, H, rank=0, world=1, only=None):
    """bool [entries, slots]: slot s is on the list of entry e (before the cap); slots = the hierarchy's part of level 0"""
    assert n_top <= R.MAX_RECORDS
    O, su, sv, fw, ru, rv, defocus = (np.asarray(a, np.float64) if not isinstance(a, bool) else a for a in R.camera_arrays(raw))
    rho = np.sqrt(max(ru @ ru, rv @ rv) + abs(ru @ rv)) * (1.0 + R.MARGIN) if defocus else 0.0
    kappa = R.MARGIN * (np.linalg.norm(O) + rho)
    n_slots = min(4 * n_top, direct_first, len(members))
    m = np.asarray(members[:n_slots], np.float64)
    r2 = -m[:, 3]
    real = np.isfinite(r2) & (r2 >= 0.0)
    q = O[None] - m[:, :3]
    q[~real] = 0.0
    Q2 = (q * q).sum(1)
    oc = np.sqrt(Q2) + rho
    Rr = np.where(real, np.sqrt(np.where(real, r2, 0.0) + R.ROUND * oc * oc) + kappa, -1.0)
    n_tex = R.local_texels(W, H, world)
    ids = np.arange((n_tex + 7) // 8) if only is None else np.asarray(only, np.int64)
    tex = (8 * ids[:, None] + np.arange(8)[None]).reshape(-1)
    px, py = R.texel_pixels(8 * ((n_tex + 7) // 8), W, rank, world)
    px, py = px[tex], py[tex]
    valid = (tex < n_tex) & (py < H)
    ps = float(np.float32(2.0) / np.float32(H))
    half = 0.5 * ps
    vx = ((px + 0.5) - 0.5 * W) * ps + half
    vy = ((py + 0.5) - 0.5 * H) * ps + half
    pc = vx[:, None] * su[None] + vy[:, None] * sv[None] - fw[None]
    P2 = (pc * pc).sum(1)
    hp = np.sqrt(half * half * (su @ su + sv @ sv + 2.0 * abs(su @ sv))) * (1.0 + R.MARGIN) + R.MARGIN * np.sqrt(P2)
    hit = R._touches(q, Q2, Rr, pc, P2, hp, rho) & real[None] & valid[:, None]           # [texels, slots]
    return hit.reshape(len(ids), 8, n_slots).any(1)


def pack(on):
    """the device's (entries, 4) uint32 words of the bool [entries, slots] lists"""
    out = np.zeros((len(on), 4), np.uint32)
    for e, row in enumerate(np.asarray(on, bool)):
        slots = np.nonzero(row)[0]
        if len(slots) > CAP:
            out[e, 0] = OVERFLOW
            continue
        bits = sum(int(s) << (10 * k) for k, s in enumerate(slots))
        assert all(int(s) < 1024 for s in slots)
        out[e] = (len(slots), bits & 0xFFFFFFFF, (bits >> 32) & 0xFFFFFFFF, bits >> 64)
    return out


def unpack(words, n_slots):
    """(bool [entries, n_slots] lists, bool [entries] overflowed) of the device's words; an overflowed entry's list is empty"""
    w = np.asarray(words, np.uint32)
    on = np.zeros((len(w), n_slots), bool)
    over = w[:, 0] == OVERFLOW
    for e in np.nonzero(~over)[0]:
        cnt = int(w[e, 0])
        assert cnt <= CAP, (e, cnt)
        bits = int(w[e, 1]) | int(w[e, 2]) << 32 | int(w[e, 3]) << 64
        slots = [(bits >> (10 * k)) & 1023 for k in range(cnt)]
        assert slots == sorted(set(slots)) and bits >> (10 * cnt) == 0, (e, slots)
        on[e, slots] = True
    return on, over


def slot_of_sphere(index, n_slots, members, n_spheres):
    """member slot of every sphere that sits in the hierarchy, -1 for the direct spheres"""
    out = np.full(n_spheres, -1, np.int64)
    for slot in range(n_slots):
        if np.isfinite(members[slot, 3]):
            out[index[slot]] = slot
    return out


def missing_pairs(on, over, rays_texel, required, slot_of):
    """(ray, sphere) pairs the oracle requires whose slot is not on the list of the ray's entry (overflowed entries hold all)"""
    ri, si = np.nonzero(required)
    sl = slot_of[si]
    keep = sl >= 0
    ri, si, sl = ri[keep], si[keep], sl[keep]
    e = rays_texel[ri] >> 3
    miss = ~(on[e, sl] | over[e])
    return ri[miss], si[miss]
