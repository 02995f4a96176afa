"""The matrix-core sweep's scaled space (hierarchy.cpp build_sweep_operand / scaled_top_records / choose_sweep_axes), checked
without a GPU through mrt_debug_build_sweep: x' = D (x - origin), D = diag of 1, 2 or 4 chosen per scene, the top level's bounds
re-made there as spheres around the scaled members.  What DESIGN.md §4 claims of it: D = I is today's operand byte for byte; D
follows the scene's flat axis and nothing else; every bound encloses its scaled members with the 1.015 margin; and the kernel's
test, restated in f32 with the bf16-split operands the host uploads, accepts the cluster of every member that the reference's
discriminant could accept."""
import ctypes as C

import numpy as np
import pytest

from myraytracer_amd import _lib
from test_hierarchy_host import INFLATE, bf16, bf16_round, build, scenes, split3

EPS = 2.0 ** -24


def build_sweep(mrt, sc, axis=None):
    L = _lib.load()
    sc = np.ascontiguousarray(sc, mrt.SPHERE_DTYPE)
    h = build(mrt, sc, 4, 0)
    force = (C.c_float * 3)(*axis) if axis is not None else None
    ax, org = (C.c_float * 3)(), (C.c_float * 3)()
    reach = C.c_double()
    rec = np.zeros((len(h["top"]), 4), np.float32)
    mf = np.zeros(len(h["top"]) // 32 * 512, np.uint16)
    assert L.mrt_debug_build_sweep(sc.ctypes.data, len(sc), force, ax, rec.ctypes.data, len(rec), mf.ctypes.data, len(mf), org,
                                   C.byref(reach)) == 0
    return dict(h=h, axis=np.array(list(ax), np.float64), origin=np.array(list(org), np.float64), rec=rec, mfma=mf, reach=reach.value)


def swap_axes(sc, a, b):
    out = sc.copy()
    c = np.asarray(sc["center"]).copy()
    c[:, [a, b]] = c[:, [b, a]]
    out["center"] = c
    return out


def blob(mrt, n=400, seed=4):
    """spheres filling a cube: no flat axis"""
    rng = np.random.default_rng(seed)
    sc = np.zeros(n, mrt.SPHERE_DTYPE)
    for i in range(n):
        sc[i] = (tuple(rng.uniform(-6, 6, 3)), float(rng.uniform(0.15, 0.4)), 1, (0.5, 0.5, 0.5), 0.0)
    return sc


def test_identity_reproduces_the_world_space_operand_byte_for_byte(mrt):
    """D = I, forced or chosen, gives the very operand, origin and reach of the world-space build: such scenes render through
    exactly the bytes and kernel arguments they had before the sweep had a space of its own."""
    for name, sc in list(scenes(mrt)) + [("blob", blob(mrt))]:
        s = build_sweep(mrt, sc, (1, 1, 1))
        h = s["h"]
        assert np.array_equal(s["mfma"], h["mfma"]), name
        assert np.array_equal(s["origin"], h["origin"]), name
        c = np.asarray(sc["center"], np.float64).reshape(-1, 3)
        r = np.abs(np.asarray(sc["radius"], np.float64))
        world_reach = float((np.linalg.norm(c - h["origin"], axis=1) + r).max()) if len(sc) else 0.0
        assert abs(s["reach"] - world_reach) <= 1e-12 * max(world_reach, 1.0), name
        auto = build_sweep(mrt, sc)
        if (auto["axis"] == 1).all():
            assert np.array_equal(auto["mfma"], h["mfma"]) and auto["reach"] == s["reach"], name


def test_the_choice_follows_the_scenes_flat_axis_and_only_that(mrt):
    cover = mrt.scene_cover(1, True)[0]
    assert build_sweep(mrt, cover)["axis"].tolist() == [1, 2, 1]
    assert build_sweep(mrt, swap_axes(cover, 0, 1))["axis"].tolist() == [2, 1, 1]
    assert build_sweep(mrt, swap_axes(cover, 2, 1))["axis"].tolist() == [1, 1, 2]
    assert build_sweep(mrt, blob(mrt))["axis"].tolist() == [1, 1, 1]
    assert build_sweep(mrt, mrt.scene_default())["axis"].tolist() == [1, 1, 1]          # too few spheres to matter
    # hierarchies of more than one level keep the world's space: their walk has the boxes
    big = build_sweep(mrt, mrt.scene_stress(3, 40)[0])
    assert big["h"]["levels"] > 1 and big["axis"].tolist() == [1, 1, 1]
    # the choice is a function of the spheres: the same scene gives the same D and bytes, whatever was built in between
    again = build_sweep(mrt, cover)
    assert np.array_equal(again["mfma"], build_sweep(mrt, cover)["mfma"])


AXES = [(1, 2, 1), (2, 1, 1), (1, 1, 4), (2, 2, 1), (4, 1, 2)]


def members_of(h, sc):
    """(top record of every real hierarchy member, its index in the scene)"""
    n_hier = h["direct_first"] if h["n_direct"] else h["n_members"]
    real = ~np.isinf(h["nodes"][:n_hier, 3])
    slot = np.arange(n_hier)[real]
    return slot // 4 ** h["levels"], h["midx"][:n_hier][real]


def test_every_scaled_bound_encloses_its_scaled_members_with_the_margin(mrt):
    """R' >= 1.015 x the farthest point of any scaled member (an ellipsoid with semi-axes r D) from the record's f32 centre:
    points all over every member's surface, among them the directions in which an ellipsoid reaches furthest."""
    rng = np.random.default_rng(21)
    u = rng.normal(size=(600, 3))
    u = np.concatenate([u, np.eye(3), -np.eye(3)])
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for name, sc in [("cover", mrt.scene_cover(1, True)[0]), ("default", mrt.scene_default()), ("stress 40x40", mrt.scene_stress(3, 40)[0])]:
        c = np.asarray(sc["center"], np.float64).reshape(-1, 3)
        r = np.abs(np.asarray(sc["radius"], np.float64))
        for axis in AXES:
            s = build_sweep(mrt, sc, axis)
            D = s["axis"]
            assert D.tolist() == list(axis)
            rec_of, idx = members_of(s["h"], sc)
            rec = s["rec"].astype(np.float64)
            assert np.isfinite(rec[np.unique(rec_of), 3]).all(), name
            assert np.isinf(rec[np.setdiff1d(np.arange(len(rec)), rec_of), 3]).all(), name      # padding stays never-hit
            ctr = (c[idx] - s["origin"]) * D - rec[rec_of, :3]
            # toward the far side the farthest point lies near D^2 p: add those directions per member
            far = np.zeros(len(idx))
            for dirs in (u[None], (ctr * D * D / np.maximum(np.linalg.norm(ctr * D * D, axis=1, keepdims=True), 1e-300))[:, None, :]):
                pts = ctr[:, None, :] + r[idx][:, None, None] * dirs * D
                far = np.maximum(far, np.linalg.norm(pts, axis=-1).max(1))
            R = np.sqrt(-rec[rec_of, 3])
            assert (R >= INFLATE * far * (1 - 1e-6)).all(), (name, axis, float((R / far).min()))
            # ... and not wastefully: never beyond the plain bound max_m(|p_m| + r_m max D) of the record's members
            plain = np.zeros(len(rec))
            np.maximum.at(plain, rec_of, np.linalg.norm(ctr, axis=1) + r[idx] * D.max())
            assert (np.sqrt(-rec[np.unique(rec_of), 3]) <= INFLATE * plain[np.unique(rec_of)] * (1 + 1e-6)).all(), (name, axis)


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def fma32(a, b, c):
    """fmaf on float32 arrays (the product is exact in float64; the one extra rounding of the sum is 2^-29 relative)"""
    return f32(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def dot32(a, b):
    """rt_math.h dot3"""
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], f32(a[..., 0] * b[..., 0])))


def rays_for(rng, c, r, org, reach, n):
    """origins and unit directions, float32: camera-like (one far origin), bounces off sphere surfaces, origins inside bounds,
    and rays grazing the scene's flat directions"""
    k = rng.integers(0, len(c), n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = c[k] + u * r[k, None]                                                  # on a sphere's surface
    d = rng.normal(size=(n, 3))
    q = n // 4
    cam = org + np.array([0.9, 0.15, 0.25]) * reach                            # a camera beside the scene
    o[:q] = cam + rng.normal(size=(q, 3)) * 0.05
    d[:q] = c[rng.integers(0, len(c), q)] + rng.normal(size=(q, 3)) * 0.5 - o[:q]
    o[q:q + q // 2] = c[k[q:q + q // 2]] + u[q:q + q // 2] * r[k[q:q + q // 2], None] * rng.uniform(0, 1, (q // 2, 1))   # inside
    g = slice(q + q // 2, 2 * q)                                                # grazing: nearly in a coordinate plane
    dg = d[g]
    dg[np.arange(len(dg)), rng.integers(0, 3, len(dg))] *= 0.02
    d[g] = dg
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o32, d32 = f32(o), f32(d)
    d32 = f32(d32 / np.sqrt(dot32(d32, d32).astype(np.float64))[:, None])      # unit to an ulp, as normalize() leaves them
    return o32, d32


@pytest.mark.parametrize("scene", ["cover", "default", "stress 40x40"])
def test_the_scaled_sweep_accepts_every_cluster_the_reference_could_hit(mrt, scene):
    """For random rays and every member whose reference discriminant b b - a c (f32, shader.wgsl:277-282) is >= 0 -- or within its
    own rounding error 14 eps |oc|^2 of that, which covers every way the reference could round it -- and that does not lie entirely
    behind the origin (b < 0 or c < 0), the kernel's test accepts the member's top record: the ray operands formed as kernels.hip
    forms them (o' = D (o - origin), D d, v_rsq_f32, the stretch), the A operand as uploaded, bf16 pieces multiplied exactly and
    accumulated in f32 in k order (and, independently, exactly).  |g| <= 1/2 and the admission test o'.o' <= (4 reach)^2 hold."""
    L = _lib.load()
    rng = np.random.default_rng(33)
    sc = dict(cover=mrt.scene_cover(1, True)[0], default=mrt.scene_default(), **{"stress 40x40": mrt.scene_stress(3, 40)[0]})[scene]
    c = np.asarray(sc["center"], np.float64).reshape(-1, 3)
    r = np.abs(np.asarray(sc["radius"], np.float64))
    c32, nr2 = np.asarray(sc["center"], np.float32).reshape(-1, 3), -(np.asarray(sc["radius"], np.float32) ** 2)
    tested = 0
    for axis in [None] + AXES:
        s = build_sweep(mrt, sc, axis)
        D, org = s["axis"], s["origin"]
        D32, org32 = f32(D), f32(org)
        rec_of, idx = members_of(s["h"], sc)
        n_top = len(s["rec"])
        A = bf16(s["mfma"].reshape(-1, 2, 32, 8))
        A = np.concatenate([A[:, 0], A[:, 1]], axis=-1).reshape(-1, 16)         # rows in the operand's order
        order = np.array([32 * t + 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3) for t in range(n_top // 32) for m in range(32)])
        row_of = np.empty(n_top, np.int64)
        row_of[order] = np.arange(n_top)
        scale = (C.c_float * 4)()
        pair = C.c_uint32()
        assert L.mrt_debug_mfma_scale(s["reach"], scale, C.byref(pair)) == 0
        s_ds, s_2k2, s_nk2slack, o2_max = (np.float32(v) for v in scale)
        neg_k2 = np.array([(pair.value & 0xFFFF) << 16], np.uint32).view(np.float32)[0]
        o, d = rays_for(rng, c, r, org, s["reach"] / D.max(), 480)
        # the ray, as the kernel's call site forms it
        o_rel = f32(o - org32) * D32                                            # a power of two: exact
        if (D != 1).any():
            dd = d * D32
            unit = f32(f32(1.0 / np.sqrt(dot32(dd, dd).astype(np.float64))) * s_ds)
            ds = f32(dd * unit[:, None])
        else:
            ds = f32(d * s_ds)
        o2 = dot32(o_rel, o_rel)
        assert (o2 <= o2_max).all(), (scene, axis)
        nk0 = f32(-dot32(o_rel, ds))
        k1p = f32(o2 * s_nk2slack)

        def pack(v, w, tail):
            hi = bf16_round(v)
            lo = bf16_round(v - hi)
            w0, w1, w2 = split3(w)
            t3 = np.full((len(v), 3), tail, np.float32)
            return np.concatenate([hi, lo, hi, np.stack([w0, w1, w2], 1), t3, np.zeros((len(v), 1), np.float32)], 1).astype(np.float64)
        B1, B2 = pack(ds, nk0, 0.0), pack(f32(o_rel * s_2k2), k1p, neg_k2)

        def gemm32(A, B, acc):                                                  # f32 accumulation in k order
            for k in range(16):
                acc = f32(acc.astype(np.float64) + A[:, None, k] * B[None, :, k])
            return acc
        g = gemm32(A, B1, np.zeros((len(A), len(B1)), np.float32))
        real = np.isfinite(s["rec"][order, 3])
        assert np.abs(g[real]).max() <= 0.5, (scene, axis)
        cand32 = ~(gemm32(A, B2, np.clip(f32(g * np.abs(g)), 0, 1).astype(np.float32)) < 0)
        g64 = A @ B1.T
        cand64 = ~(A @ B2.T + np.clip(g64 * np.abs(g64), 0.0, 1.0) < 0)
        # the reference's discriminant per (member, ray), in f32 as the kernel's exact test evaluates it
        oc = o[None, :, :] - c32[idx][:, None, :]
        a = dot32(d, d)[None, :]
        b = dot32(oc, np.broadcast_to(d[None], oc.shape))
        cq = fma32(oc[..., 2], oc[..., 2], fma32(oc[..., 1], oc[..., 1], fma32(oc[..., 0], oc[..., 0], np.broadcast_to(nr2[idx][:, None], b.shape))))
        disc = fma32(b, b, -f32(a * cq))
        oc2 = (oc.astype(np.float64) ** 2).sum(-1)
        could = ~(disc.astype(np.float64) < -14 * EPS * oc2) & ((b < 0) | (cq < 0))
        rows = row_of[rec_of]
        missed32 = could & ~cand32[rows]
        missed64 = could & ~cand64[rows]
        assert not missed32.any() and not missed64.any(), (scene, axis, int(missed32.sum()), int(missed64.sum()))
        assert not cand32[~real].any() and not cand64[~real].any(), (scene, axis)      # padding records are never candidates
        assert could.sum() > 100 and (~cand32[real]).sum() > 0, (scene, axis)          # both outcomes occur
        tested += int(could.sum())
    assert tested > 1000
