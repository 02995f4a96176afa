"""A float64 checker for a hierarchy -- the host builder's (mrt_debug_build_hierarchy / mrt_debug_build_boxes_top_down) or the
device's after mrt_update_spheres (mrt_debug_read_hierarchy) -- against a list of spheres.  It restates what
tests/test_hierarchy_host.py demands of the host builder, and checks the 24-byte box form the kernel reads directly.

h: a dict with levels, top (n_top, 4), nodes (n_nodes, 4), midx, n_members, n_direct, direct_first, level_base, and optionally
boxes / boxes_open (n, 6: the kernel's top-down numbering) with box_kc and box_quad, mfma (the A operand) with origin, reach,
direct / direct_index (the kernel arguments' records), spheres / shade / centres / radii (the device's copies of the geometry).
xyzr: (n, 4) float32 -- centre and (signed) radius of every sphere.  Every check raises AssertionError naming what failed."""
import numpy as np

INFLATE = 1.015          # mrt_internal.h kBoundInflate
SLACK = 2.0 ** -13       # hierarchy.h kMfmaSlack
EPS = 2.0 ** -24


def bf16(u16):
    return (np.asarray(u16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_bits(x):
    """round-to-nearest-even of float32 values to bf16, as the 16 bits"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def split3_bits(x):
    """a float32 as three bf16 pieces hi + mid + lo (pack_top_mfma's split of Ck)"""
    x = np.asarray(x, np.float32)
    a = bf16_bits(x)
    r1 = (x - bf16(a).astype(np.float32)).astype(np.float32)
    b = bf16_bits(r1)
    c = bf16_bits((r1 - bf16(b).astype(np.float32)).astype(np.float32))
    return a, b, c


def tile_order(n_top):
    """row m of tile t of the A operand is top record order[32 t + m]"""
    return np.array([32 * t + 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3) for t in range(n_top // 32) for m in range(32)], np.int64)


def _geometry(xyzr):
    xyzr = np.asarray(xyzr, np.float32).reshape(-1, 4)
    return xyzr, xyzr[:, :3].astype(np.float64), np.abs(xyzr[:, 3].astype(np.float64))


def _n_hier(h):
    return h["direct_first"] if h["n_direct"] else h["n_members"]


def _level_records(h, k):
    if k == h["levels"]:
        return h["top"]
    end = h["level_base"][k + 1] if k + 1 < h["levels"] else len(h["nodes"])
    return h["nodes"][h["level_base"][k]:end]


def _members_under(h, k, j, never0):
    span, n_hier = 4 ** k, _n_hier(h)
    lo, hi = min(n_hier, j * span), min(n_hier, (j + 1) * span)
    return h["midx"][lo:hi][~never0[lo:hi]]


def check_members(h, xyzr):
    xyzr, _, _ = _geometry(xyzr)
    mem = h["nodes"][:h["n_members"]]
    never = np.isinf(mem[:, 3]) & (mem[:, 3] > 0)
    real = h["midx"][~never]
    assert sorted(real.tolist()) == list(range(len(xyzr))), "members: every sphere must be a member (or direct) exactly once"
    want = np.concatenate([xyzr[real, :3], -(xyzr[real, 3:4] * xyzr[real, 3:4])], axis=1)
    bad = np.nonzero((mem[~never].view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, f"members: {len(bad)} member records are not (centre, -(r r)) of their sphere; first: slot of sphere {int(real[bad[0]])}"
    if h["n_direct"]:
        d = h["midx"][h["direct_first"]:h["direct_first"] + h["n_direct"]]
        assert not never[h["direct_first"]:h["direct_first"] + h["n_direct"]].any(), "members: a direct slot is never-hit"
        if "direct" in h:
            assert np.array_equal(np.asarray(h["direct_index"][:h["n_direct"]], np.uint32), d.astype(np.uint32)), "direct: indices"
            want = np.concatenate([xyzr[d, :3], -(xyzr[d, 3:4] * xyzr[d, 3:4])], axis=1)
            assert np.array_equal(h["direct"][:h["n_direct"]].view(np.uint32), want.view(np.uint32)), "direct: the kernel arguments' records are stale"


def check_copies(h, xyzr):
    xyzr, _, _ = _geometry(xyzr)
    want = np.concatenate([xyzr[:, :3], -(xyzr[:, 3:4] * xyzr[:, 3:4])], axis=1)
    assert np.array_equal(h["spheres"].view(np.uint32), want.view(np.uint32)), "copies: the exact-test records"
    assert np.array_equal(h["shade"][:, :4].view(np.uint32), xyzr.view(np.uint32)), "copies: the shade records' centre and radius"
    assert np.array_equal(h["centres"][:, :3].view(np.uint32), xyzr[:, :3].view(np.uint32)), "copies: the SoA's centres"
    assert np.array_equal(h["radii"].view(np.uint32), xyzr[:, 3].view(np.uint32)), "copies: the SoA's radii"


def check_bounds(h, xyzr):
    _, c, r = _geometry(xyzr)
    never0 = np.isinf(h["nodes"][:_n_hier(h), 3])
    for k in range(1, h["levels"] + 1):
        for j, rec in enumerate(_level_records(h, k)):
            ids = _members_under(h, k, j, never0)
            if len(ids) == 0:
                assert np.isinf(rec[3]) and rec[3] > 0, f"bounds: level {k} node {j} has no member and is not never-hit"
                continue
            assert np.isfinite(rec).all() and rec[3] <= 0, f"bounds: level {k} node {j} has members and no bound"
            R = np.sqrt(-np.float64(rec[3]))
            far = (np.linalg.norm(c[ids] - rec[:3].astype(np.float64), axis=1) + r[ids]).max()
            assert R >= INFLATE * far * (1 - 1e-6), f"bounds: level {k} node {j}: R {R} < {INFLATE} x {far}"


def check_boxes(h, xyzr):
    """the 24-byte boxes: (centre, e') with e' >= the enclosing extent (three roundings: 1 + 1e-6) + kpad, kpad = kc |e|^2 +
    4.4e-14 / kc (quadratic slack; kc >= 1.3e-6 / the smallest clustered radius) or 1.5e-3 |e|_1 (linear; kc = 1.5e-3)"""
    if "boxes" not in h or len(h["boxes"]) == 0:
        return
    _, c, r = _geometry(xyzr)
    boxes, kc, quad = h["boxes"], float(h["box_kc"]), bool(h["box_quad"])
    n_hier, n_top, levels = _n_hier(h), len(h["top"]), h["levels"]
    never0 = np.isinf(h["nodes"][:n_hier, 3])
    clustered = h["midx"][:n_hier][~never0]
    if quad:
        if len(clustered):
            assert kc >= 1.3e-6 / max(r[clustered].min(), 1e-30) * (1 - 1e-12), f"boxes: kc {kc} is below 1.3e-6 / the smallest radius {r[clustered].min()}"
    else:
        assert np.float32(kc) == np.float32(1.5e-3), "boxes: the linear form's kc"
    o = [n_top * (4 ** t - 1) // 3 for t in range(levels + 1)]
    assert len(boxes) == o[levels], "boxes: count"
    placed = np.zeros(len(boxes), bool)
    wide = h.get("boxes_open")
    for k in range(1, levels + 1):
        t = levels - k
        for j, rec in enumerate(_level_records(h, k)):
            g = o[t] + j
            placed[g] = True
            ids = _members_under(h, k, j, never0)
            if len(ids) == 0:
                assert (boxes[g, 3:6] < -1e38).all(), f"boxes: level {k} node {j} has no member and its box is not never-hit"
                continue
            ctr, e = boxes[g, :3].astype(np.float64), boxes[g, 3:6].astype(np.float64)
            need = (np.abs(c[ids] - ctr) + r[ids][:, None]).max(axis=0) * (1 + 1e-6)
            kpad = kc * float(need @ need) + 4.4e-14 / kc if quad else 1.5e-3 * float(need.sum())
            assert (e >= (need + kpad) * (1 - 1e-12)).all(), f"boxes: level {k} node {j}: extents {e} < enclosure {need} + kpad {kpad}"
            assert (e < 1e37).all(), f"boxes: level {k} node {j} is opened wide"
            if wide is not None:
                assert np.array_equal(wide[g, :3], boxes[g, :3]) and (wide[g, 3:6] == np.float32(3.0e37)).all(), f"boxes: the opened copy of level {k} node {j}"
    assert (boxes[~placed][:, 3:6] == np.float32(-3.0e38)).all(), "boxes: a slot without a node is not never-hit"
    if wide is not None:
        never = boxes[:, 3] < 0
        assert np.array_equal(wide[never].view(np.uint32), boxes[never].view(np.uint32)), "boxes: the opened copy's never-hit boxes"


def operand_rows(h):
    """(records in row order, the rows' 16 K slots as float64, Ck = the sum of its three pieces)"""
    top = h["top"]
    mf = np.asarray(h["mfma"]).reshape(-1, 2, 32, 8)
    k = np.concatenate([mf[:, 0], mf[:, 1]], axis=-1).reshape(-1, 16)
    return top[tile_order(len(top))], bf16(k), k


def check_operand(h):
    """the A operand restates the top records, relative to the origin, for D = I: C - origin split into bf16 hi + lo (hi twice),
    (1, 1, 1), Ck in three pieces and 0; Ck <= C.C - R^2 - 2^-13 (C.C + R^2) with R = the record's radius + 2 eps |C| (the rounding
    of C - origin, which the radius absorbs: pack_top_mfma), i.e. rounded DOWN"""
    rec, v, raw = operand_rows(h)
    org = np.asarray(h["origin"], np.float64)
    assert np.array_equal(v[:, 0:3], v[:, 3:6]) and (v[:, 9:12] == 1.0).all() and (raw[:, 15] == 0).all(), "operand: layout"
    crel = (rec[:, :3].astype(np.float64) - org).astype(np.float32).astype(np.float64)
    assert (np.abs(v[:, 0:3] + v[:, 6:9] - crel) <= 2.0 ** -16 * np.abs(crel) + 1e-300).all(), "operand: hi + lo is not C - origin"
    ck = v[:, 12:15].sum(axis=1)
    real = np.isfinite(rec[:, 3])
    assert (ck[~real] > 1e38).all(), "operand: a never-hit record's Ck"
    c2 = (crel[real] ** 2).sum(axis=1)
    R = np.sqrt(-rec[real, 3].astype(np.float64)) + 2.0 * EPS * np.sqrt(c2)
    R2 = R * R
    lim = c2 - R2 - SLACK * (c2 + R2)
    bad = np.nonzero(ck[real] > lim + 1e-13 * (c2 + R2))[0]
    assert len(bad) == 0, f"operand: Ck above C.C - R^2 - slack for {len(bad)} records (rounded up?); first row {int(np.nonzero(real)[0][bad[0]])}"
    assert (ck[real] >= lim - 0.01 * SLACK * (c2 + R2) - 1e-5 * (np.sqrt(c2 * R2) + R2)).all(), "operand: Ck gives away more than its slack"


def check_reach(h, xyzr):
    _, c, r = _geometry(xyzr)
    if len(c) == 0:
        return
    far = (np.linalg.norm(c - np.asarray(h["origin"], np.float64), axis=1) + r).max()
    assert h["reach"] >= far * (1 - 1e-12), f"reach {h['reach']} does not cover every sphere ({far})"


def check(h, xyzr):
    check_members(h, xyzr)
    if "spheres" in h:
        check_copies(h, xyzr)
    check_bounds(h, xyzr)
    check_boxes(h, xyzr)
    if "mfma" in h:
        check_operand(h)
    if "reach" in h:
        check_reach(h, xyzr)


def xyzr_of(spheres):
    """(n, 4) float32 from an array of the product's sphere dtype"""
    return np.concatenate([np.asarray(spheres["center"], np.float32).reshape(-1, 3), np.asarray(spheres["radius"], np.float32).reshape(-1, 1)], axis=1)
