"""The ordering of mrt_regroup_spheres (include/myraytracer_amd.h; myraytracer_amd/csrc/regroup.hip), restated in numpy: the
definition the device reproduces bit for bit, plus what the tests derive from a regrouped member_index.

The pool clusters are the clusters [0, n_pool) of the hierarchy (those build_clusters made from the spheres that may share a
cluster); `real` marks the member slots that hold a sphere.  pref[k] = real slots of the pool clusters [0, k).  The pooled
spheres, ascending by index, are cut kd fashion -- but at pref[] of power-of-two blocks of CLUSTERS, not at a sphere count --
sorting each part stably by the integer key of the f32 coordinate along the axis of its largest extent; the spheres at ranks
[pref[k], pref[k + 1]) then fill cluster k's real slots in ascending index.  Nothing else moves.

regroup(..., variant=...) also holds three references broken on purpose (tests/test_regroup_host.py shows that the tests reject
them): "float" sorts by float compare (-0.0 ties with +0.0), "median" cuts at the sphere median instead of pref, "index" breaks
ties by sphere index instead of keeping the previous depth's order."""
import numpy as np

INFLATE = 1.015


def keys_of(x):
    """the total order of float32 as uint32: -0.0 before +0.0"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return u ^ np.where(u >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def real_slots(h):
    """which of the hierarchy's member slots hold a sphere (h: the dict of refit_ref)"""
    mem = h["nodes"][:h["n_members"]]
    return ~(np.isinf(mem[:, 3]) & (mem[:, 3] > 0))


def pool_layout(real, n_pool):
    """-> (pref, the pool clusters' real-slot mask (n_pool, 4))"""
    rp = np.asarray(real[:4 * n_pool], bool).reshape(n_pool, 4)
    return np.concatenate([[0], np.cumsum(rp.sum(1))]).astype(np.int64), rp


def widest_axis(c):
    """the first axis with the largest f32 extent (strict >) of the float32 centres c (m, 3)"""
    ext = c.max(0) - c.min(0)
    q = 0
    for k in (1, 2):
        if ext[k] > ext[q]:
            q = k
    return q


def regroup(midx, real, n_pool, xyz, variant="", splits=None):
    """the regrouped member_index.  midx, real: per member slot; xyz: (n, 3) float32 centres by sphere index.
    splits (a list): every split made is appended as (a, a + half, b, axis), in clusters."""
    midx = np.asarray(midx, np.uint32)
    out = midx.copy()
    if n_pool <= 1:
        return out
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    pref, rp = pool_layout(real, n_pool)
    order = np.sort(midx[:4 * n_pool][rp.ravel()]).astype(np.int64)

    def split(a, b, size, r0, r1):
        if b - a <= 1:
            return
        half = size // 2
        if b - a <= half:
            split(a, b, half, r0, r1)
            return
        S = order[r0:r1]
        c = xyz[S]
        q = widest_axis(c)
        if variant == "float":
            perm = np.argsort(c[:, q], kind="stable")
        elif variant == "index":
            perm = np.lexsort((S, keys_of(c[:, q])))
        else:
            perm = np.argsort(keys_of(c[:, q]), kind="stable")
        order[r0:r1] = S[perm]
        mid = (r0 + r1) // 2 if variant == "median" else int(pref[a + half])
        if splits is not None:
            splits.append((a, a + half, b, q))
        split(a, a + half, half, r0, mid)
        split(a + half, b, half, mid, r1)

    size = 1 << (n_pool - 1).bit_length()
    split(0, n_pool, size, 0, int(pref[n_pool]))
    for k in range(n_pool):
        slots = 4 * k + np.nonzero(rp[k])[0]
        out[slots] = np.sort(order[pref[k]:pref[k + 1]])
    return out


def regroup_by_depths(midx, real, n_pool, xyz):
    """the same ordering the way the device computes it: depth by depth, all segments of a depth by ONE sort on the composite key
    (segment, key, rank) -- the claim regroup.hip rests on"""
    midx = np.asarray(midx, np.uint32)
    out = midx.copy()
    if n_pool <= 1:
        return out
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    pref, rp = pool_layout(real, n_pool)
    order = np.sort(midx[:4 * n_pool][rp.ravel()]).astype(np.int64)
    clus = np.repeat(np.arange(n_pool), np.diff(pref))
    rank = np.arange(len(order), dtype=np.uint64)
    size = 1 << (n_pool - 1).bit_length()
    while size >= 2:
        seg = clus // size
        key = np.zeros(len(order), np.uint64)
        for s in range((n_pool + size - 1) // size):
            if min(n_pool, (s + 1) * size) - s * size <= size // 2:
                continue
            sel = seg == s
            c = xyz[order[sel]]
            key[sel] = keys_of(c[:, widest_axis(c)])
        comp = (seg.astype(np.uint64) << np.uint64(52)) | (key << np.uint64(20)) | rank
        order = order[(np.sort(comp) & np.uint64(0xFFFFF)).astype(np.int64)]
        size //= 2
    for k in range(n_pool):
        out[4 * k + np.nonzero(rp[k])[0]] = np.sort(order[pref[k]:pref[k + 1]])
    return out


def check_alignment(midx, real, n_pool, xyz):
    """from the regrouped member_index alone: at every split of the recursion, along the axis of the part's largest extent, the
    largest key of the left clusters' spheres is <= the smallest of the right clusters'.  -> the number of splits checked"""
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
    pref, rp = pool_layout(real, n_pool)
    by_cluster = [np.asarray(midx[4 * k:4 * k + 4], np.int64)[rp[k]] for k in range(n_pool)]
    count = 0

    def split(a, b, size):
        nonlocal count
        if b - a <= 1:
            return
        half = size // 2
        if b - a <= half:
            split(a, b, half)
            return
        left, right = np.concatenate(by_cluster[a:a + half]), np.concatenate(by_cluster[a + half:b])
        q = widest_axis(xyz[np.concatenate([left, right])])
        kl, kr = keys_of(xyz[left, q]), keys_of(xyz[right, q])
        assert kl.max() <= kr.min(), f"split of clusters [{a}, {a + half}, {b}) along axis {q}: left key {kl.max():#x} > right key {kr.min():#x}"
        count += 1
        split(a, a + half, half)
        split(a + half, b, half)

    if n_pool > 1:
        split(0, n_pool, 1 << (n_pool - 1).bit_length())
    return count


def check_permutation(before, after, real, n_pool):
    """`after` permutes the pooled spheres over the real slots of the pool clusters, ascending within a cluster, and leaves every
    other slot (alone clusters, padding, direct slots, never-hit slots) as it was"""
    before, after = np.asarray(before, np.uint32), np.asarray(after, np.uint32)
    _, rp = pool_layout(real, n_pool)
    mask = np.zeros(len(before), bool)
    mask[:4 * n_pool] = rp.ravel()
    assert np.array_equal(before[~mask], after[~mask]), "a slot outside the pool's real slots changed"
    assert np.array_equal(np.sort(before[mask]), np.sort(after[mask])), "the pool's real slots do not hold a permutation of the pool"
    for k in range(n_pool):
        m = after[4 * k:4 * k + 4][rp[k]]
        assert (np.diff(m.astype(np.int64)) > 0).all(), f"cluster {k}: members not ascending by index"


def _node_bound(c, r):
    """build_hierarchy's bound of the spheres (c float64 (m, 3), r (m,)): the f32 centre of their common box, the enclosing radius"""
    ctr = (0.5 * ((c - r[:, None]).min(0) + (c + r[:, None]).max(0))).astype(np.float32)
    return ctr, float((np.linalg.norm(c - ctr.astype(np.float64), axis=1) + r).max())


def with_members(h, midx, xyzr):
    """a copy of the hierarchy h (refit_ref's dict) with member_index replaced and its level-0 records and every level's bounding
    spheres recomputed in float64 for the spheres xyzr (boxes, operand and the device's copies are dropped)"""
    xyzr = np.asarray(xyzr, np.float32).reshape(-1, 4)
    c, r = xyzr[:, :3].astype(np.float64), np.abs(xyzr[:, 3].astype(np.float64))
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in h.items()
           if k not in ("boxes", "boxes_open", "mfma", "reach", "spheres", "shade", "centres", "radii", "direct", "direct_index")}
    real = real_slots(h)
    midx = np.asarray(midx, np.uint32)
    out["midx"] = midx.copy()
    nodes = out["nodes"]
    nodes[:h["n_members"]][real] = np.concatenate([xyzr[midx[real], :3], -(xyzr[midx[real], 3:4] * xyzr[midx[real], 3:4])], axis=1)
    n_hier = h["direct_first"] if h["n_direct"] else h["n_members"]
    for k in range(1, h["levels"] + 1):
        if k == h["levels"]:
            recs = out["top"]
        else:
            end = h["level_base"][k + 1] if k + 1 < h["levels"] else len(nodes)
            recs = nodes[h["level_base"][k]:end]
        for j in range(len(recs)):
            lo, hi = min(n_hier, j * 4 ** k), min(n_hier, (j + 1) * 4 ** k)
            ids = midx[lo:hi][real[lo:hi]]
            if len(ids) == 0:
                recs[j] = (0.0, 0.0, 0.0, np.inf)
                continue
            ctr, R = _node_bound(c[ids], r[ids])
            Rf = np.nextafter(np.float32(R * INFLATE), np.float32(np.inf))
            recs[j] = (ctr[0], ctr[1], ctr[2], -(np.float64(Rf) ** 2))
            if -np.float64(recs[j][3]) < np.float64(Rf) ** 2:          # (the square was rounded down)
                recs[j][3] = np.nextafter(recs[j][3], np.float32(-np.inf))
    return out


def sum_r2(midx, real, n_hier, levels, xyzr):
    """[sum over the nodes of level k of R^2, k = 1 .. levels]: R the enclosing radius (not inflated) of build_hierarchy's bound"""
    xyzr = np.asarray(xyzr, np.float32).reshape(-1, 4)
    c, r = xyzr[:, :3].astype(np.float64), np.abs(xyzr[:, 3].astype(np.float64))
    midx = np.asarray(midx, np.int64)
    out = []
    for k in range(1, levels + 1):
        span, total = 4 ** k, 0.0
        for lo in range(0, n_hier, span):
            ids = midx[lo:lo + span][:n_hier - lo][real[lo:lo + span][:n_hier - lo]]
            if len(ids):
                total += _node_bound(c[ids], r[ids])[1] ** 2
        out.append(total)
    return out
