"""Host reference of adaptive sampling by budget (include/myraytracer_amd.h, "adaptive sampling by budget"), in numpy float64:
the summed-S tile map of noise_query(tile_map="sum_s") in the summation order the header states, mrt_budget_allocate's
definition restated as a sort over the candidates, and the levels render_budget renders.  Bit for bit the library's."""
import numpy as np

import adaptive_ref
import noise_ref

TILE = 8


def _padded(S, fb):
    """(bands, tiles_x, 8 rows, 8 columns) float64: (double)S of a counted pixel -- S and lum(fb) finite --, +0.0 elsewhere and
    outside the image."""
    S = np.asarray(S, np.float32)
    h, w = S.shape
    tr, tx = -(-h // TILE), -(-w // TILE)
    with np.errstate(all="ignore"):
        counted = np.isfinite(S) & np.isfinite(noise_ref.lum(np.asarray(fb, np.float32)))
    pad = np.zeros((tr * TILE, tx * TILE), np.float64)
    pad[:h, :w] = np.where(counted, S.astype(np.float64), 0.0)
    return pad.reshape(tr, TILE, tx, TILE).transpose(0, 2, 1, 3)


def tile_sums(S, fb) -> np.ndarray:
    """The map of a MRT_TILE_MAP_SUM_S query, (tile rows, tiles_x) float32: per tile row ((p0 + p1) + (p2 + p3)) + ((p4 + p5) +
    (p6 + p7)), then the eight row sums one after the other from the bottom row (row 0), starting at 0.0; rounded to float."""
    p = _padded(S, fb)
    with np.errstate(all="ignore"):
        rows = ((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])) + ((p[..., 4] + p[..., 5]) + (p[..., 6] + p[..., 7]))
        m = np.zeros(rows.shape[:2], np.float64)
        for r in range(TILE):
            m = m + rows[..., r]
        return m.astype(np.float32)


def tile_sums_row_major(S, fb) -> np.ndarray:
    """The same 64 values of every tile added one after the other in row-major order: NOT the definition (the self-check of
    tests/test_budget_host.py: a fixture must tell the two orders apart)."""
    p = _padded(S, fb).reshape(-1, TILE * TILE)
    with np.errstate(all="ignore"):
        m = np.zeros(p.shape[0], np.float64)
        for i in range(TILE * TILE):
            m = m + p[:, i]
        return m.astype(np.float32)


def k_values(n_max: int, max_w: float) -> np.ndarray:
    """K(n) = mrt_noise_factor(n, max_w) for n = 0 .. n_max, float64 (+inf for n < 2)."""
    return np.array(adaptive_ref.k_table(n_max, max_w), np.float64)


def allocate(s, n, max_w: float, budget: int, max_frames: int):
    """mrt_budget_allocate: (k as uint32 in s's shape, {tile_frames, tiles, frames, var_before, var_after})."""
    shape = np.shape(s)
    s = np.asarray(s, np.float32).ravel()
    n = np.asarray(n, np.int64).ravel()
    assert s.shape == n.shape and 1 <= max_frames <= 32 and budget >= 0
    T, M = s.size, max_frames
    with np.errstate(invalid="ignore"):
        sc = np.where(s >= np.float32(0), s.astype(np.float64), 0.0)            # a NaN or a negative value reads as 0
    K = k_values(int(n.max()) + M + 1, max_w)
    m = np.where(n < 2, np.minimum(2 - n, M), 0)
    k = np.zeros(T, np.int64)
    left = budget
    # mandatory frames: j ascending, then t ascending, until the budget ends
    for j in range(min(2, M)):
        for t in np.nonzero(m > j)[0]:
            if left == 0:
                break
            k[t] += 1
            left -= 1
    if left:
        g, cj, ct = [], [], []
        for t in range(T):
            if not (sc[t] > 0.0) or np.isinf(sc[t]) or n[t] + m[t] < 2:
                continue
            js = np.arange(m[t], M)
            gains = np.minimum.accumulate(sc[t] * (K[n[t] + js] - K[n[t] + js + 1]))      # g': never increases with j
            keep = gains > 0.0
            g.extend(gains[keep])
            cj.extend(js[keep])
            ct.extend([t] * int(keep.sum()))
        g, cj, ct = np.array(g, np.float64), np.array(cj, np.int64), np.array(ct, np.int64)
        order = np.lexsort((ct, cj, -g))                    # g' descending, then j ascending, then t ascending
        for t in ct[order[:left]]:
            k[t] += 1
    before = after = 0.0
    for t in range(T):
        if n[t] >= 2:
            before += float(sc[t] * K[n[t]])
            after += float(sc[t] * K[n[t] + k[t]])
    res = {"tile_frames": int(k.sum()), "tiles": int((k > 0).sum()), "frames": int(k.max()), "var_before": before, "var_after": after}
    return k.astype(np.uint32).reshape(shape), res


def var_after(s, n, k, max_w: float) -> float:
    """The model's summed variance once tile t has had k[t] more frames: the allocation's var_after for any k."""
    s, n, k = np.asarray(s, np.float32).ravel(), np.asarray(n, np.int64).ravel(), np.asarray(k, np.int64).ravel()
    with np.errstate(invalid="ignore"):
        sc = np.where(s >= np.float32(0), s.astype(np.float64), 0.0)
    K = k_values(int((n + k).max()), max_w)
    return float(sum(float(sc[t] * K[n[t] + k[t]]) for t in range(s.size) if n[t] >= 2))


def levels(k):
    """render_budget's calls: [(tile ids ascending, run length)], L_j = {t : k_t >= j} with consecutive equal lists merged."""
    k = np.asarray(k, np.int64).ravel()
    out = []
    for j in range(1, int(k.max(initial=0)) + 1):
        L = np.nonzero(k >= j)[0].astype(np.uint32)
        if out and len(out[-1][0]) == len(L):
            out[-1] = (out[-1][0], out[-1][1] + 1)
        else:
            out.append((L, 1))
    return out


def map_fixture(h: int = 20, w: int = 44, seed: int = 7):
    """(S (h, w) f32, rgba (h, w, 4) f32) for the map tests.  S spans 40 binades inside every tile: most values lie near 2^-20,
    and every row of a tile holds one pair x, -x with |x| near 2^20 (a loaded S may be anything).  The large values cancel, so
    what the double additions rounded away beside them -- which depends on their order -- is a large part of the tile's sum and
    survives the rounding to float.  Some S are NaN or +inf, and one pixel has a non-finite colour (counted in nothing)."""
    rng = np.random.default_rng(seed)
    S = (rng.uniform(1.0, 2.0, (h, w)) * np.exp2(rng.integers(-22, -18, (h, w)))).astype(np.float32)
    big = (rng.uniform(1.0, 2.0, (h, w)) * np.exp2(rng.integers(18, 21, (h, w)))).astype(np.float32)
    for y in range(h):
        for x0 in range(0, w, TILE):                        # one pair in every row of every tile, at random columns of it
            a, b = x0 + rng.permutation(min(TILE, w - x0))[:2]
            S[y, a], S[y, b] = big[y, a], -big[y, a]
    S[3, 5] = np.nan
    S[9, 17] = np.inf
    S[h - 1, w - 1] = np.nan
    S[12, 40] = np.inf
    rgba = rng.uniform(0.05, 1.5, (h, w, 4)).astype(np.float32)
    rgba[..., 3] = 1
    rgba[6, 30, 1] = np.inf
    return S, rgba
