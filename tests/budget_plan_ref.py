"""Host reference of the budget allocation on the device (include/myraytracer_amd.h, "budget allocation on the device"), in numpy:
mrt_budget_allocate's definition restated as ONE total order over the candidates, the blocked variance sums, and the target rule
of mrt_render_planned.

The order.  Candidate (t, j), j = 0 .. max_frames - 1, has the key (class, G, j, t):
    class 0 = mandatory: n_t + j < 2 and j < min(2, max_frames); G = 0
    class 1 = gain:      G = the bits of g'(t, j) as an unsigned 64-bit integer, complemented
g'(t, j) is the running minimum from j = m_t (the tile's mandatory frames) of s'_t * (K(n_t + j) - K(n_t + j + 1)) -- one
difference, one product, in double --, which stops at the first value that is not > 0; only tiles with s'_t > 0, s'_t finite and
n_t + m_t >= 2 have gain candidates; s'_t = s[t], a NaN or a negative value read as 0.  A positive finite double orders as its
bits, so ascending keys are "mandatory by j then t, then g' descending, j ascending, t ascending".  The keys are unique; the
allocation is the `budget` smallest (all if there are fewer); k_t = the number of those that belong to tile t.

The sums.  a_t = s'_t * K(n_t) for var_before and s'_t * K(n_t + k_t) for var_after, +0.0 for a tile with n_t < 2; P_b = the
sequential sum from 0.0 of a_t over t = 64 b .. 64 b + 63, ascending; the field = the sequential sum from 0.0 of P_b, b ascending.

The target rule.  A plan is a target: tile t should reach n_q[t] + k_t frames; k'_t = max(0, n_q[t] + k_t - n_now[t])."""
import numpy as np

import budget_ref

BLOCK = 64


def clean(s) -> np.ndarray:
    s = np.asarray(s, np.float32).ravel()
    with np.errstate(invalid="ignore"):
        return np.where(s >= np.float32(0), s.astype(np.float64), 0.0)


def counts(n, tiles: int) -> np.ndarray:
    """n as one int64 per tile: a scalar is the uniform accumulation's frame count"""
    n = np.asarray(n, np.int64)
    return np.full(tiles, int(n), np.int64) if n.ndim == 0 else n.ravel()


def keys(s, n, max_w: float, max_frames: int):
    """every candidate's (cls, G, j, t), unsorted"""
    sc = clean(s)
    T, M = sc.size, max_frames
    n = counts(n, T)
    K = budget_ref.k_values(int(n.max()) + M + 1, max_w)
    m = np.where(n < 2, np.minimum(2 - n, M), 0)
    j = np.arange(M)[None, :]
    mandatory = j < m[:, None]                                          # n_t + j < 2 and j < min(2, M)
    with np.errstate(all="ignore"):
        g = sc[:, None] * (K[n[:, None] + j] - K[n[:, None] + j + 1])   # (inf - inf where n_t + j < 2: masked below)
        g = np.where(mandatory, np.inf, g)
        g = np.minimum.accumulate(g, axis=1)                            # from j = m_t: the entries before it are +inf
        alive = np.logical_and.accumulate(np.where(mandatory, True, g > 0.0), axis=1)      # stops at the first value not > 0
    gains = (~mandatory) & alive & ((sc > 0.0) & np.isfinite(sc) & (n + m >= 2))[:, None]
    tt = np.broadcast_to(np.arange(T)[:, None], (T, M))
    jj = np.broadcast_to(j, (T, M))
    G = ~np.ascontiguousarray(g).view(np.uint64)
    cls = np.concatenate([np.zeros(int(mandatory.sum()), np.int64), np.ones(int(gains.sum()), np.int64)])
    Gs = np.concatenate([np.zeros(int(mandatory.sum()), np.uint64), G[gains]])
    return cls, Gs, np.concatenate([jj[mandatory], jj[gains]]), np.concatenate([tt[mandatory], tt[gains]])


def blocked_sums(s, n, k, max_w: float):
    """(var_before, var_after) in the blocked order"""
    sc = clean(s)
    n = counts(n, sc.size)
    k = np.asarray(k, np.int64).ravel()
    K = budget_ref.k_values(int((n + k).max()), max_w)
    out = []
    for add in (np.zeros_like(k), k):
        with np.errstate(all="ignore"):
            a = np.where(n >= 2, sc * K[n + add], 0.0)
        # every block's chain at once: a last block's missing tiles add +0.0, which changes no sum that started at +0.0
        pad = np.zeros(-(-a.size // BLOCK) * BLOCK, np.float64)
        pad[:a.size] = a
        pad = pad.reshape(-1, BLOCK)
        P = np.zeros(pad.shape[0], np.float64)
        with np.errstate(all="ignore"):
            for i in range(BLOCK):
                P = P + pad[:, i]
            total = 0.0
            for p in P:
                total = total + float(p)
        out.append(total)
    return out[0], out[1]


def order(s, n, max_w: float, max_frames: int) -> dict:
    """the candidates in ascending key order: {t: their tiles, mandatory: how many are mandatory, all: how many there are,
    tie: a budget that cuts through the largest group of equal gains, or None where no two gains are equal}"""
    cls, G, j, t = keys(s, n, max_w, max_frames)
    o = np.lexsort((t, j, G, cls))
    cls, G, t = cls[o], G[o], t[o]
    tie = None
    gain = np.nonzero(cls == 1)[0]
    if gain.size >= 2:
        first = int(gain[0])
        starts = np.concatenate([[0], np.nonzero(np.diff(G[first:]) != 0)[0] + 1, [G.size - first]])
        run = np.diff(starts)
        if run.max() >= 2:
            i = int(run.argmax())
            tie = first + int(starts[i]) + int(run[i]) // 2
    return {"t": t, "mandatory": int((cls == 0).sum()), "all": int(cls.size), "tie": tie}


def budgets(ordered: dict) -> list:
    """the budgets worth a case: 0 and 1; around the mandatory count; a cut through a group of equal gains; around the
    candidate count; 2^40"""
    o = ordered
    b = {0, 1, o["mandatory"] - 1, o["mandatory"], o["mandatory"] + 1, o["all"] - 1, o["all"], o["all"] + 7, 1 << 40}
    if o["tie"] is not None:
        b.add(o["tie"])
    return sorted(x for x in b if x >= 0)


def plan(s, n, max_w: float, budget: int, max_frames: int, ordered: dict = None):
    """(k as uint32 in s's shape, {tile_frames, tiles, frames, var_before, var_after}): the `budget` smallest keys"""
    shape = np.shape(s)
    ordered = order(s, n, max_w, max_frames) if ordered is None else ordered
    k = np.bincount(ordered["t"][:budget], minlength=int(np.prod(shape, dtype=np.int64))).astype(np.uint32)
    before, after = blocked_sums(s, n, k, max_w)
    res = {"tile_frames": int(k.sum()), "tiles": int((k > 0).sum()), "frames": int(k.max(initial=0)), "var_before": before, "var_after": after}
    return k.reshape(shape), res


DIGITS = 13                                                 # of a key: G's eight bytes from the top, j, t's four bytes from the top


def sort_keys(keys):
    """(G, lo) of keys()'s candidates in ascending key order, lo = (j << 32) | t; a mandatory candidate's G is 0 and a gain's has
    its top bit set, so the class needs no part of its own"""
    _, G, j, t = keys
    lo = (np.asarray(j, np.uint64) << np.uint64(32)) | np.asarray(t, np.uint64)
    o = np.lexsort((lo, G))
    return G[o], lo[o]


def digits_of(G, lo) -> list:
    """the thirteen 8-bit digits of the key (G, j, t), most significant first"""
    G, lo = int(G), int(lo)
    return list(G.to_bytes(8, "big")) + [lo >> 32] + list((lo & 0xFFFFFFFF).to_bytes(4, "big"))


def replay(keys, budget: int) -> dict:
    """What a selection of the `budget` smallest keys by 8-bit digits, most significant first, goes through -- said from the
    sorted keys, not by selecting: {mode, T, q, bins}.
        mode "none": budget 0 or no candidate; "all": no more candidates than the budget; "bin": T = the budget-th smallest key
        T    that key as (G, (j << 32) | t), or None
        q    the digit at which the selection ends: the first at which the next larger key differs from T -- from there on every
             key that shares T's digits 0 .. q is taken, the bin is taken whole (keys are unique: q <= 12)
        bins T's digits 0 .. q: the bin the selection descends into at each digit it looks at
    keys: keys()'s tuple, or sort_keys()'s pair for several budgets of one map.  It only says what a case exercises: the expected
    allocation is mrt_budget_allocate's."""
    G, lo = keys if len(keys) == 2 else sort_keys(keys)
    if budget == 0 or G.size == 0:
        return {"mode": "none", "T": None, "q": None, "bins": []}
    if budget >= G.size:
        return {"mode": "all", "T": None, "q": None, "bins": []}
    T, nxt = digits_of(G[budget - 1], lo[budget - 1]), digits_of(G[budget], lo[budget])
    q = next(i for i in range(DIGITS) if T[i] != nxt[i])
    return {"mode": "bin", "T": (int(G[budget - 1]), int(lo[budget - 1])), "q": q, "bins": T[:q + 1]}


def target(n_q, k, n_now) -> np.ndarray:
    """k' = max(0, n_q + k - n_now): what is left of a plan whose tiles have had frames since its query"""
    k = np.asarray(k, np.int64)
    left = counts(n_q, k.size).reshape(k.shape) + k - counts(n_now, k.size).reshape(k.shape)
    return np.maximum(left, 0).astype(np.uint32)
