"""What "heaviest first" means for the tile queue, in plain numpy (no GPU, no library).

Written from the design text ("tile queue"; the head of csrc/tile_order.hip), not from the kernels: a tile's cost is
the largest number of bounce-loop trips any of its pixels took; the queue is a bucket sort of those costs, heaviest bucket first,
ties in any order.  The documented bucket key is the cost itself below 32, else a 5-bit exponent and the 5 bits below the leading
one -- monotone in the cost, 1,024 buckets at most.

check_order() never compares with one particular expected array (ties may land anywhere).  It holds three things:

  permutation  the order holds every member exactly once (members: range(n), or a subset frame's list);
  key          the documented key does not increase along the order;
  bound        whatever the buckets are, no entry is much heavier than one before it: for entries i before j,
               cost[j] <= cost[i] if cost[i] < 32, else cost[j] <= cost[i] + (cost[i] >> 5).  A bucket of exponent e is 2^(e-5)
               wide and every cost in it is at least 2^e, so a correct bucket sort of this resolution meets it; it is checked
               in one pass with a running minimum, in uint64 (2^32 - 1 is an input).

The cost inputs below are chosen to make those checks sharp: both edges of buckets over the whole exponent range, the values
around the exact / bucketed boundary, one bucket only (every lane of a wave in one ballot group), 64 distinct buckets per wave
(one group per lane), and orders that are already sorted either way."""
import numpy as np

TILE = 8
U32_MAX = 2 ** 32 - 1
N_KEYS = 28 * 32               # keys 0 .. 895: 32 exact costs, then 32 mantissas for each exponent 5 .. 31
FIXED_VALUES = (0, 1, 30, 31, 32, 33, 63, 64, 65, 2 ** 31, U32_MAX)


def key_of(cost):
    """The documented bucket key of u32 costs (any shape) as int64: monotone, larger = heavier."""
    c = np.asarray(cost).astype(np.uint64)
    e = np.zeros(c.shape, np.int64)
    for b in range(5, 32):                                       # floor(log2 c) for c >= 32, by comparison (no floats)
        e[c >= np.uint64(1 << b)] = b
    shift = np.maximum(e - 5, 0).astype(np.uint64)
    m = ((c >> shift) & np.uint64(31)).astype(np.int64)
    return np.where(c < 32, c.astype(np.int64), (e - 4) * 32 + m)


def cost_of_key(key):
    """The smallest cost with this key (0 .. N_KEYS - 1), a Python int."""
    key = int(key)
    assert 0 <= key < N_KEYS
    return key if key < 32 else (32 + key % 32) << (key // 32 + 4 - 5)


def bucket_edges(e, m):
    """(smallest, largest) cost of the bucket with exponent e (5 .. 31) and mantissa m (0 .. 31)."""
    lo = (32 + m) << (e - 5)
    return lo, lo + (1 << (e - 5)) - 1


def order_violations(cost, order, members=None):
    """The names of the checks (see the module's head) that `order` fails for these costs: a subset of
    ["permutation", "key", "bound"], empty for a sound order.  cost: u32 per tile id; members: the tile ids queued (None: all)."""
    cost = np.asarray(cost).astype(np.uint64).ravel()
    order = np.asarray(order).astype(np.int64).ravel()
    members = np.arange(len(cost), dtype=np.int64) if members is None else np.asarray(members).astype(np.int64).ravel()
    bad = []
    in_range = (order >= 0) & (order < len(cost))
    if len(order) != len(members) or not in_range.all() or not np.array_equal(np.sort(order), np.sort(members)):
        bad.append("permutation")
    c = cost[order[in_range]]                                   # (entries that name no tile have no cost to judge)
    if len(c) > 1:
        if (np.diff(key_of(c)) > 0).any():
            bad.append("key")
        allowed = np.where(c < 32, c, c + (c >> np.uint64(5)))  # what may follow an entry of this cost
        if (c[1:] > np.minimum.accumulate(allowed)[:-1]).any():
            bad.append("bound")
    return bad


def check_order(cost, order, members=None):
    bad = order_violations(cost, order, members)
    assert not bad, f"the queue order fails: {', '.join(bad)} ({len(np.ravel(order))} entries)"


def tile_max(pixel_costs, width, rows):
    """Per-tile maximum over 8 x 8 tiles of a (rows, width) cost image, flat, tile = tile row * tiles_x + tile column; a ragged
    right column and a ragged top row hold the pixels there are."""
    p = np.asarray(pixel_costs).reshape(rows, width)
    ty, tx = (rows + TILE - 1) // TILE, (width + TILE - 1) // TILE
    padded = np.zeros((ty * TILE, tx * TILE), p.dtype)
    padded[:rows, :width] = p
    return padded.reshape(ty, TILE, tx, TILE).max(axis=(1, 3)).ravel()


# ---- cost inputs

def edge_values():
    """Both edges of the buckets of every exponent 5 .. 31 and mantissa 0, 1, 30, 31, and the fixed values."""
    v = list(FIXED_VALUES)
    for e in range(5, 32):
        for m in (0, 1, 30, 31):
            v.extend(bucket_edges(e, m))
    return np.array(sorted(set(v)), np.uint64).astype(np.uint32)


def _fill(pool, n, rng):
    """n values of the pool in random order: each once while they last, then again."""
    reps = -(-n // len(pool))
    return np.concatenate([rng.permutation(pool) for _ in range(reps)])[:n].astype(np.uint32)


def cost_families(n, seed=0):
    """{name: n u32 costs}, the input families of the module's head."""
    rng = np.random.default_rng([seed, n])
    log_uniform = np.minimum(np.floor(2.0 ** rng.uniform(0.0, 32.0, n)), float(U32_MAX)).astype(np.uint64).astype(np.uint32)
    i = np.arange(n)
    # 64 consecutive entries (a wave of the 256-thread launches) in 64 different buckets, other buckets in the next wave
    distinct = np.array([cost_of_key((13 * (k % 64) + 7 * (k // 64)) % N_KEYS) for k in range(n)], np.uint64).astype(np.uint32)
    return {
        "edges": _fill(edge_values(), n, rng),
        "log-uniform": log_uniform,
        "below-40": rng.integers(0, 40, n).astype(np.uint32),
        "all-equal": np.full(n, 1000, np.uint32),
        "distinct-per-wave": distinct,
        "ascending": np.sort(log_uniform),
        "descending": np.sort(log_uniform)[::-1].copy(),
        "alternating": np.where(i % 2 == 0, 16, 4000).astype(np.uint32),
    }
