"""The direct cases of the device's budget allocation (mrt_debug_budget_plan: budget.hip on the caller's arrays): maps of s and n
with the budgets worth asking, built on the CPU from seeds.  tests/test_gpu_budget_select.py runs them against
mrt_budget_allocate; tests/test_budget_plan_host.py asserts, by budget_plan_ref.replay alone, what they exercise of the radix
select: the digit at which the selection ends, the mode, the bins it descends into.

A case is a dict {name, s (float32, one per tile), n (uint32 per tile, or an int: uniform), max_w, max_frames, budgets, ends}.
`ends`, where a case was built for it, is the digit at which budgets[0] must end the selection (replay confirms it).

The digits of a key: 0 .. 7 = G's bytes from the top, 8 = j, 9 .. 12 = t's bytes from the top.  Digit 9 would need two tiles whose
ids differ in bit 24 or above, 2^24 tiles: it is left out."""
import functools
import math

import numpy as np

import budget_plan_ref as ref
import budget_ref

# 63 .. 65 and 255 .. 257: around a wave's block of sums and a workgroup; 4,095 / 4,097: a partial last block of 64; 65,535 / 65,537:
# digit 10 switches on; 2^19 and 2^19 + 257: a full and a partial second trip of the grid stride (8,197 blocks of sums)
TILES = (1, 63, 64, 65, 255, 256, 257, 4095, 4097, 65535, 65537, 1 << 19, (1 << 19) + 257)
FLT_MIN, FLT_MAX = np.float32(1.17549435e-38), np.float32(3.4028235e38)


def log_uniform(rng, tiles):
    return np.exp(rng.uniform(math.log(1e-8), math.log(1e4), tiles)).astype(np.float32)       # 12 decades


def ordered_of(case):
    return ref.order(case["s"], case["n"], case["max_w"], case["max_frames"])


def rank_budgets(all_, rng, draws=16):
    """ranks worth selecting where the gains are distinct: the first, around a histogram's 256, the middle, the last but one, and
    `draws` ranks across [1, all]"""
    b = {1, 2, 255, 256, 257, all_ // 2, all_ - 1}
    if all_ >= 1:
        b |= {int(x) for x in rng.integers(1, all_ + 1, draws)}
    return sorted(x for x in b if 1 <= x <= all_)


def _case(name, s, n, max_w, max_frames, budgets=None, seed=0, draws=16, ends=None):
    c = {"name": name, "s": np.ascontiguousarray(s, np.float32), "n": n if np.ndim(n) == 0 else np.ascontiguousarray(n, np.uint32),
         "max_w": max_w, "max_frames": max_frames, "ends": ends}
    if budgets is None:
        o = ordered_of(c)
        budgets = sorted(set(ref.budgets(o)) | set(rank_budgets(o["all"], np.random.default_rng(seed), draws)))
    c["budgets"] = [int(b) for b in budgets]
    return c


def n_full(case):
    """n per tile, as mrt_budget_allocate takes it"""
    return np.full(case["s"].size, case["n"], np.uint32) if np.ndim(case["n"]) == 0 else case["n"]


# ---- sizes: log-uniform s, n random in 0 .. 40 (with tiles at 0 and 1) and n uniform
@functools.lru_cache(maxsize=None)
def size_cases(tiles):
    i = TILES.index(tiles)
    out = []
    rng = np.random.default_rng(100 + i)
    big = tiles >= 65535
    n = rng.integers(0, 41, tiles).astype(np.uint32)
    if tiles >= 2:
        n[0], n[-1] = 0, 1
    out.append(_case(f"size-{tiles}", log_uniform(rng, tiles), n, 1.0, 4 if big else 32, seed=i))
    if tiles in (1, 65, 257, 4097, 65537, (1 << 19) + 257):
        out.append(_case(f"size-{tiles}-uniform", log_uniform(rng, tiles), (5, 2, 17)[i % 3], (1.0, 0.9)[i % 2], 3 if big else 32,
                         seed=50 + i))
    return out


# ---- the deciding digit: pairs of gains whose keys first differ at byte d of G
def first_difference(G, lo):
    """for keys in ascending order: the first digit at which key i + 1 differs from key i"""
    def top_byte(x, width):                                  # the index from the top of the first nonzero byte of a width-byte value
        b = x.astype(">u8").view(np.uint8).reshape(-1, 8)[:, 8 - width:]
        return np.argmax(b != 0, axis=1)
    g, l = G[1:] ^ G[:-1], lo[1:] ^ lo[:-1]
    return np.where(g != 0, top_byte(g, 8), 8 + top_byte(l, 5))


@functools.lru_cache(maxsize=None)
def gain_pairs(seed=2024, count=1 << 22):
    """{d: [(s_a, n_a, s_b, n_b)]}: tiles whose single gains' keys first differ at byte d of G, d = 1 .. 7, found among `count`
    gains of random s in [1, 2) and n in 2 .. 130 (max_frames 1, weight 1: one candidate a tile), sorted; for every d pairs whose
    smaller key has each residue mod 4 at byte d, and pairs with a byte 0x00 .. 0x03 or 0xFC .. 0xFF among bytes 1 .. d"""
    rng = np.random.default_rng(seed)
    s = (np.float32(1) + rng.integers(0, 1 << 23, count).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
    n = rng.integers(2, 131, count)
    K = budget_ref.k_values(132, 1.0)
    G = ~np.ascontiguousarray(s.astype(np.float64) * (K[n] - K[n + 1])).view(np.uint64)
    o = np.argsort(G, kind="stable")
    G, s, n = G[o], s[o], n[o]
    d = first_difference(G, np.zeros_like(G))                # (equal G: reads 8 + 0 = 8: not a pair of distinct gains)
    bytes_ = G[:-1].astype(">u8").view(np.uint8).reshape(-1, 8)
    pairs, found = {}, {}
    for dig in range(1, 8):
        at = np.nonzero(d == dig)[0]
        found[dig] = int(at.size)
        chosen, have = [], set()
        for i in at[:4000]:
            row = bytes_[i]
            new = {("res", int(row[dig]) % 4)} | {("lane0",) for b in row[1:dig + 1] if b < 4} | {("lane63",) for b in row[1:dig + 1] if b >= 252} \
                | {("bin", int(b)) for b in row[1:dig + 1] if b in (0, 255)}
            if new - have:
                have |= new
                chosen.append((np.float32(s[i]), int(n[i]), np.float32(s[i + 1]), int(n[i + 1])))
            if len(have) == 8:
                break
        pairs[dig] = chosen
    return pairs, found


def pair_map(rng, tiles, pair, scale=1.0):
    """a map of `tiles` tiles holding the pair's two tiles, the other gains two to six decades above or below; n in 2 .. 130"""
    sa, na, sb, nb = pair
    mag = 10.0 ** (rng.integers(2, 7, tiles) * rng.choice((-1, 1), tiles))
    s = (rng.uniform(1.0, 2.0, tiles) * mag).astype(np.float32)
    n = rng.integers(2, 131, tiles).astype(np.uint32)
    a, b = rng.choice(tiles, 2, replace=False)
    s[a], n[a], s[b], n[b] = sa, na, sb, nb
    return (s * np.float32(scale)).astype(np.float32), n, int(a), int(b)


def rank_of_pair(case, a, b):
    """the rank (1-based) of the smaller of the two keys (j = 0 of tiles a and b)"""
    G, lo = ref.sort_keys(ref.keys(case["s"], case["n"], case["max_w"], case["max_frames"]))
    at = np.nonzero((lo == a) | (lo == b))[0]
    assert at.size == 2 and at[1] == at[0] + 1, "the pair's keys are not next to each other"
    return int(at[0]) + 1


@functools.lru_cache(maxsize=None)
def digit_cases():
    out = []
    rng = np.random.default_rng(7)
    # byte 0: two exponent ranges -- s in [1, 2) gives gains below 1 (top byte 0x3F), s * 2^20 gains of 2 and more (0x40 and 0x41)
    for i, tiles in enumerate((40, 300)):
        s = rng.uniform(1.0, 2.0, tiles).astype(np.float32)
        n = rng.integers(2, 131, tiles).astype(np.uint32)
        high = rng.random(tiles) < 0.4
        high[:2] = True, False
        s[high] *= np.float32(2.0 ** (20 + 8 * i))
        c = _case(f"digit-0-{tiles}", s, n, 1.0, 1, budgets=[0])
        c["budgets"] = [int(high.sum()), int(high.sum()) + 1]
        c["ends"] = 0
        out.append(c)
    pairs, _ = gain_pairs()
    for d in range(1, 8):
        for i, pair in enumerate(pairs[d]):
            tiles = int(rng.integers(20, 301))
            # every power of two scales both gains alike: the mantissa bytes stay, the exponent bytes move
            s, n, a, b = pair_map(rng, tiles, pair, 2.0 ** int(rng.integers(-30, 31)) if d >= 2 else 1.0)
            c = _case(f"digit-{d}-{i}", s, n, 1.0, 1, budgets=[0])
            r = rank_of_pair(c, a, b)
            c["budgets"], c["ends"] = [r, r + 1], d
            out.append(c)
    # digit 8: equal G, different j -- the same s, n_B = n_A + 1: tile A's gain at j + 1 is tile B's at j
    for i, (tiles, max_frames) in enumerate(((30, 2), (300, 4), (120, 32))):
        mag = 10.0 ** (rng.integers(3, 7, tiles) * rng.choice((-1, 1), tiles))
        s = (rng.uniform(1.0, 2.0, tiles) * mag).astype(np.float32)
        n = rng.integers(60, 131, tiles).astype(np.uint32)      # (32 frames from n = 60 on span less than a decade)
        a, b = rng.choice(tiles, 2, replace=False)
        s[a] = s[b] = np.float32(1.37)
        n[a], n[b] = 70, 71
        c = _case(f"digit-8-{i}", s, n, 1.0, max_frames, budgets=[0])
        G, lo = ref.sort_keys(ref.keys(c["s"], c["n"], 1.0, max_frames))
        at = np.nonzero(first_difference(G, lo) == 8)[0]
        assert at.size == max_frames - 1
        c["budgets"] = sorted({int(x) + 1 for x in at} | {int(x) + 2 for x in at})
        c["ends"] = 8
        out.append(c)
    # digits 10 .. 12: equal G and equal j, t differing in bit 16 and above, in the second byte alone, in the low byte alone
    t_pairs = ((12, 63, 1, 2), (12, 257, 252, 255), (12, 257, 2, 3), (12, 4095, 0x703, 0x7C8), (12, 65537, 0xFFFC, 0xFFFF),
               (11, 4095, 5, 0x105), (11, 4097, 0x3FE, 0x9FE), (11, 65535, 0xFC07, 0xFF07), (11, 65537, 0x0101, 0xFF01),
               (10, 65537, 0, 0x10000), (10, (1 << 19) + 257, 0x100FD, 0x700FD), (10, 1 << 19, 0x2FFFF, 0x3FFFF),
               (10, (1 << 19) + 257, 0x7FFFE, 0x80100))
    for i, (d, tiles, a, b) in enumerate(t_pairs):
        s = np.zeros(tiles, np.float32)                     # most tiles have no candidate
        some = rng.choice(tiles, min(tiles, 40), replace=False)
        s[some] = (rng.uniform(1.0, 2.0, some.size) * 10.0 ** (rng.integers(2, 7, some.size) * rng.choice((-1, 1), some.size))).astype(np.float32)
        s[a] = s[b] = np.float32(1.62)
        c = _case(f"digit-{d}-t{i}", s, 9, 1.0, 1, budgets=[0])
        r = rank_of_pair(c, a, b)
        c["budgets"], c["ends"] = [r, r + 1], d
        out.append(c)
    return out


# ---- values a tile sum never produces, each mixed into a random map
@functools.lru_cache(maxsize=None)
def value_cases():
    out = []
    sub = np.float32(1e-41)
    kinds = {"subnormal": (sub, 5), "flt-min": (FLT_MIN, 5), "flt-max": (FLT_MAX, 2), "minus-zero": (np.float32(-0.0), 5),
             "inf": (np.float32(np.inf), 7), "inf-below-2": (np.float32(np.inf), 1), "nan": (np.float32(np.nan), 6)}
    for i, (name, (v, nv)) in enumerate(kinds.items()):
        rng = np.random.default_rng(300 + i)
        tiles = 65 + 64 * (i % 2)
        s = log_uniform(rng, tiles)
        n = rng.integers(0, 41, tiles).astype(np.uint32)
        at = rng.choice(tiles, 9, replace=False)
        s[at] = v
        n[at] = nv
        if name == "subnormal":
            s[at[:4]] = np.float32([1.4e-45, 2.8e-45, 5.9e-39, 1.1754942e-38])     # the smallest two, and the largest subnormal
        out.append(_case(f"value-{name}", s, n, 1.0, (32, 4)[i % 2], seed=300 + i))
    rng = np.random.default_rng(399)
    s = log_uniform(rng, 129)
    n = rng.integers(2, 41, 129).astype(np.uint32)
    for t, base in ((3, np.float32(0.75)), (70, np.float32(1e-30)), (128, FLT_MAX)):      # adjacent floats, at equal n
        s[t], s[t - 1] = base, np.nextafter(base, np.float32(0))
        n[t] = n[t - 1] = 11
    out.append(_case("value-adjacent", s, n, 1.0, 8, seed=399))
    return out


# ---- the K table: n_t + j + 1 crosses its end (4,096 entries at first, doubled as needed)
@functools.lru_cache(maxsize=None)
def ktable_cases(max_w):
    """in the order a context should meet them: the table doubles once, once more, then several times in one call"""
    out = []
    i = (1.0, 0.9).index(max_w)
    rng = np.random.default_rng(400 + i)
    for lo, hi in ((4060, 4100), (8180, 8200)):
        out.append(_case(f"ktable-{lo}-w{max_w}", log_uniform(rng, 257), rng.integers(lo, hi + 1, 257).astype(np.uint32), max_w, 32,
                         seed=400 + i))
    n = rng.integers(0, 200, 130).astype(np.uint32)
    n[[7, 129]] = 70000
    out.append(_case(f"ktable-70000-w{max_w}", log_uniform(rng, 130), n, max_w, 32, seed=410 + i))
    return out


DIGITS_COVERED = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12)
GROUPS = tuple(f"size-{t}" for t in TILES) + tuple(f"digit-{d}" for d in DIGITS_COVERED) + ("values", "ktable-w1.0", "ktable-w0.9")


def group(name):
    """the cases of one group of GROUPS (the groups are built one by one: the largest maps take seconds to order)"""
    kind, _, arg = name.partition("-")
    if kind == "size":
        return size_cases(int(arg))
    if kind == "digit":
        return [c for c in digit_cases() if c["name"].split("-")[1] == arg]
    if kind == "values":
        return value_cases()
    return ktable_cases(float(arg[1:]))


def cases():
    """every case, in a fixed order; the names are unique"""
    out = [c for g in GROUPS for c in group(g)]
    assert len({c["name"] for c in out}) == len(out)
    return out
