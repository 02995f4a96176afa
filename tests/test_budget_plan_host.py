"""Budget allocation on the device, host side (no GPU): the key order of tests/budget_plan_ref.py -- what budget.hip selects --
gives mrt_budget_allocate's allocation (the C function) on every input family; the blocked variance sums agree with the host's
chained ones; the new entry points are declared, bound, exported by both libraries, and refuse a NULL context."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import budget_plan_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MRT_ERR_INVALID_ARG = 1
NEW = ("mrt_noise_query_budget", "mrt_read_budget_plan", "mrt_render_planned", "mrt_debug_budget_plan")
TILES = (1, 6, 65, 260, 8192)
S_KINDS = ("equal", "zero", "log-uniform", "negative", "nan", "inf")
N_KINDS = (0, 1, 2, 17, "random", "below-2")
MAX_FRAMES = (1, 2, 3, 32)
WEIGHTS = (1.0, 0.9, 0.5)


def s_of(kind, tiles, rng):
    if kind == "equal":
        return np.full(tiles, 0.75, np.float32)            # the order is decided by j, then t
    if kind == "zero":
        return np.zeros(tiles, np.float32)
    s = np.exp(rng.uniform(math.log(1e-8), math.log(1e4), tiles)).astype(np.float32)      # 12 decades
    some = rng.random(tiles) < 0.3
    some[0] = kind != "log-uniform"
    if kind == "negative":
        s[some] = -s[some]
    elif kind == "nan":
        s[some] = np.nan
    elif kind == "inf":
        s[some] = np.inf
    return s


def n_of(kind, tiles, rng):
    """(the n the reference takes -- a scalar for a uniform accumulation --, n per tile for the C function)"""
    if isinstance(kind, int):
        return kind, np.full(tiles, kind, np.uint32)
    n = rng.integers(0, 2 if kind == "below-2" else 41, tiles).astype(np.uint32)
    if kind == "random" and tiles >= 2:
        n[0], n[-1] = 0, 1
    return n, n


def close(a, b):
    return a == b or (math.isfinite(a) and math.isfinite(b) and abs(a - b) <= 1e-12 * max(abs(a), abs(b)))


def check_family(mrt, tiles, s_kind, n_kind, max_frames, max_w, seed):
    rng = np.random.default_rng(seed)
    s = s_of(s_kind, tiles, rng)
    n_ref, n = n_of(n_kind, tiles, rng)
    o = ref.order(s, n_ref, max_w, max_frames)
    for budget in ref.budgets(o):
        k, res = mrt.State.budget_allocate(s, n, max_w, budget, max_frames)
        k_ref, want = ref.plan(s, n_ref, max_w, budget, max_frames, o)
        what = (tiles, s_kind, n_kind, max_frames, max_w, budget)
        assert np.array_equal(k, k_ref), what
        for f in ("tile_frames", "tiles", "frames"):
            assert res[f] == want[f], (what, f)
        for f in ("var_before", "var_after"):
            assert close(res[f], want[f]), (what, f, res[f], want[f])
    return o


@pytest.mark.parametrize("tiles", TILES[:4])
@pytest.mark.parametrize("max_w", WEIGHTS)
def test_the_key_order_is_the_hosts_allocation(mrt, tiles, max_w):
    cut = 0
    for a, s_kind in enumerate(S_KINDS):
        for b, n_kind in enumerate(N_KINDS):
            for max_frames in MAX_FRAMES:
                o = check_family(mrt, tiles, s_kind, n_kind, max_frames, max_w, 1000 * tiles + 10 * a + b)
                cut += o["tie"] is not None
    assert cut or tiles == 1                                # some budget did cut through a group of equal gains


def test_the_key_order_is_the_hosts_allocation_at_8192_tiles(mrt):
    """every s family and every n family, with max_frames and the weight taken in turn"""
    i = 0
    for a, s_kind in enumerate(S_KINDS):
        for b, n_kind in enumerate(N_KINDS):
            check_family(mrt, TILES[4], s_kind, n_kind, MAX_FRAMES[i % 4], WEIGHTS[i % 3], 77 + i)
            i += 1


def test_a_saturated_weight_ends_the_gains(mrt):
    """max_framebuffer_weight 0.9: K reaches its fixed point, the gains become 0 and a tile far along has no candidate"""
    s = np.ones(4, np.float32)
    o_early, o_late = ref.order(s, 3, 0.9, 4), ref.order(s, 4000, 0.9, 4)
    assert o_early["all"] == 16 and o_late["all"] == 0
    k, res = mrt.State.budget_allocate(s, np.full(4, 4000, np.uint32), 0.9, 10, 4)
    assert not k.any() and res["tile_frames"] == 0


def test_the_target_rule():
    k = np.array([3, 0, 2, 1], np.uint32)
    assert ref.target(5, k, 5).tolist() == [3, 0, 2, 1]                            # nothing queued in between
    assert ref.target(5, k, np.array([6, 6, 8, 5])).tolist() == [2, 0, 0, 1]
    assert ref.target(np.array([1, 2, 3, 4]), k, np.array([4, 2, 4, 9])).tolist() == [0, 0, 1, 0]


def test_the_blocked_sums_are_blocked():
    """65 tiles: the last tile is a block of its own, and the order of the additions shows in the last bits"""
    rng = np.random.default_rng(3)
    s = np.exp(rng.uniform(-20, 20, 65)).astype(np.float32)
    before, _ = ref.blocked_sums(s, 5, np.zeros(65, np.uint32), 1.0)
    K5 = ref.budget_ref.k_values(5, 1.0)[5]
    a = ref.clean(s) * K5
    head = 0.0
    for v in a[:64]:
        head += float(v)
    assert before == (0.0 + head) + (0.0 + float(a[64]))


def test_the_new_entry_points_are_declared_bound_and_exported(mrt):
    from myraytracer_amd import _lib
    header = open(os.path.join(ROOT, "include", "myraytracer_amd.h")).read() + open(os.path.join(ROOT, "include", "myraytracer_amd_debug.h")).read()
    for lib in ("libmyraytracer_amd.so", "libmyraytracer_amd_failinject.so"):
        names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "myraytracer_amd", "lib", lib)],
                               capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert f" {name}\n" in names, (lib, name)
    for name in NEW:
        assert f"int {name}(mrt_ctx* ctx" in header and name in _lib.EXPORTS
    assert "MRT_ABI_VERSION 4" in header and _lib.load().mrt_abi_version() == 4


def test_a_null_context_is_refused(mrt):
    from myraytracer_amd import _lib
    L = _lib.load()
    r = _lib.MrtBudgetResult()
    k = np.zeros(4, np.uint32)
    assert L.mrt_noise_query_budget(None, 0.02, 0.01, 10, 4) == MRT_ERR_INVALID_ARG
    assert L.mrt_read_budget_plan(None, 0, k.ctypes.data, k.size, C.byref(r)) == MRT_ERR_INVALID_ARG
    assert L.mrt_render_planned(None, 0, C.byref(r), k.ctypes.data, k.size) == MRT_ERR_INVALID_ARG
    s = np.ones(4, np.float32)
    assert L.mrt_debug_budget_plan(None, s.ctypes.data, None, 3, 4, 10, 4, k.ctypes.data, C.byref(r)) == MRT_ERR_INVALID_ARG


def test_replay_says_where_a_selection_ends():
    """hand-made keys: G in the top byte, the second byte and the last; then j; then each byte of t"""
    def keys(rows):
        G, j, t = (np.array(c, np.uint64) for c in zip(*rows))
        return np.ones(len(rows), np.int64), G, j.astype(np.int64), t.astype(np.int64)
    top = 0x80 << 56
    rows = [(top, 0, 5), (top, 0, 0x0105), (top, 0, 0x010005), (top, 0, 0x01010005), (top, 1, 0), (top | 1, 0, 0), (top | (1 << 48), 0, 0),
            (0x81 << 56, 0, 0)]
    got = [ref.replay(keys(rows[::-1]), b) for b in range(10)]
    assert got[0]["mode"] == "none" and got[8]["mode"] == got[9]["mode"] == "all" and ref.replay((np.zeros(0, np.uint64),) * 2, 3)["mode"] == "none"
    assert [g["q"] for g in got[1:8]] == [11, 10, 9, 8, 7, 1, 0]
    assert got[1]["T"] == (top, 5) and got[1]["bins"] == [0x80] + [0] * 11 and got[7]["bins"] == [0x80]
    assert got[5]["T"] == (top, 1 << 32) and got[5]["bins"] == [0x80, 0, 0, 0, 0, 0, 0, 0]
    two = ref.replay(keys([(top, 0, 0xFE), (top, 0, 0xFF), (top | 2, 3, 9)]), 1)
    assert two["q"] == 12 and two["bins"][-1] == 0xFE


def test_the_direct_cases_end_the_selection_at_every_digit():
    """What tests/test_gpu_budget_select.py's cases exercise of the radix select, by replay alone: over their union the selection
    ends at every digit of 0 .. 8 and 10 .. 12 (digit 9, t's top byte, would need 2^24 tiles: not covered), in all three modes;
    the bin it descends into is 0 and is 255 somewhere, falls on every residue mod 4 (the four counts of a lane) and in the first
    and the last lane's four; and every case built for a digit ends there."""
    import budget_select_cases as bc
    ends, modes, bins = set(), set(), set()
    per_digit = {}
    for case in bc.cases():
        sk = ref.sort_keys(ref.keys(case["s"], case["n"], case["max_w"], case["max_frames"]))
        for i, budget in enumerate(case["budgets"]):
            r = ref.replay(sk, budget)
            modes.add(r["mode"])
            if r["mode"] != "bin":
                continue
            if i == 0 and case["ends"] is not None:
                assert r["q"] == case["ends"], (case["name"], r)
            ends.add(r["q"])
            bins |= set(r["bins"])
            per_digit.setdefault(r["q"], set()).add(r["bins"][-1] % 4)
    assert ends == set(bc.DIGITS_COVERED) == {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12}, sorted(ends)
    assert modes == {"bin", "all", "none"}
    assert {0, 255} <= bins and {b % 4 for b in bins} == {0, 1, 2, 3}
    assert bins & {0, 1, 2, 3} and bins & {252, 253, 254, 255}          # the owner is lane 0, and lane 63
    for q in range(1, 8):                                               # at G's mantissa digits the deciding bin itself is in every slot
        assert per_digit[q] == {0, 1, 2, 3}, (q, per_digit[q])
    tiles = {case["s"].size for case in bc.cases()}
    assert set(bc.TILES) <= tiles and max(tiles) == (1 << 19) + 257
