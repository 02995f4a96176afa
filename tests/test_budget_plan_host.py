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
NEW = ("mrt_noise_query_budget", "mrt_read_budget_plan", "mrt_render_planned")
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
    header = open(os.path.join(ROOT, "include", "myraytracer_amd.h")).read()
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
