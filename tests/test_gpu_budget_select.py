"""The budget allocation on the device on the caller's arrays (mrt_debug_budget_plan: budget.hip's kernels, launched as
mrt_noise_query_budget launches them, without an image in front): every case of tests/budget_select_cases.py against the host's
mrt_budget_allocate -- k bit for bit, tile_frames, tiles and frames equal, var_before and var_after equal to the blocked reference
(tests/budget_plan_ref.blocked_sums) as 64-bit patterns.  No tolerance anywhere.

What the cases exercise of the radix select is asserted without a GPU (tests/test_budget_plan_host.py,
test_the_direct_cases_end_the_selection_at_every_digit): the selection ends at every digit of 0 .. 8 and 10 .. 12.  Digit 9 -- the
top byte of t -- would need 2^24 tiles and is not tested.

The groups: sizes from 1 tile to 2^19 + 257 (a partial second trip of the grid stride, 8,197 blocks of sums: 129 rounds of the last
kernel), ranks across distinct gains; pairs of keys that first differ at each digit; values no tile sum produces; frame counts at
which n + j + 1 crosses the K table's end."""
import numpy as np
import pytest

import budget_plan_ref as ref
import budget_select_cases as bc

pytestmark = pytest.mark.gpu

MRT_ERR_INVALID_ARG = 1


def _f64(x):
    return np.float64(x).view(np.uint64)


def _state(mrt, max_w):
    return mrt.State(mrt.Args(8, 8, 1, 2, max_w), seed=1)          # no scene, no tracking, no frames


def _check(mrt, st, case, budgets=None):
    s, n, nf = case["s"], case["n"], bc.n_full(case)
    for budget in case["budgets"] if budgets is None else budgets:
        what = (case["name"], budget)
        k, got = st.debug_budget_plan(s, n, budget, case["max_frames"])
        k_host, want = mrt.State.budget_allocate(s, nf, case["max_w"], budget, case["max_frames"])
        bad = np.nonzero(k != k_host)[0]
        assert bad.size == 0, (what, bad[:8], k[bad[:8]], k_host[bad[:8]])
        assert got["used_seq"] == 0, what
        for f in ("tile_frames", "tiles", "frames"):
            assert got[f] == want[f], (what, f, got[f], want[f])
        before, after = ref.blocked_sums(s, n, k_host, case["max_w"])
        assert _f64(got["var_before"]) == _f64(before), (what, got["var_before"], before)
        assert _f64(got["var_after"]) == _f64(after), (what, got["var_after"], after)


@pytest.mark.parametrize("group", bc.GROUPS)
def test_the_device_allocates_as_the_host(mrt, group):
    """every case of the group in a context of its own (so a K-table case's first call is the one that grows the table)"""
    for case in bc.group(group):
        with _state(mrt, case["max_w"]) as st:
            _check(mrt, st, case)
            assert st.debug_check_context() is None


@pytest.mark.parametrize("max_w", [1.0, 0.9])
def test_the_k_table_grows_under_one_context(mrt, max_w):
    """n_t 4,060 .. 4,100, then 8,180 .. 8,200, then 70,000 in one context: the table of 4,096 entries doubles once, once more, then
    several times within one call, and a smaller map after that reads the grown table.  At weight 0.9 K is constant from n = 178 on:
    those tiles have no gains, and var_after is still exact."""
    cases = bc.ktable_cases(max_w)
    with _state(mrt, max_w) as st:
        for case in cases + cases[:1]:
            _check(mrt, st, case, case["budgets"][::3] + case["budgets"][-1:])
        assert st.debug_check_context() is None
    if max_w == 0.9:
        o = bc.ordered_of(cases[0])
        assert o["all"] == 0                                 # no candidate at all: every budget is "nothing to take"


def test_an_n_above_2_to_the_24_is_refused_and_the_context_goes_on(mrt):
    case = bc.group("size-65")[0]
    n = case["n"].copy()
    n[17] = (1 << 24) + 1
    with _state(mrt, 1.0) as st:
        _check(mrt, st, case, case["budgets"][:4])
        for bad_n in (n, (1 << 24) + 1):
            with pytest.raises(mrt.MrtError) as e:
                st.debug_budget_plan(case["s"], bad_n, 10, 4)
            assert e.value.status == MRT_ERR_INVALID_ARG, e.value
        for bad_frames in (0, 33):
            with pytest.raises(mrt.MrtError) as e:
                st.debug_budget_plan(case["s"], case["n"], 10, bad_frames)
            assert e.value.status == MRT_ERR_INVALID_ARG, e.value
        assert st.debug_check_context() is None
        _check(mrt, st, case)
        n[17] = 1 << 12                                      # and the table still grows afterwards
        grown = dict(case, n=n)
        _check(mrt, st, grown, case["budgets"][-6:])
        assert st.debug_check_context() is None
