"""What the noise report's tests share: crafted S / framebuffer pairs with the special values the reduction must classify, the
rules a report is checked by, the rule that ties a summed-S query's report to a max-rel query's, and the four forms of the one
reduction kernel (noise.hip: uniform or per-tile K, max-rel or summed-S map) with their expected values from the existing
references (tests/noise_ref.py, tests/adaptive_ref.py, tests/budget_ref.py)."""
import ctypes as C
import math

import numpy as np

import adaptive_ref
import budget_ref
import noise_ref


def crafted(shapes, seed=3):
    """One (S, rgba) pair per (rows, width) of `shapes`, from ONE generator in that order: random S and colours with, at random
    places, NaN and +-inf in S and in a colour, L = 0, S = 0 and an S whose product with K overflows (as many as fit)."""
    rng = np.random.default_rng(seed)
    cases = []
    for rows, width in shapes:
        S = (rng.random((rows, width), np.float32) ** 3 * 0.02).astype(np.float32)
        rgba = rng.random((rows, width, 4), np.float32) * 1.5
        flat_s, flat_c = S.reshape(-1), rgba.reshape(-1, 4)
        n = flat_s.size
        pick = rng.permutation(n)
        specials = [(0, "s", np.nan), (1, "s", np.inf), (2, "s", -np.inf), (3, "c", np.nan), (4, "c", np.inf),
                    (5, "c", -np.inf), (6, "zero", 0.0), (7, "s0", 0.0), (8, "big", 3.0e38)]
        for j, kind, v in specials:
            if j >= n:
                break
            i = pick[j]
            if kind == "s":
                flat_s[i] = v
            elif kind == "c":
                flat_c[i, j % 3] = v
            elif kind == "zero":
                flat_c[i, :3] = 0.0                                     # L = 0 < floor
            elif kind == "s0":
                flat_s[i] = 0.0
            else:
                flat_s[i] = v                                           # S * K overflows to inf
        cases.append((S, rgba))
    return cases


def check_report(rep, want, exact_seq=None):
    for k in ("pixels", "above", "non_finite"):
        assert rep[k] == want[k], (k, rep[k], want[k])
    for k in ("max_se", "rmse", "rel_rmse", "sum_var"):
        if math.isinf(want[k]):
            assert math.isinf(rep[k]), k
    assert rep["max_se"] == want["max_se"], (rep["max_se"], want["max_se"])
    for k in ("sum_var", "sum_lum"):
        if not math.isinf(want[k]):
            assert abs(rep[k] - want[k]) <= 1e-12 * max(abs(want[k]), 1e-300), (k, rep[k], want[k])


def raw_report(mrt, st):
    """the newest report as the C struct, after its bounded wait"""
    r = mrt._lib.MrtNoiseReport()
    st._check(st._L.mrt_noise_result(st._ctx, 1, C.byref(r)), "mrt_noise_result")
    return r


def check_same_but_kind(mrt, a, b):
    """a: the report of a max-rel query, b: of the summed-S query queued right behind it on the same state: equal in every
    field but seq and reserved (the map's kind), floats bit for bit"""
    assert b.seq == a.seq + 1 and a.reserved == 0 and b.reserved == 1 and a.reserved2 == b.reserved2 == 0
    for name, ctype in mrt._lib.MrtNoiseReport._fields_:
        if name in ("seq", "reserved"):
            continue
        x, y = getattr(a, name), getattr(b, name)
        if ctype in (C.c_double, C.c_float):
            x, y = np.float64(x).view(np.uint64), np.float64(y).view(np.uint64)
        assert x == y, (name, getattr(a, name), getattr(b, name))


# ---- the four forms of the reduction on the same crafted data (tests/test_gpu_noise_forms.py, tests/test_noise_host.py) --------
# (W, H): a partial tile column and a partial band, whose rows at or beyond H are skipped (5 x 3, 37 x 9); exactly one block of
# 256 columns (256 x 8); a second block of one column (257 x 17); a third block of eight (520 x 20)
FORM_SIZES = ((5, 3), (37, 9), (256, 8), (257, 17), (520, 20))
# form -> (frames rendered before the load, the tile_frames cycle loaded or None: a uniform accumulation)
FORMS = {"uniform": (3, None), "no-estimate": (0, None), "per-tile-inf": (0, (0, 1, 2, 3, 5, 9)), "per-tile": (0, (2, 3, 5, 9, 17))}
FORM_MAX_W = 1.0
_cases = {}


def form_case(size):
    """(S, rgba) of FORM_SIZES' entry `size`, made once"""
    if not _cases:
        _cases.update(zip(FORM_SIZES, crafted([(h, w) for w, h in FORM_SIZES])))
    return _cases[size]


def form_tile_frames(size, form):
    """the n_t a form loads: its cycle over the tiles in id order, or None"""
    cycle = FORMS[form][1]
    w, h = size
    return None if cycle is None else np.resize(np.array(cycle, np.uint32), (-(-w // 8)) * (-(-h // 8)))


def form_expected(size, form, threshold, floor):
    """{report, max_rel, sum_s}: what the two queries of `form` give for form_case(size), from the references"""
    S, rgba = form_case(size)
    w, h = size
    n = form_tile_frames(size, form)
    if n is None:
        K = adaptive_ref.k_table(FORMS[form][0], FORM_MAX_W)[-1]
        report = noise_ref.report(S, rgba, K, threshold, floor)
        max_rel = noise_ref.tiles(S, rgba, K, threshold, floor)
    else:
        acc = adaptive_ref.Accum(h, w, FORM_MAX_W)
        acc.load(rgba, S, n)
        report, max_rel = acc.report(threshold, floor), acc.tiles(threshold, floor)
    return {"report": report, "max_rel": max_rel, "sum_s": budget_ref.tile_sums(S, rgba)}
