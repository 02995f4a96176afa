"""The temporal response on the host (include/myraytracer_amd.h, "temporal reprojection", steps 4b and 4c): the float32 restatement
(tests/temporal_response_ref.py, which the GPU tests compare the device against bit for bit) against a plain float64 form of the
same definition and on the cases the definition singles out; three references broken on purpose, which the synthetic history the
GPU test loads too must tell from the intact one; the parameter checks that need no context.  Scenes and frames are
tests/test_temporal_host.py's, made on the host."""
import ctypes as C

import numpy as np
import pytest

from myraytracer_amd import _lib, api
from temporal_ref import camera_matrix, index_bits
from temporal_ref import step as plain_step
from temporal_response_ref import BROKEN, R_DEFAULTS, WINDOW, clamp, step, step_f64, synthetic_history
from test_temporal_host import CAM2, H, LOOKAT, SPHERES, W, frame, moved, view

F = np.float32
MRT_OK, MRT_ERR_INVALID_ARG = 0, 1


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def empty():
    return tuple(np.zeros((H, W, 4), F) for _ in range(3))


def advance(prev, now, cur, hist, params=None, rparams=None, broken=None):
    M, o = camera_matrix((prev or now)["raw"])
    return step(cur, now["rays"], now["index"], now["t"], now["xyzr"], (prev or now)["xyzr"], M, o, *hist, params, rparams, broken)


def moving_pair(seed, rparams):
    """(the state before, the state after, a history of four frames at the state before, the generator): the spheres and the
    camera of test_temporal_host.moving_pair"""
    rng = np.random.default_rng(seed)
    a = view(LOOKAT, SPHERES)
    b = view(CAM2, moved(SPHERES, rng))
    hist = empty()
    for _ in range(4):
        hist = advance(a, a, frame(rng, nonfinite=True), hist, None, rparams)[:3]
    return a, b, hist, rng


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("rparams", [{}, {"fast_history": 1, "clamp_sigma": 0.5, "antilag": 0.5}, {"fast_history": 16, "clamp_sigma": 1.0}])
def test_float32_form_matches_float64(seed, rparams):
    a, b, hist, rng = moving_pair(seed, rparams)
    cur = frame(rng, nonfinite=True)
    M, o = camera_matrix(a["raw"])
    args = (cur, b["rays"], b["index"], b["t"], b["xyzr"], a["xyzr"], M, o, *hist, None, rparams)
    g0, g1, g2, info = step(*args)
    r0, r1, r2, taps, window, side = step_f64(*args)
    assert all(g.dtype == F for g in (g0, g1, g2))
    # compared where both forms take the same taps, count the same window and clamp to the same side of the box (a colour within
    # rounding of a box edge may fall either way): that share is capped as tests/test_temporal_host.py caps the taps', at 1 %
    same = (info["taps"] == taps).all(-1) & (info["window"] == window).all(-1) & (info["side"] == side).all(-1)
    fin = np.isfinite(cur[..., :3]).all(-1) & same
    worst = 0.0
    for g, r in ((g0[..., :3], r0[..., :3]), (g0[..., 3], r0[..., 3]), (g1[..., :2], r1[..., :2]), (g2[..., :3], r2[..., :3])):
        g, r = g[fin].astype(np.float64), r[fin]
        worst = max(worst, float((np.abs(g - r) / (2e-6 + 2e-4 * np.abs(r))).max()))
    differ = 1.0 - same.mean()
    print(f"seed {seed} {rparams}: {differ:.4f} differ, worst {worst:.3f}, moved {info['moved'].mean():.3f}, kept {info['kept'].mean():.3f}")
    assert differ <= 0.01 and worst <= 1.0, (differ, worst)
    assert np.array_equal(g2[..., 3], np.isfinite(cur[..., :3]).all(-1).astype(F))
    # no trivial case: the clamp moved some pixels and left others with their history alone
    assert info["moved"].any() and info["kept"].mean() >= 0.05, (info["moved"].mean(), info["kept"].mean())


@pytest.mark.parametrize("fast_history", [1, 4, 16])
def test_a_clamp_that_never_acts_leaves_todays_step(fast_history):
    """clamp_sigma 1e6 and antilag 0: H0' and H1' are tests/temporal_ref.py's bit for bit over a moving sequence"""
    rng = np.random.default_rng(4)
    rp = {"fast_history": fast_history, "clamp_sigma": 1e6, "antilag": 0.0}
    a = view(LOOKAT, SPHERES)
    states = [a, a, view(CAM2, moved(SPHERES, rng)), view(CAM2, moved(SPHERES, rng, 0.08))]
    hist, plain = empty(), empty()[:2]
    prev = None
    for now in states:
        cur = frame(rng, nonfinite=True)
        M, o = camera_matrix((prev or now)["raw"])
        geo = (cur, now["rays"], now["index"], now["t"], now["xyzr"], (prev or now)["xyzr"], M, o)
        h0, h1, h2, info = step(*geo, *hist, None, rp)
        p0, p1, pinfo = plain_step(*geo, *plain)
        assert np.array_equal(_bits(h0), _bits(p0)) and np.array_equal(_bits(h1), _bits(p1))
        assert np.array_equal(info["taps"], pinfo["taps"]) and not info["moved"].any()
        hist, plain, prev = (h0, h1, h2), (p0, p1), now
    assert info["found"].mean() >= 0.5


def test_a_constant_frame_over_a_constant_history_is_not_clamped():
    a = view(LOOKAT, SPHERES)
    cur = np.full((H, W, 4), F(0.5), F)         # (0.5: every weighted sum is the weight sum halved, exactly)
    hist = empty()
    for k in range(1, 7):
        h0, h1, h2, info = advance(a, a, cur, hist, None, {"fast_history": 2, "clamp_sigma": 0.5})
        assert not info["moved"].any() and (h0[..., 3] == k).all() and np.array_equal(_bits(h0[..., :3]), _bits(cur[..., :3]))
        assert np.array_equal(_bits(h0), _bits(info["unclamped"])) and (info["applied"] == (k >= 2)).all()
        hist = (h0, h1, h2)


@pytest.mark.parametrize("fast_history,antilag", [(4, 1.0), (2, 1.0), (4, 0.25)])
def test_a_history_far_from_a_noisy_frame_lands_in_its_box(fast_history, antilag):
    rng = np.random.default_rng(6)
    a = view(LOOKAT, SPHERES)
    rp = {"fast_history": fast_history, "clamp_sigma": 2.0, "antilag": antilag}
    h0 = np.full((H, W, 4), F(5), F)
    h0[..., 3] = 8
    h1 = np.zeros((H, W, 4), F)
    h1[..., 2], h1[..., 3] = a["t"], index_bits(a["index"])
    h2 = frame(rng)
    cur = frame(rng)
    out, o1, o2, info = advance(a, a, cur, (h0, h1, h2), None, rp)
    found = info["found"]
    assert found.all() and info["applied"].all() and info["moved"].all() and (info["unclamped"][..., 3] == 9).all()
    # inside the box: clamping the result again moves nothing
    again, ainfo = clamp(out, o1, o2, rp)
    assert not ainfo["moved"].any() and np.array_equal(_bits(again[..., :3]), _bits(out[..., :3]))
    assert (out[..., :3] < 2).all() and (info["unclamped"][..., :3] > 4).all()
    full = info["r"] == 1
    assert full.mean() >= 0.9
    if antilag == 1.0:      # pulled all the way to the fast length
        assert (out[..., 3][full] == min(9, fast_history)).all()
    else:
        assert np.array_equal(_bits(out[..., 3][full]), _bits(np.full(int(full.sum()), F(9) + F(antilag) * (F(fast_history) - F(9)), F)))


def _field(rng):
    """a history after step 4 in which every window tap counts: one sphere index, valid fast colours"""
    h0 = rng.random((H, W, 4), dtype=F)
    h0[..., 3] = 3
    h1 = rng.random((H, W, 4), dtype=F)
    h1[..., 3] = index_bits(np.full((H, W), 2, np.int32))
    h2 = rng.random((H, W, 4), dtype=F)
    h2[..., 3] = 1
    return h0, h1, h2


@pytest.mark.parametrize("what", ["index", "valid", "colour"])
def test_a_window_tap_that_does_not_qualify_is_ignored(what):
    rng = np.random.default_rng(8)
    h0, h1, h2 = _field(rng)
    rp = {"clamp_sigma": 0.5}
    clean, cinfo = clamp(h0, h1, h2, rp)
    # a position outside the image never counts: a corner's window is 3 x 3, an edge's 3 x 5, the interior's all 25
    n = cinfo["window"].sum(-1)
    assert n[0, 0] == 9 and n[H - 1, W - 1] == 9 and n[0, 5] == 15 and n[7, 0] == 15 and (n[2:-2, 2:-2] == 25).all()
    assert cinfo["window"][0, 0].tolist() == [dy >= 0 and dx >= 0 for dy, dx in WINDOW]
    y, x = 9, 13
    b1, b2 = h1.copy(), h2.copy()
    if what == "index":
        b1[y, x, 3] = index_bits(np.array([3], np.int32))[0]
    elif what == "valid":
        b2[y, x, 3] = 0
    else:
        b2[y, x, 1] = np.inf
    got, info = clamp(h0, b1, b2, rp)
    for k, (dy, dx) in enumerate(WINDOW):       # the pixel that sees it at (dy, dx) does not count it; every other tap stays
        assert info["window"][y - dy, x - dx, k] == (what == "index" and (dy, dx) == (0, 0))        # (its own index is its own)
    assert info["window"].sum() == cinfo["window"].sum() - (25 if what != "index" else 24 + 24)
    far = np.ones((H, W), bool)
    far[y - 2:y + 3, x - 2:x + 3] = False
    assert np.array_equal(_bits(got[far]), _bits(clean[far]))
    near = ~far
    near[y, x] = False
    assert (_bits(got[near]) != _bits(clean[near])).any()
    if what == "index":     # the pixel itself: only its own tap matches it, fewer than two: left alone
        assert info["window"][y, x].sum() == 1 and np.array_equal(_bits(got[y, x]), _bits(h0[y, x]))


def test_fewer_than_two_counted_taps_leave_the_pixel_alone():
    rng = np.random.default_rng(10)
    h0, h1, h2 = _field(rng)
    h0[..., :3] += 7                    # far outside every box
    h2[..., 3] = 0
    h2[4, 4, 3] = h2[4, 6, 3] = h2[12, 20, 3] = 1
    got, info = clamp(h0, h1, h2, {"clamp_sigma": 0.5})
    n = info["window"].sum(-1)
    assert n[12, 20] == 1 and n[4, 4] == 2 and n[4, 5] == 2 and n.max() == 2
    assert not info["applied"][12, 20] and np.array_equal(_bits(got[12, 20]), _bits(h0[12, 20]))
    assert info["moved"][4, 5] and info["moved"][n == 2].all() and not info["moved"][n < 2].any()
    assert np.array_equal(_bits(got[n < 2]), _bits(h0[n < 2]))
    # a pixel without history (len < 2) is not clamped whatever its window holds
    h2[..., 3] = 1
    h0[3, 3, 3], h0[5, 5, 3] = 1, 0
    got, info = clamp(h0, h1, h2, {"clamp_sigma": 0.5})
    assert not info["applied"][3, 3] and not info["applied"][5, 5] and info["moved"].sum() == H * W - 2
    assert np.array_equal(_bits(got[3, 3]), _bits(h0[3, 3])) and np.array_equal(_bits(got[5, 5]), _bits(h0[5, 5]))


def loaded_case(w, h, seed):
    """the synthetic history the GPU test loads, here over a host-made view of the same size"""
    rng = np.random.default_rng(seed)
    idx = (np.add.outer(np.arange(h), np.arange(w)) // 7 % 3).astype(np.int32) - 1
    t = (F(1) + rng.random((h, w), dtype=F)).astype(F)
    return synthetic_history(rng, idx, t)


@pytest.mark.parametrize("broken", BROKEN)
@pytest.mark.parametrize("w,h", [(37, 29), (65, 17)])
def test_a_broken_reference_is_rejected(broken, w, h):
    """window_order takes the window dx then dy (another order of the sums); sample_variance divides by n - 1; no_halo stops the
    window at the 32 x 8 tile's border.  The synthetic history that tests/test_gpu_temporal_response.py loads (and holds the device
    to, bit for bit, through the intact form) tells each from the intact form."""
    h0, h1, h2 = loaded_case(w, h, w * h)
    rp = {"clamp_sigma": 0.5}
    want, info = clamp(h0, h1, h2, rp)
    assert info["moved"].any() and info["kept"].any() and info["halo"].any()
    got, _ = clamp(h0, h1, h2, rp, broken)
    differ = (_bits(got) != _bits(want)).any(-1)
    assert differ.mean() >= (0.01 if broken == "window_order" else 0.05), (broken, differ.mean())


def test_parameters_and_null_context():
    L = _lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/myraytracer_amd.h").read()
    assert C.sizeof(_lib.MrtTemporalResponse) == 32 and hdr.count("/* 32 bytes */") == 2
    assert api.temporal_response_default() == {k: (v if k == "fast_history" else float(F(v))) for k, v in api.temporal_response_default().items()}
    assert set(api.temporal_response_default()) == set(R_DEFAULTS)
    p = _lib.MrtTemporalResponse()
    L.mrt_temporal_response_default(C.byref(p))
    assert p.size == 32 and p.enabled == 0 and list(p.reserved) == [0, 0, 0]
    assert 1 <= p.fast_history <= 16 and p.clamp_sigma > 0 and 0 <= p.antilag <= 1
    assert L.mrt_set_temporal_response(None, C.byref(p)) == MRT_OK            # ctx NULL: the setting alone
    assert L.mrt_set_temporal_response(None, None) == MRT_ERR_INVALID_ARG
    assert L.mrt_get_temporal_response(None, C.byref(p)) == MRT_ERR_INVALID_ARG
    L.mrt_temporal_response_default(None)                                     # (tolerated, as its siblings tolerate it)

    def with_(**kw):
        q = _lib.MrtTemporalResponse()
        L.mrt_temporal_response_default(C.byref(q))
        for k, v in kw.items():
            if k == "reserved":
                q.reserved[v] = 1
            else:
                setattr(q, k, v)
        return L.mrt_set_temporal_response(None, C.byref(q))
    for ok in ({"enabled": 0}, {"enabled": 1}, {"fast_history": 1}, {"fast_history": 16}, {"clamp_sigma": 1e-6}, {"clamp_sigma": 1e6},
               {"antilag": 0.0}, {"antilag": 1.0}):
        assert with_(**ok) == MRT_OK, ok
    for bad in ({"enabled": 2}, {"fast_history": 0}, {"fast_history": 17}, {"clamp_sigma": 0.0}, {"clamp_sigma": -1.0},
                {"clamp_sigma": float("nan")}, {"clamp_sigma": float("inf")}, {"antilag": -1e-6}, {"antilag": float(np.nextafter(F(1), F(2)))},
                {"antilag": float("nan")}, {"antilag": float("inf")}, {"size": 28}, {"size": 36}, {"reserved": 0}, {"reserved": 1},
                {"reserved": 2}):
        assert with_(**bad) == MRT_ERR_INVALID_ARG, bad
    for fn, args in ((L.mrt_debug_read_temporal_fast, (None, None, 0)), (L.mrt_debug_load_temporal_fast, (None, None))):
        assert fn(*args) == MRT_ERR_INVALID_ARG
