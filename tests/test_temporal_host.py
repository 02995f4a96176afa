"""Temporal reprojection on the host (include/myraytracer_amd.h, "temporal reprojection"): the float32 restatement
(tests/temporal_ref.py, which the GPU tests compare the device against bit for bit) against a plain float64 form of the same
definition and on the cases the definition singles out; three references broken on purpose, which those properties must reject;
the parameter checks that need no context.  The scenes here are made on the host: rays as the guide pass makes them, closest
hits in float64."""
import ctypes as C
import re

import numpy as np
import pytest

from myraytracer_amd import _lib, api
from denoise_ref import lum
from temporal_ref import BROKEN, T_DEFAULTS, camera_matrix, image, index_bits, step, step_f64, variance_field

F = np.float32
MRT_OK, MRT_ERR_INVALID_ARG = 0, 1
H, W = 19, 27
SPHERES = np.array([[0.0, -100.5, -1.0, 100.0], [0.0, 0.0, -1.2, 0.5], [-1.0, 0.1, -1.5, 0.45], [0.9, -0.1, -1.0, 0.35]], F)
LOOKAT = api.Camera(mode=1, lookfrom=(0.4, 0.3, 0.8), lookat=(0.0, 0.0, -1.2), vup=(0.0, 1.0, 0.0), vfov_deg=60.0,
                    defocus_angle_deg=0.0, focus_dist=1.0)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def guide_rays(raw, h=H, w=W):
    """the centre ray of every pixel, as denoise.hip's guide_rays_kernel forms it (to float32 rounding)"""
    side = F(2) / F(h)
    x, y = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    vx = ((x + F(0.5)) - F(0.5) * F(w)) * side + F(0.5) * side
    vy = ((y + F(0.5)) - F(0.5) * F(h)) * side + F(0.5) * side
    if raw is None or raw.mode == 0:
        d = np.stack([vx, vy, np.full_like(vx, -1)], -1)
        o = np.zeros((h, w, 3), F)
    else:
        su, sv, fw = (np.array(list(v), F) for v in (raw.su, raw.sv, raw.fw))
        d = (vx[..., None] * su + vy[..., None] * sv) - fw
        o = np.broadcast_to(np.array(list(raw.origin), F), (h, w, 3)).copy()
    d = (d / np.sqrt((d * d).sum(-1, keepdims=True))).astype(F)
    return np.concatenate([o, d], -1).astype(F)


def first_hits(rays, xyzr):
    """(index, t) of the closest hit over [0.001, 1e4), float64 inside"""
    o, d = rays[..., :3].astype(np.float64), rays[..., 3:].astype(np.float64)
    best = np.full(rays.shape[:2], np.inf)
    idx = np.full(rays.shape[:2], -1, np.int32)
    for k, (cx, cy, cz, r) in enumerate(np.asarray(xyzr, np.float64)):
        oc = o - (cx, cy, cz)
        b = (oc * d).sum(-1)
        disc = b * b - ((oc * oc).sum(-1) - r * r)
        with np.errstate(invalid="ignore"):
            sq = np.sqrt(disc)
        for root in (-b - sq, -b + sq):
            ok = (disc >= 0) & (root >= 0.001) & (root < 1e4) & (root < best)
            best = np.where(ok, root, best)
            idx = np.where(ok, k, idx)
    return idx, best.astype(F)


def view(cam, xyzr):
    raw = None if cam is None else api.camera_derive(cam)
    rays = guide_rays(raw)
    idx, t = first_hits(rays, xyzr)
    return {"raw": raw, "rays": rays, "index": idx, "t": t, "xyzr": np.asarray(xyzr, F)}


def empty_history():
    return np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)


def advance(prev, now, cur, h0, h1, params=None, broken=None):
    """one step from the state `prev` (None: no previous state, the history is empty) to `now`"""
    M, o = camera_matrix((prev or now)["raw"])
    return step(cur, now["rays"], now["index"], now["t"], now["xyzr"], (prev or now)["xyzr"], M, o, h0, h1, params, broken)


def frame(rng, nonfinite=False):
    cur = rng.random((H, W, 4), dtype=F)
    cur[..., 3] = 1
    if nonfinite:
        cur[3, 4, 0] = np.nan
        cur[10, 20, 2] = np.inf
    return cur


def moved(xyzr, rng, shift=0.04, scale=0.1):
    out = np.array(xyzr, F)
    out[1:, :3] += (rng.random((len(out) - 1, 3), dtype=F) - F(0.5)) * F(2 * shift)
    out[1:, 3] *= F(1) + (rng.random(len(out) - 1, dtype=F) - F(0.5)) * F(2 * scale)
    return out


CAM2 = api.Camera(mode=1, lookfrom=(0.45, 0.32, 0.78), lookat=(0.02, 0.0, -1.2), vup=(0.02, 1.0, 0.0), vfov_deg=60.0,
                  defocus_angle_deg=0.0, focus_dist=1.0)


def moving_pair(seed, towards=0.0):
    """(the state before, the state after, a history of three frames at the state before): every small sphere translated and its
    radius changed, the camera moved and turned; towards: the spheres also come this share of their distance nearer"""
    rng = np.random.default_rng(seed)
    a = view(LOOKAT, SPHERES)
    x1 = moved(SPHERES, rng)
    if towards:
        eye = np.array(LOOKAT.lookfrom, F)
        x1[1:, :3] = eye + (x1[1:, :3] - eye) * F(1 - towards)
    b = view(CAM2, x1)
    h0, h1 = empty_history()
    for _ in range(3):
        h0, h1, _ = advance(a, a, frame(rng, nonfinite=True), h0, h1)
    return a, b, h0, h1, rng


def agreement(got, ref, a, b, h0, h1, cur, params=None):
    """the float32 form `got` against the float64 form: (share of texels whose taps differ, the largest |difference| / (atol +
    rtol |ref|) over the others)"""
    g0, g1, info = got
    r0, r1, taps = ref
    same = (info["taps"] == taps).all(-1)
    fin = np.isfinite(cur[..., :3]).all(-1) & same
    worst = 0.0
    for g, r in ((g0[..., :3], r0[..., :3]), (g0[..., 3], r0[..., 3]), (g1[..., :2], r1[..., :2])):
        g, r = g[fin].astype(np.float64), r[fin]
        worst = max(worst, float((np.abs(g - r) / (2e-6 + 2e-4 * np.abs(r))).max()))
    return 1.0 - same.mean(), worst


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("params", [{}, {"max_history": 3, "depth_tol": 0.2}])
def test_float32_form_matches_float64(seed, params):
    a, b, h0, h1, rng = moving_pair(seed)
    cur = frame(rng, nonfinite=True)
    M, o = camera_matrix(a["raw"])
    args = (cur, b["rays"], b["index"], b["t"], b["xyzr"], a["xyzr"], M, o, h0, h1, params)
    got = step(*args)
    assert got[0].dtype == F and got[1].dtype == F
    differ, worst = agreement(got, step_f64(*args), a, b, h0, h1, cur)
    # rtol 2e-4 / atol 2e-6, tests/test_denoise_var_host.py's: the step is a dozen float32 operations on values of order 1
    assert differ <= 0.01 and worst <= 1.0, (differ, worst)
    # the case is no trivial one: most pixels found history, some restarted
    found = got[2]["found"]
    assert found.mean() >= 0.5 and (~found).mean() >= (0.02 if not params else 0.005)     # (a depth_tol of 0.2 forgives more)
    # a texel that is not finite is kept with an empty history
    for y, x in ((3, 4), (10, 20)):
        assert got[0][y, x, 3] == 0 and np.array_equal(_bits(got[0][y, x, :3]), _bits(cur[y, x, :3]))
    assert np.array_equal(_bits(got[1][..., 3]), _bits(index_bits(b["index"]))) and np.array_equal(_bits(got[1][..., 2]), _bits(b["t"]))


@pytest.mark.parametrize("broken", BROKEN)
def test_a_broken_reference_is_rejected(broken):
    """no_scale drops k = r0 / r1; tap_order weighs the tap (x0 + i, y0 + j) with i and j exchanged; depth_t tests the taps'
    distance against the current t instead of te.  The agreement with the float64 form above rejects each (for depth_t on
    spheres that come 15 % nearer, three times depth_tol; the intact form still passes there)."""
    a, b, h0, h1, rng = moving_pair(3, towards=0.15 if broken == "depth_t" else 0.0)
    cur = frame(rng)
    M, o = camera_matrix(a["raw"])
    args = (cur, b["rays"], b["index"], b["t"], b["xyzr"], a["xyzr"], M, o, h0, h1, None)
    ref = step_f64(*args)
    differ, worst = agreement(step(*args), ref, a, b, h0, h1, cur)
    assert differ <= 0.01 and worst <= 1.0
    differ, worst = agreement(step(*args, broken=broken), ref, a, b, h0, h1, cur)
    assert differ > 0.01 or worst > 1.0, (broken, differ, worst)


@pytest.mark.parametrize("cam", [None, LOOKAT])
def test_identity_motion_returns_each_texels_own_history(cam):
    rng = np.random.default_rng(5)
    a = view(cam, SPHERES)
    h0, h1 = empty_history()
    first = frame(rng)
    h0, h1, info = advance(None, a, first, h0, h1)
    assert not info["found"].any() and np.array_equal(_bits(h0[..., :3]), _bits(first[..., :3])) and (h0[..., 3] == 1).all()
    assert np.array_equal(_bits(h1[..., 0]), _bits(lum(first))) and np.array_equal(_bits(h1[..., 1]), _bits(lum(first) * lum(first)))
    # the same picture again: every pixel finds its own texel.  fx is x up to the rounding of a handful of operations on values
    # below W, so the bilinear weight that leaks to a neighbour -- whose colour differs by at most 1 -- is below 64 * 2^-24 * W
    g0, g1, info = advance(a, a, first, h0, h1)
    assert info["found"].all() and (g0[..., 3] == 2).all()
    leak = 64 * 2.0 ** -24 * W
    assert np.abs(g0[..., :3] - first[..., :3]).max() <= leak
    assert np.abs(g1[..., 0] - lum(first)).max() <= leak


def test_a_constant_sequence_keeps_variance_zero_and_passes_through():
    a = view(LOOKAT, SPHERES)
    guides = {"index": a["index"], "t": a["t"], "normal": -a["rays"][..., 3:], "albedo": np.ones((H, W, 3), F)}
    h0, h1 = empty_history()
    cur = np.zeros((H, W, 4), F)            # (0: every sum is exact whatever the weights, as in test_denoise_var_host.py)
    cur[..., 3] = 1
    for k in range(1, 7):
        h0, h1, _ = advance(a, a, cur, h0, h1)
        assert (h0[..., 3] == k).all()
        for spatial_len in (1, 4, 16):
            cv = variance_field(h0, h1, guides, None, spatial_len)
            assert np.array_equal(cv[..., 3], np.zeros((H, W), F))
            assert np.array_equal(_bits(image(h0, h1, cur[..., 3], guides, None, spatial_len)), _bits(cur))


@pytest.mark.parametrize("max_history", [1, 3, 32])
def test_identical_weight_frames_give_the_running_mean(max_history):
    rng = np.random.default_rng(7)
    a = view(None, SPHERES)
    h0, h1 = empty_history()
    values = rng.random(8)
    mean = 0.0
    for k, v in enumerate(values, 1):
        cur = np.full((H, W, 4), F(v), F)       # (constant over the image: the bilinear leak has nothing to mix)
        h0, h1, _ = advance(a, a, cur, h0, h1, {"max_history": max_history})
        n = min(k, max_history)
        mean = mean + (float(F(v)) - mean) / n  # the running mean while k <= max_history, the EMA of weight 1 / max_history after
        assert (h0[..., 3] == n).all()
        np.testing.assert_allclose(h0[..., :3], mean, rtol=1e-5)
        if k <= max_history:
            np.testing.assert_allclose(h0[..., :3], np.mean(values[:k].astype(F)), rtol=1e-5)


@pytest.mark.parametrize("what", ["index", "depth", "len", "colour"])
def test_a_tap_that_does_not_qualify_is_ignored(what):
    rng = np.random.default_rng(9)
    a = view(LOOKAT, SPHERES)
    h0, h1 = empty_history()
    for _ in range(2):
        h0, h1, _ = advance(a, a, frame(rng), h0, h1)
    cur = frame(rng)
    clean0, clean1, info = advance(a, a, cur, h0, h1)
    assert info["found"].all()

    def spoil(b0, b1, where):
        if what == "index":
            b1[..., 3][where] = index_bits(a["index"] + 1)[where]
        elif what == "depth":
            b1[..., 2][where] = F(1e6)          # (beyond every hit's tolerance, the leak taps of grazing neighbours included)
        elif what == "len":
            b0[..., 3][where] = 0
        else:
            b0[..., 1][where] = np.nan
    # every texel spoilt: every pixel restarts (a miss has no depth test: only the hits do)
    b0, b1 = h0.copy(), h1.copy()
    spoil(b0, b1, np.ones((H, W), bool))
    g0, g1, info = advance(a, a, cur, b0, b1)
    restarted = a["index"] >= 0 if what == "depth" else np.ones((H, W), bool)
    assert not info["found"][restarted].any() and info["found"][~restarted].all()
    assert np.array_equal(_bits(g0[restarted][:, :3]), _bits(cur[restarted][:, :3])) and (g0[restarted][:, 3] == 1).all()
    assert np.array_equal(_bits(g1[restarted][:, 0]), _bits(lum(cur)[restarted]))
    # one texel spoilt: nothing further than one pixel away changes, and the pixel itself no longer takes its own texel
    y, x = np.argwhere(a["index"] >= 0)[len(np.argwhere(a["index"] >= 0)) // 2]
    b0, b1 = h0.copy(), h1.copy()
    one = np.zeros((H, W), bool)
    one[y, x] = True
    spoil(b0, b1, one)
    g0, g1, _ = advance(a, a, cur, b0, b1)
    far = np.ones((H, W), bool)
    far[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = False
    assert np.array_equal(_bits(g0[far]), _bits(clean0[far])) and np.array_equal(_bits(g1[far]), _bits(clean1[far]))
    assert not np.array_equal(_bits(g0[y, x]), _bits(clean0[y, x]))


def test_variance_of_the_moments_and_the_short_histories():
    rng = np.random.default_rng(11)
    a = view(LOOKAT, SPHERES)
    guides = {"index": a["index"], "t": a["t"], "normal": -a["rays"][..., 3:], "albedo": np.ones((H, W, 3), F)}
    h0 = rng.random((H, W, 4), dtype=F)
    h1 = rng.random((H, W, 4), dtype=F)
    h0[..., 3] = rng.integers(0, 7, (H, W)).astype(F)
    h0[2, 3, 0] = np.nan
    cv = variance_field(h0, h1, guides, None, 4)
    n = h0[..., 3]
    long_ = n >= 4
    want = np.maximum(0, h1[..., 1].astype(np.float64) - h1[..., 0].astype(np.float64) ** 2) / np.maximum(n - 1.0, 1)
    np.testing.assert_allclose(cv[..., 3][long_], want[long_], rtol=1e-5, atol=1e-7)
    assert (cv[..., 3][n == 0] == 0).all() and (cv[..., 3] >= 0).all() and np.array_equal(_bits(cv[..., :3]), _bits(h0[..., :3]))
    short = (n >= 1) & ~long_ & np.isfinite(h0[..., :3]).all(-1)
    assert short.any() and (cv[..., 3][short] > 0).any()        # (0 where no neighbour qualifies: the centre tap alone)
    # spatial_len 1: only a history of one frame is short (a variance of one sample does not exist)
    cv1 = variance_field(h0, h1, guides, None, 1)
    with np.errstate(all="ignore"):
        moments = np.fmax(F(0), h1[..., 1] - h1[..., 0] * h1[..., 0]) / (n - F(1))
    assert np.array_equal(_bits(cv1[..., 3][n >= 2]), _bits(moments[n >= 2]))


def test_parameters_and_null_context():
    L = _lib.load()
    hdr = open(__file__.rsplit("/tests/", 1)[0] + "/include/myraytracer_amd.h").read()
    assert C.sizeof(_lib.MrtTemporalParams) == 32 and "/* 32 bytes */" in hdr
    assert re.search(r"#define MRT_PRESENT_TEMPORAL 16u", hdr) and _lib.PRESENT_TEMPORAL == 16
    assert re.search(r"#define MRT_ABI_VERSION 4\b", hdr)
    assert api.temporal_params_default() == T_DEFAULTS | {"depth_tol": float(F(0.05))}
    p = _lib.MrtTemporalParams()
    L.mrt_temporal_params_default(C.byref(p))
    assert p.size == 32 and list(p.reserved) == [0, 0, 0, 0]
    assert L.mrt_set_temporal(None, 1, C.byref(p)) == MRT_OK            # ctx NULL: the parameters alone
    assert L.mrt_set_temporal(None, 1, None) == MRT_ERR_INVALID_ARG

    def with_(**kw):
        q = _lib.MrtTemporalParams()
        L.mrt_temporal_params_default(C.byref(q))
        for k, v in kw.items():
            if k == "reserved":
                q.reserved[v] = 1
            else:
                setattr(q, k, v)
        return L.mrt_set_temporal(None, 1, C.byref(q))
    for ok in ({"max_history": 1}, {"max_history": 256}, {"spatial_len": 1}, {"spatial_len": 16}, {"depth_tol": 1e-6}, {"depth_tol": 10.0}):
        assert with_(**ok) == MRT_OK, ok
    for bad in ({"max_history": 0}, {"max_history": 257}, {"spatial_len": 0}, {"spatial_len": 17}, {"depth_tol": 0.0},
                {"depth_tol": -0.05}, {"depth_tol": float("nan")}, {"depth_tol": float("inf")}, {"size": 28}, {"size": 36},
                {"reserved": 0}, {"reserved": 3}):
        assert with_(**bad) == MRT_ERR_INVALID_ARG, bad
    for fn, args in ((L.mrt_get_temporal, (None, None, C.byref(p))), (L.mrt_temporal_step, (None,)), (L.mrt_temporal_reset, (None,)),
                     (L.mrt_read_temporal, (None, None, 0)), (L.mrt_debug_read_temporal, (None, None, None, None, 0)),
                     (L.mrt_debug_load_temporal, (None, None, None, None, 0, None))):
        assert fn(*args) == MRT_ERR_INVALID_ARG
