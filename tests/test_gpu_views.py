"""The diagnostic views (include/myraytracer_amd.h, "diagnostic views"; views.hip) on the GPU: mrt_set_view, mrt_read_view and
mrt_present(.. | MRT_PRESENT_VIEW) against tests/view_ref.py.  Every comparison is bit equality, or -- where the definition says
"a NaN" -- a NaN in the same position (view_ref.same).  Shapes: 1 x 1; 20 x 12 (partial 8 x 8 tiles both ways, two bands: the shape
of tests/test_gpu_present_sources.py); 67 x 17 (wider than a wave, with an odd tail)."""
import os
import subprocess

import numpy as np
import pytest

import view_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPES = ((1, 1), (20, 12), (67, 17))
SPP, DEPTH, SEED = 2, 8, 5
THRESHOLD = 0.02
FLOORS = (0.01, 0.5)
ERR_INVALID_ARG, ERR_NO_SCENE, ERR_TOO_SMALL, ERR_STATE = 1, 4, 6, 7
S_SPECIAL = (0.0, 1e-30, 1e-42, 3e30, np.nan, np.inf, -np.inf)          # 0, tiny (a normal and a subnormal), large, not finite
C_SPECIAL = ((np.nan, 0.5, 0.5), (np.inf, 0.0, 0.0), (0.0, -np.inf, 1.0), (np.inf, -np.inf, 0.0), (0.0, 0.0, 0.0), (1e30, 1e30, 1e30))
N_T = (0, 1, 2, 3, 1000)


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _state(mrt, w, h, frames=2, tracking=True, scene="default"):
    st = mrt.State(mrt.Args(w, h, SPP, DEPTH), seed=SEED)
    if tracking:
        st.set_noise_tracking(True)
    if scene == "default":
        st.set_world(mrt.scene_default())
    else:
        spheres, cam = mrt.scene_cover(1, True)         # the cover scene with glass
        st.set_world(spheres)
        st.set_camera(cam)
    if frames:
        st.render(frames)
    return st


def _crafted(w, h):
    """(rgba, S, n_t): every special S and every special texel, alone and together, and the five frame counts over the tiles"""
    n, off = w * h, w + h
    rng = np.random.default_rng(100 * w + h)
    rgba = rng.uniform(0.0, 2.0, (n, 4)).astype(F)
    rgba[:, 3] = 1
    S = (rng.uniform(0.0, 1.0, n) ** 4 * 0.05).astype(F)
    for i in range(0, n, 3):
        S[i] = S_SPECIAL[(i // 3 + off) % len(S_SPECIAL)]
    for i in range(0, n, 5):
        rgba[i, :3] = C_SPECIAL[(i // 5 + off) % len(C_SPECIAL)]
    tiles = -(-w // 8) * -(-h // 8)
    n_t = np.array([N_T[(t + off) % len(N_T)] for t in range(tiles)], np.uint32)
    return rgba.reshape(h, w, 4), S.reshape(h, w), n_t


def _loaded(mrt, w, h, diverged):
    """A context whose accumulation is the crafted one, and (rgba, S, K per pixel or the one K, q of TILE_FRAMES)"""
    st = _state(mrt, w, h)
    rgba, S, n_t = _crafted(w, h)
    st.debug_load_accumulation(rgba, S, n_t if diverged else None)
    if diverged:
        max_w = st.args.max_framebuffer_weight
        K = view_ref.per_pixel([F(mrt.noise_factor(int(n), max_w)) for n in n_t], h, w)
        frames = view_ref.per_pixel(n_t.astype(F), h, w)
    else:
        st.noise_query(THRESHOLD, FLOORS[0])
        K = F(st.noise_result()["noise_factor"])        # the factor the report uses at this point of the stream
        frames = np.full((h, w), F(st.frames_done), F)
    return st, rgba, S, K, frames


def _view(st, kind, ramp="grey", lo=0.0, hi=1.0, rel_floor=None):
    st.set_view(kind, ramp, lo, hi, rel_floor)
    return st.read_view()


@pytest.mark.parametrize("diverged", (False, True), ids=("uniform", "diverged"))
@pytest.mark.parametrize("w,h", SHAPES)
def test_crafted_accumulation(mrt, w, h, diverged):
    st, rgba, S, K, frames = _loaded(mrt, w, h, diverged)
    with st:
        assert np.isfinite(K).any() or (w, h) == (1, 1)
        se = _view(st, "noise_se")
        assert view_ref.same(se, view_ref.ramp(view_ref.noise_q(S, rgba, K, 0.0, False), "grey", 0.0, 1.0))
        for floor in FLOORS:
            got = _view(st, "noise_rel", rel_floor=floor)
            assert view_ref.same(got, view_ref.ramp(view_ref.noise_q(S, rgba, K, floor, True), "grey", 0.0, 1.0)), floor
        assert np.array_equal(_u32(_view(st, "tile_frames")), _u32(view_ref.ramp(frames, "grey", 0.0, 1.0)))
        # the NaN pixels are the report's non_finite ones
        st.noise_query(THRESHOLD, FLOORS[0])
        rep = st.noise_result()
        assert int(np.isnan(se[..., 0]).sum()) == rep["non_finite"] and rep["pixels"] + rep["non_finite"] == w * h
        if (w, h) != (1, 1):
            assert rep["non_finite"] > 0 and rep["pixels"] > 0
        assert (se[..., 3] == 1).all()


def _report_state(mrt, w, h, how):
    if how == "diverged":
        st = _state(mrt, w, h, frames=2)
        tiles = np.arange(-(-w // 8) * -(-h // 8))
        st.render_tiles(tiles[::2], 1)
    else:
        st = _state(mrt, w, h, frames=how)
    return st


@pytest.mark.parametrize("how", (1, 3, "diverged"), ids=("1-frame", "3-frames", "diverged"))
@pytest.mark.parametrize("w,h", SHAPES)
def test_consistent_with_the_noise_report(mrt, w, h, how):
    floor = FLOORS[0]
    with _report_state(mrt, w, h, how) as st:
        st.noise_query(THRESHOLD, floor)
        rep = st.noise_result()
        tiles = st.read_noise_tiles()
        rel = _view(st, "noise_rel", rel_floor=floor)[..., 0]
        se = _view(st, "noise_se")[..., 0]
        assert int(np.isnan(se).sum()) == rep["non_finite"] == 0
        if how == 1:
            assert np.isinf(se).all() and np.isinf(rep["noise_factor"])             # K = +inf: no estimate yet
        elif how == 3:
            assert np.isfinite(se).all()
        tr, tx = tiles.shape
        pad = np.zeros((tr * 8, tx * 8), F)
        pad[:h, :w] = np.where(np.isnan(rel), F(0), rel)
        assert np.array_equal(_u32(pad.reshape(tr, 8, tx, 8).max(axis=(1, 3))), _u32(tiles))
        with np.errstate(invalid="ignore"):
            assert int((rel > F(THRESHOLD)).sum()) == rep["above"]
        assert float(np.fmax.reduce(se, axis=None, initial=F(0))) == rep["max_se"]


def _guide_views_match(st):
    g = st.debug_read_guides()
    for kind in ("depth", "normal", "albedo", "sphere"):
        assert view_ref.same(_view(st, kind), view_ref.guide_view(kind, g, "grey", 0.0, 1.0)), kind
    return g


@pytest.mark.parametrize("scene", ("default", "cover-glass"))
@pytest.mark.parametrize("w,h", SHAPES)
def test_guide_views(mrt, w, h, scene):
    with _state(mrt, w, h, frames=1, tracking=False, scene=scene) as st:
        g0 = _guide_views_match(st)
        if (w, h) != (1, 1):
            assert (g0["index"] >= 0).any() and np.isinf(g0["t"][g0["index"] < 0]).all()
        # a new camera: the stale guides are rebuilt by the view itself (the view comes first here, the debug read second)
        cam = mrt.Camera(1, (0.3, 0.4, 1.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 70.0) if scene == "default" else \
            mrt.Camera(1, (10.0, 2.5, 4.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 25.0)
        st.set_camera(cam)
        depth = _view(st, "depth")
        g1 = _guide_views_match(st)
        assert view_ref.same(depth, view_ref.guide_view("depth", g1, "grey", 0.0, 1.0))
        if (w, h) != (1, 1):
            assert not np.array_equal(g0["t"], g1["t"])
        # new materials: the albedo changes and a Dielectric reads (1, 1, 1)
        hit = np.unique(g1["index"][g1["index"] >= 0])
        if hit.size == 0:
            return
        n = int(hit.max()) + 1
        m = np.zeros(n, mrt.MATERIAL_DTYPE)
        m["material_ty"] = np.where(np.arange(n) % 2 == 0, mrt.DIELECTRIC, mrt.LAMBERTIAN)
        m["albedo"] = np.stack([np.linspace(0.1, 0.9, n), np.full(n, 0.25), np.linspace(0.8, 0.2, n)], axis=1)
        m["param"] = np.where(np.arange(n) % 2 == 0, 1.5, 0.0)
        st.update_materials(0, m)
        albedo = _view(st, "albedo")
        g2 = _guide_views_match(st)
        assert view_ref.same(albedo, view_ref.guide_view("albedo", g2))
        glass = (g2["index"] >= 0) & (g2["index"] % 2 == 0)
        matte = (g2["index"] >= 0) & (g2["index"] % 2 == 1)
        assert (albedo[glass][:, :3] == 1).all()
        assert np.array_equal(albedo[matte][:, :3], m["albedo"][g2["index"][matte]].astype(F))
        assert np.array_equal(g2["index"], g1["index"])


@pytest.mark.parametrize("w,h", SHAPES[1:])
def test_mapping(mrt, w, h):
    st, rgba, S, K, _ = _loaded(mrt, w, h, True)
    with st:
        q = view_ref.noise_q(S, rgba, K, FLOORS[0], True)
        with np.errstate(invalid="ignore"):
            u = (q - F(0.02)) * (F(1) / (F(0.3) - F(0.02)))
            assert (u < 0).any() and (u > 1).any() and np.isposinf(q).any() and np.isnan(q).any() and ((u > 0) & (u < 1)).any()
        for lo, hi in ((0.02, 0.3), (0.3, 0.02)):
            for ramp in ("heat", "grey"):
                got = _view(st, "noise_rel", ramp, lo, hi, FLOORS[0])
                assert view_ref.same(got, view_ref.ramp(q, ramp, lo, hi)), (ramp, lo, hi)
                assert st.view() == {"kind": "noise_rel", "ramp": ramp, "lo": float(F(lo)), "hi": float(F(hi)), "rel_floor": float(F(FLOORS[0]))}
        heat = _view(st, "noise_rel", "heat", 0.02, 0.3, FLOORS[0])
        assert (heat[np.isnan(q)] == (1, 0, 1, 1)).all() and (heat[np.isposinf(q)] == (1, 0, 0, 1)).all()
        assert np.isfinite(heat).all() and (heat >= 0).all() and (heat <= 1).all()
        # a vector kind ignores the ramp, lo and hi
        a = _view(st, "sphere", "heat", 5.0, -3.0)
        assert np.array_equal(_u32(a), _u32(_view(st, "sphere", "grey", 0.0, 1.0)))


@pytest.mark.parametrize("w,h", SHAPES)
def test_through_the_ring(mrt, w, h):
    st, *_ = _loaded(mrt, w, h, True)
    with st:
        st.set_view("noise_rel", "heat", 0.02, 0.3, FLOORS[0])
        want = st.read_view()
        for fmt in ("rgba32f", "rgba16f", "rgba8", "bgra8"):
            for flip in (False, True):
                st.present(fmt, flip=flip, view=True)
                img, info = st.acquire_presented(newest=True, wait=True)
                st.release_presented()
                src = want[::-1] if flip else want
                if fmt == "rgba32f":
                    assert np.array_equal(img.view(np.uint32), _u32(src)), (fmt, flip)
                elif fmt == "rgba16f":
                    assert np.array_equal(img.view(np.uint16), mrt._lib.half_bits(src)), (fmt, flip)
                else:
                    assert np.array_equal(img, st.debug_present_encode(want, fmt, flip)), (fmt, flip)
                assert info["flags"] & 128 and bool(info["flags"] & 1) == flip
                assert (info["frames_done"], info["rows"], info["width"]) == (st.frames_done, h, w)
        # a grey view keeps its NaNs and infinities through the float format
        st.set_view("noise_se", "grey", 0.0, 1.0)
        want = st.read_view()
        st.present("rgba32f", flip=False, view=True)
        img, _ = st.acquire_presented(newest=True, wait=True)
        st.release_presented()
        assert view_ref.same(img, want)


def _refused(mrt, call, status, message):
    with pytest.raises(mrt.MrtError) as e:
        call()
    assert e.value.status == status and message in str(e.value), str(e.value)


def test_refusals(mrt):
    W, H = SHAPES[1]
    calls = lambda st: (("mrt_present", lambda: st.present("rgba32f", view=True)), ("mrt_read_view", st.read_view))
    # 1. a shard; before "no scene" (this one has none)
    with mrt.State(mrt.Args(W, H, SPP, DEPTH), seed=SEED, shard=(0, 2)) as st:
        for who, call in calls(st):
            _refused(mrt, call, ERR_STATE, f"{who}: a shard (world 2) has no views")
    # 2. no scene; before "tracking off" (the default view is a noise view, tracking is off)
    with mrt.State(mrt.Args(W, H, SPP, DEPTH), seed=SEED) as st:
        for who, call in calls(st):
            _refused(mrt, call, ERR_NO_SCENE, f"{who}: no scene")
    # (3. an empty image: mrt_create resolves a size of 0, so no context has one; the row stands behind "no scene" all the same)
    # 4. a noise kind with tracking off; the other kinds are served, and too small a buffer comes after the state
    with _state(mrt, W, H, tracking=False) as st:
        for kind in ("noise_se", "noise_rel"):
            st.set_view(kind)
            for who, call in calls(st):
                _refused(mrt, call, ERR_STATE, f"{who}: a noise view with noise tracking off")
        with pytest.raises(mrt.MrtError):
            st.acquire_presented()                                  # (nothing was queued by any of them)
        buf = np.empty(W * H * 4, F)
        L = mrt._lib.load()
        assert L.mrt_read_view(st._ctx, buf.ctypes.data, 1) == ERR_STATE
        st.set_view("tile_frames", "grey", 0.0, 1.0)
        assert L.mrt_read_view(st._ctx, buf.ctypes.data, buf.size - 1) == ERR_TOO_SMALL
        assert L.mrt_last_error(st._ctx).decode() == f"mrt_read_view: need {W * H * 4} floats"
        assert (st.read_view()[..., :3] == 2).all()
        # VIEW with each other source bit, each with a reason of its own; 4 and 64 stay undefined
        lib = mrt._lib
        for bit in (lib.PRESENT_GATHERED, lib.PRESENT_DENOISED, lib.PRESENT_TEMPORAL, lib.PRESENT_GATHERED_DENOISED):
            for flip in (0, 1):
                flags = lib.PRESENT_VIEW | bit | flip
                assert L.mrt_present(st._ctx, lib.PRESENT_RGBA8_SRGB, flags) == ERR_INVALID_ARG
                assert L.mrt_last_error(st._ctx).decode() == ("mrt_present: a view is computed from the accumulation, not from another source "
                                                              f"(flags 0x{flags:x}: with FLIP_Y only)")
        for flags in (128 | 4, 128 | 64, 256 | 128):
            assert L.mrt_present(st._ctx, lib.PRESENT_RGBA8_SRGB, flags) == ERR_INVALID_ARG
            assert L.mrt_last_error(st._ctx).decode() == f"mrt_present: flags 0x{flags:x}"


def test_the_setting_survives_and_a_refused_one_changes_nothing(mrt):
    import ctypes as C
    W, H = SHAPES[1]
    with _state(mrt, W, H) as st:
        default = mrt.view_default()
        assert st.view() == default
        st.set_view("depth", "grey", 0.5, 8.0, 0.125)
        want = {"kind": "depth", "ramp": "grey", "lo": 0.5, "hi": 8.0, "rel_floor": 0.125}
        assert st.view() == want
        L = mrt._lib.load()
        for field, bad in (("kind", 9), ("ramp", 2), ("hi", 0.5), ("lo", float("nan")), ("rel_floor", -1.0), ("size", 16)):
            v = mrt._lib.MrtView()
            L.mrt_get_view(st._ctx, C.byref(v))
            setattr(v, field, bad)
            assert L.mrt_set_view(st._ctx, C.byref(v)) == ERR_INVALID_ARG and L.mrt_last_error(st._ctx).decode().startswith("mrt_set_view: size")
            assert st.view() == want, field
        st.reset()
        assert st.view() == want
        st.set_world(mrt.scene_default())
        assert st.view() == want
        st.set_camera(mrt.Camera(1, (0.0, 0.5, 1.0)))
        assert st.view() == want
        st.set_shard(0, 2)
        assert st.view() == want
        st.set_shard(0, 1)
        st.render(1)
        assert view_ref.same(st.read_view(), view_ref.guide_view("depth", st.debug_read_guides(), "grey", 0.5, 8.0))


KINDS = ("noise_rel", "sphere", "tile_frames", "noise_se", "depth", "normal", "albedo")


def _sequence(mrt, w, h, views):
    """What a caller reads of an accumulation that goes uniform -> diverged, with views between the steps or without"""
    out = {}
    with _state(mrt, w, h, frames=0) as st:
        st.set_denoise_adaptive(True)
        k = 0

        def look():
            nonlocal k
            if views:
                st.set_view(KINDS[k % len(KINDS)], ("heat", "grey")[k % 2], 0.0, 0.5)
                if k % 2:
                    st.read_view()
                else:
                    st.present(("rgba8", "rgba32f")[k // 2 % 2], view=True)
                k += 1
        look()
        st.render(2)
        look()
        out["fb2"] = st.read_framebuffer()
        look()
        out["S2"] = st.read_noise()
        out["den2"] = st.read_denoised()
        look()
        st.render_tiles(np.arange(-(-w // 8) * -(-h // 8))[::2], 1)
        look()
        look()
        out["tiles"] = st.tile_frames()
        out["fb3"] = st.read_framebuffer()
        look()
        out["S3"] = st.read_noise()
        look()
        out["den3"] = st.read_denoised()
        c = st.read_counters()
        out["counters"] = np.array([c["samples"], c["world_hit_calls"], c["rng_draws"]], np.uint64)
    return out


def test_views_change_nothing_else(mrt):
    w, h = SHAPES[1]
    plain, viewed = _sequence(mrt, w, h, False), _sequence(mrt, w, h, True)
    assert sorted(plain) == sorted(viewed)
    for name in plain:
        assert np.array_equal(plain[name].view(np.uint32 if plain[name].dtype == F else plain[name].dtype),
                              viewed[name].view(np.uint32 if viewed[name].dtype == F else viewed[name].dtype)), name
    assert sorted(set(plain["tiles"].ravel().tolist())) == [2, 3]


@pytest.mark.parametrize("w,h", SHAPES[1:])
def test_a_view_of_queued_frames_is_the_view_after_the_sync(mrt, w, h):
    with _state(mrt, w, h, frames=0) as st:
        st.set_view("noise_rel", "grey", 0.0, 1.0)
        st.render(4)
        st.present("rgba32f", flip=False, view=True)            # behind the four frames' blends, no host wait
        st.sync()
        want = st.read_view()
        img, info = st.acquire_presented(newest=True, wait=True)
        st.release_presented()
        assert view_ref.same(img, want) and info["frames_done"] == 4
        assert np.isfinite(want).all()


def _read_pfm(path, w, h):
    raw = open(path, "rb").read()
    head = f"PF\n{w} {h}\n-1.0\n".encode()
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], F).reshape(h, w, 3)


def test_native_runner_writes_a_view(mrt, tmp_path):
    w, h = SHAPES[1]
    exe = os.path.join(ROOT, "myraytracer_amd", "lib", "native_runner")
    common = [exe, "--width", str(w), "--height", str(h), "--samples-per-frame", str(SPP), "--ray-depth", str(DEPTH), "--frames", "1"]
    r = subprocess.run(common + ["--view", "sphere", "--view-out", str(tmp_path / "x.pfm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    with _state(mrt, w, h, frames=1, tracking=False) as st:
        want = _view(st, "sphere", "heat", 0.0, 0.1)
    assert np.array_equal(_read_pfm(tmp_path / "x.pfm", w, h).view(np.uint32), _u32(want[..., :3]))
    assert len(np.unique(want.reshape(-1, 4), axis=0)) >= 3              # (the ground, a sphere or two, the sky)
    for bad in (["--view", "sphere"], ["--view", "spheres", "--view-out", str(tmp_path / "y.pfm")],
                ["--view", "depth:1:1", "--view-out", str(tmp_path / "y.pfm")]):
        r = subprocess.run(common + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--view" in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "y.pfm")
