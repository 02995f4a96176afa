"""Converged renders against an independent float64 ground truth (tests/radiometry_ref.py), on the CPU: the truth's pieces
against exact answers, its Monte-Carlo integrator against its closed forms, a committed fixture against a fresh run, and the
ORACLE -- the root of trust of every bit-parity test -- against the truth in both RNG modes: unbiased per pixel, the variance
independent samples give, no correlation between neighbouring pixels or consecutive frames."""
import os

import numpy as np
import pytest

import radiometry_ref as R
from common import to_oracle_spheres

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H = R.WIDTH, R.HEIGHT
STREAM, COUNTER = 0, 1
# about 4,096 samples per pixel in several frames x spp splits; counter mode also above 64 spp (more than one layer is summed)
SPLITS = {STREAM: ((1, 4096), (64, 64), (4096, 1)), COUNTER: ((1, 4096), (64, 64), (4096, 1), (16, 256))}


def fixture(name):
    with np.load(os.path.join(GOLDEN, f"radiometry_{name}.npz")) as f:
        return {k: (int(f[k]) if k == "n" else f[k]) for k in f.files}


_truth = {}


def truth(name):
    """Closed form on the smooth pixels; on the others (a silhouette, the edge of total reflection: no bounded quadrature error)
    the committed fixture of integrator (c)."""
    if name not in _truth:
        _truth[name] = R.truth(name, fixture(name) if name != "sky" else None)
    return _truth[name]


def oracle_camera(O, cam):
    if cam is None:
        return O.pinhole_camera()
    return O.lookat_camera(cam["lookfrom"], cam["lookat"], cam["vup"], cam["vfov"], cam["defocus"], cam["focus"])


def oracle_render(O, name, seed, frames, spp, rng_mode, max_w=1.0):
    sc = R.SCENES[name]
    sp = sc["spheres"]
    if len(sp) == 0:                                     # the oracle packs at least one sphere: one far behind the camera
        sp = R.spheres(((0, 0, 50), 1.0, R.LAMBERTIAN, (0.5, 0.5, 0.5), 0.0))
    packed = O.pack_world(to_oracle_spheres(O, sp))
    return O.render(W, H, spp, sc["depth"], packed, oracle_camera(O, sc["cam"]), seed, frames=frames, max_w=max_w, rng_mode=rng_mode)


# ------------------------------------------------------------------ the truth's pieces

def test_cosine_distribution_moments_by_quadrature():
    """E[y] = (2/3) n_y and E[y^2] = 1/4 + n_y^2 / 4 of a direction cosine-distributed about n, by dense quadrature."""
    th = (np.arange(2000) + 0.5) * (np.pi / 2 / 2000)
    ph = (np.arange(2000) + 0.5) * (2 * np.pi / 2000)
    T, P = np.meshgrid(th, ph, indexing="ij")
    wgt = np.cos(T) * np.sin(T)
    wgt /= wgt.sum()
    for n in ((0, 1, 0), (0.6, 0.0, 0.8), (0.3, -0.5, 0.81240384)):
        n = np.array(n) / np.linalg.norm(n)
        a = np.cross(n, (1, 0, 0) if abs(n[0]) < 0.9 else (0, 1, 0))
        a /= np.linalg.norm(a)
        b = np.cross(n, a)
        y = np.cos(T) * n[1] + np.sin(T) * (np.cos(P) * a[1] + np.sin(P) * b[1])
        assert abs((wgt * y).sum() - 2 / 3 * n[1]) < 1e-6
        assert abs((wgt * y * y).sum() - (0.25 + 0.25 * n[1] ** 2)) < 1e-6


def test_xoshiro_model_known_answer():
    s = np.array([[1], [2], [3], [4]], np.uint32)
    assert [int(R.xoshiro128plus(s)[0]) for _ in range(8)] == [5, 12295, 25178119, 27286542, 39879690, 1140358681, 3276312097,
                                                               4110231701]
    assert s[:, 0].tolist() == [857776784, 3957087773, 2428778008, 3837013768]
    sd = R.xor_shuffle_spread(8, n_c=64, n_a=2048)
    assert (sd > 0.05).all() and (sd < 1.0).all()        # the outputs from a and a ^ c ARE correlated, c by c
    assert 0.0 < R.xor_shuffle_allowance(64, 64) < 1.0 and R.xor_shuffle_allowance(64, 1) == 0.0


def test_dielectric_tree_probabilities_sum_to_one():
    for name in ("glass", "glass-low"):
        cf = R.closed_form(name, G=4)
        assert np.abs(cf["prob"] - 1.0).max() < 1e-12
        assert (cf["var"] >= 0).all() and np.isfinite(cf["mu"]).all()


def test_glass_of_ior_one_is_invisible():
    """Refraction at ior 1 changes no direction.  Schlick's approximation still reflects (1 - cos)^5 of the light at r0 = 0 (the
    material's definition, not an error of the truth), so the image equals the sky's exactly only through the refracted paths:
    with the reflected share taken out, and to 1e-4 where the sphere is seen head-on."""
    rng = np.random.default_rng(3)
    d = R._unit(rng.standard_normal((1000, 3)))
    n = R._unit(rng.standard_normal((1000, 3)))
    n = np.where(((d * n).sum(-1) > 0)[:, None], -n, n)
    refl_p, _, refr, tir = R.dielectric_split(d, n, np.ones(1000, bool), 1.0)
    assert np.abs(refr - d).max() < 1e-7 and not tir.any()
    assert np.abs(refl_p - (1.0 + (d * n).sum(-1)) ** 5).max() < 1e-12
    sc = dict(R.SCENES["glass"], spheres=R.spheres((*R._BALL, R.DIELECTRIC, (1, 1, 1), 1.0)))
    a, b = R.closed_form(sc, G=4), R.closed_form("sky", G=4)
    head_on = (16, 24)                                   # the pixel the sphere's centre projects into
    assert (a["cls"][head_on] % 3 != 0).all() and abs(a["mu"][head_on] - b["mu"][head_on]) < 1e-4
    assert np.abs(a["mu"] - b["mu"]).max() < 0.2


def test_depth_one_is_black_on_the_sphere():
    tr = truth("lambert-depth1")
    on = tr["smooth"] & tr["on"]
    assert on.sum() >= 50 and (tr["mu"][on] == 0).all() and (tr["var"][on] == 0).all() and (tr["rgb"][on] == 0).all()
    off = tr["smooth"] & ~tr["on"]
    assert np.array_equal(tr["mu"][off], truth("lambert")["mu"][off])


@pytest.mark.parametrize("name", R.CLOSED_FORM)
def test_smooth_pixels_are_most_of_the_image(name):
    tr = truth(name)
    sm = tr["smooth"]
    assert sm.mean() >= 0.75, sm.mean()
    assert (sm & ~tr["on"]).sum() >= 50
    if len(R.SCENES[name]["spheres"]):
        assert (sm & tr["on"]).sum() >= 50, (sm & tr["on"]).sum()
    # the sky's blue channel is exactly 1: a cross-check of the classification
    assert np.abs(tr["rgb"][sm & ~tr["on"], 2] - 1.0).max() < 1e-12


def test_grid_error_is_far_below_the_standard_error():
    """The truth's own error, estimated as the difference between grids G and 2 G on the smooth pixels, against the standard
    error at the largest sample count any test uses (2^20): se >= 10 x the difference."""
    for name in ("lambert", "glass"):
        a, b = R.closed_form(name, G=16, rows=(8, 24)), R.closed_form(name, G=32, rows=(8, 24))
        sm = R.smooth_mask(R.closed_form(name, G=16)["cls"])[8:24]
        se = np.sqrt(b["var"][sm] / 2 ** 20 + R.rounding_var(b["mu"][sm], 1024, 1024))
        ratio = np.abs(a["mu"] - b["mu"])[sm] / se
        print(f"{name}: max |mu_16 - mu_32| / se(2^20) = {ratio.max():.4f}, max |var_16 / var_32 - 1| = "
              f"{np.abs(a['var'][sm] / b['var'][sm] - 1).max():.5f}")
        assert ratio.max() <= 0.1
        assert np.abs(a["var"][sm] / b["var"][sm] - 1).max() < 0.01


# ------------------------------------------------------------------ integrator (c) against closed forms (b) and fixtures

@pytest.mark.parametrize("name", R.CLOSED_FORM)
def test_monte_carlo_agrees_with_the_closed_form(name):
    tr = truth(name)
    mc = R.monte_carlo(name, 512, 1234)
    R.check(R.statistics(mc["rgb"], dict(tr, ref_var=np.zeros_like(tr["mu"])), 1.0 / 512, tr["smooth"]), label=f"mc {name}")
    # the variances too: the ratio of the summed estimates, within 6 standard deviations of a sum of sample variances
    # (each sample variance's own variance bounded through its range: samples lie in [0, 1])
    sm = tr["smooth"] & (tr["var"] > 0)
    ratio = mc["var"][sm].sum() / tr["var"][sm].sum()
    assert abs(ratio - 1.0) <= 6.0 * np.sqrt((tr["var"][sm] * 1.0 / 512).sum()) / tr["var"][sm].sum() + 0.01, ratio


def test_a_fixture_regenerates():
    """tests/golden/make_radiometry.py's result for one scene, again at a reduced sample count and another seed."""
    fx = fixture("fuzzy")
    assert fx["mu"].shape == (H, W) and fx["mu"].dtype == np.float64 and fx["n"] >= 8192
    mc = R.monte_carlo("fuzzy", 512, 99)
    R.check(R.statistics(mc["rgb"], R.truth("fuzzy", fx), 1.0 / 512), label="fixture fuzzy")


def test_fixtures_are_small():
    total = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.startswith("radiometry_"))
    assert total < 600_000, total


# ------------------------------------------------------------------ the oracle against the truth

@pytest.mark.parametrize("rng_mode", [STREAM, COUNTER])
@pytest.mark.parametrize("name", R.CLOSED_FORM + tuple(n for n in R.FIXTURES if n not in R.CLOSED_FORM))
def test_oracle_converges_to_the_truth(oracle, name, rng_mode):
    tr = truth(name)
    for i, (frames, spp) in enumerate(SPLITS[rng_mode]):
        fb = oracle_render(oracle, name, 100 + 7 * i + rng_mode, frames, spp, rng_mode)
        stream = rng_mode == STREAM
        allowance = R.xor_shuffle_allowance(spp, frames) if stream else 0.0
        extra = R.rounding_var(tr["mu"], frames, spp)
        label = f"oracle {name} {'stream' if stream else 'counter'} {frames}x{spp}"
        if name in R.CLOSED_FORM:                        # the closed form where it holds, the integrator on the edges
            R.check(R.statistics(fb, tr, 1.0 / (frames * spp), tr["smooth"], extra), variance=not (stream and spp < 64 and frames > 1),
                    allowance=allowance, label=label + " [smooth]")
        R.check(R.statistics(fb, tr, 1.0 / (frames * spp), None, extra), variance=not (stream and spp < 64 and frames > 1),
                allowance=allowance, label=label + " [all]")


@pytest.mark.parametrize("rng_mode", [STREAM, COUNTER])
def test_oracle_frames_are_independent(oracle, rng_mode):
    """max_framebuffer_weight = 0: the framebuffer IS frame k's mean.  Stream mode: the XOR shuffle correlates whole frame
    pairs with one sign per pair (radiometry_ref.xor_shuffle_allowance); only "zero on average" is asserted there."""
    tr = truth("glass")
    sc = R.SCENES["glass"]
    packed = oracle.pack_world(to_oracle_spheres(oracle, sc["spheres"]))
    seeds = oracle.fill_seeds(21, W, H)
    for spp in (1, 4, 64):
        zs = []
        for k in range(96):
            fb = oracle.render_frame(W, H, spp, sc["depth"], packed, oracle.pinhole_camera(), seeds, oracle.frame_shuffle(21, k), 0.0,
                                     rng_mode=rng_mode)
            zs.append(R.statistics(fb, tr, 1.0 / spp, tr["smooth"])["z"])
        R.frame_independence(zs, rng_mode == COUNTER, label=f"oracle glass {'counter' if rng_mode else 'stream'} {spp} spp")
