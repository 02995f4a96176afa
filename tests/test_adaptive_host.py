"""Adaptive sampling's host side (no GPU): the float32 restatement (tests/adaptive_ref.py) against noise_ref's uniform
accumulation when every tile is in every frame, its weights and K(n) against the library's host functions, what a subset frame
does to the listed and the other tiles, the selection, and the new symbols' bindings."""
import math
import os

import numpy as np
import pytest

import adaptive_ref
import noise_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _means(rng, frames, h, w):
    out = []
    for _ in range(frames):
        m = rng.random((h, w, 4), dtype=np.float32) * np.float32(2)
        m[..., 3] = 1
        out.append(m)
    return out


@pytest.mark.parametrize("max_w", [1.0, 0.75])
@pytest.mark.parametrize("shape", [(16, 24), (13, 21)])
def test_every_tile_every_frame_is_the_uniform_accumulation(shape, max_w):
    h, w = shape
    means = _means(np.random.default_rng(3), 7, h, w)
    fb_want, S_want, K_want = noise_ref.accumulate(means, [adaptive_ref.frame_weight(k, max_w) for k in range(7)])
    acc = adaptive_ref.Accum(h, w, max_w)
    for m in means:
        acc.frame(m)
    assert np.array_equal(acc.fb.view(np.uint32), fb_want.view(np.uint32))
    assert np.array_equal(acc.S.view(np.uint32), S_want.view(np.uint32))
    assert (acc.tile_frames() == 7).all()
    kt, kmax = acc.k_per_pixel()
    assert kmax == K_want
    # the per-tile report of a uniform accumulation is the uniform report
    want = noise_ref.report(S_want, fb_want, K_want)
    got = acc.report()
    for k in ("pixels", "above", "non_finite", "max_se"):
        assert got[k] == want[k], k
    assert got["sum_var"] == pytest.approx(want["sum_var"], rel=1e-12)
    assert np.array_equal(acc.tiles(), noise_ref.tiles(S_want, fb_want, K_want))


@pytest.mark.parametrize("max_w", [1.0, 0.9, 0.75, 0.5])
def test_k_table_is_mrt_noise_factor(mrt, max_w):
    L = mrt._lib.load()
    table = adaptive_ref.k_table(3000, max_w)
    for n in list(range(0, 50)) + list(range(50, 3001, 37)):
        got = L.mrt_noise_factor(n, max_w)
        if math.isinf(table[n]):
            assert math.isinf(got), n
        else:
            assert got == table[n], (n, got, table[n])


@pytest.mark.parametrize("max_w", [1.0, 0.75, 0.3])
def test_frame_weight_is_mrt_frame_weight(mrt, max_w):
    L = mrt._lib.load()
    for n in list(range(0, 300)) + [2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 123456789, 0xFFFFFFFE, 0xFFFFFFFF]:
        assert np.float32(L.mrt_frame_weight(n, max_w)) == adaptive_ref.frame_weight(n, max_w), n


def test_a_subset_frame_leaves_other_tiles_and_weighs_each_tile_by_its_own_count():
    h, w, max_w = 24, 32, 1.0
    rng = np.random.default_rng(9)
    means = _means(rng, 6, h, w)
    acc = adaptive_ref.Accum(h, w, max_w)
    acc.frame(means[0])
    acc.frame(means[1])
    fb0, S0 = acc.fb.copy(), acc.S.copy()
    tiles = [1, 4, 5, 11]
    acc.frame(means[2], tiles)
    listed = np.isin(acc.tile, tiles)
    assert np.array_equal(acc.fb[~listed].view(np.uint32), fb0[~listed].view(np.uint32))
    assert np.array_equal(acc.S[~listed].view(np.uint32), S0[~listed].view(np.uint32))
    n = acc.tile_frames().ravel()
    assert (n[tiles] == 3).all() and (np.delete(n, tiles) == 2).all() and acc.frames_done == 3
    # tile 4 has seen frames 0, 1, 2: exactly a uniform accumulation of them
    fb_u, S_u, _ = noise_ref.accumulate(means[:3], [adaptive_ref.frame_weight(k, max_w) for k in range(3)])
    m4 = acc.tile == 4
    assert np.array_equal(acc.fb[m4].view(np.uint32), fb_u[m4].view(np.uint32))
    assert np.array_equal(acc.S[m4].view(np.uint32), S_u[m4].view(np.uint32))
    # a whole frame afterwards: every tile at its own weight
    acc.frame(means[3])
    m0 = acc.tile == 0
    fb_t, S_t, _ = noise_ref.accumulate([means[0], means[1], means[3]], [adaptive_ref.frame_weight(k, max_w) for k in range(3)])
    assert np.array_equal(acc.fb[m0].view(np.uint32), fb_t[m0].view(np.uint32))
    assert np.array_equal(acc.S[m0].view(np.uint32), S_t[m0].view(np.uint32))
    # K per tile: the least-sampled tiles' is the report's
    kt, kmax = acc.k_per_pixel()
    assert kmax == adaptive_ref.k_table(3, max_w)[3] and kt[4] == adaptive_ref.k_table(4, max_w)[4]


def test_selection_is_the_tiles_above_the_threshold():
    h, w = 24, 40
    acc = adaptive_ref.Accum(h, w, 1.0)
    rng = np.random.default_rng(1)
    for m in _means(rng, 4, h, w):
        acc.frame(m)
    tmap = acc.tiles(0.3)
    sel = adaptive_ref.select(tmap, 0.3)
    assert (tmap.ravel()[sel] > np.float32(0.3)).all()
    assert (np.delete(tmap.ravel(), sel) <= np.float32(0.3)).all()
    # the tiles selected are exactly those holding a pixel counted in `above`
    finite, se, L, rel, above = acc.per_pixel(acc.k_per_pixel()[0], 0.3, 0.01)
    assert set(np.unique(acc.tile[above]).tolist()) == set(sel.tolist())
    assert len(adaptive_ref.select(np.zeros((3, 5), np.float32), 0.02)) == 0


def test_adaptive_symbols_are_bound(mrt):
    L = mrt._lib.load()
    header = open(os.path.join(ROOT, "include", "myraytracer_amd.h")).read()
    for name in ("mrt_render_tiles", "mrt_render_adaptive", "mrt_read_tile_frames"):
        assert name in mrt._lib.EXPORTS and name + "(" in header
        assert getattr(L, name).argtypes is not None
    st = mrt.State
    for meth in ("render_tiles", "render_adaptive", "tile_frames"):
        assert callable(getattr(st, meth))
    import inspect
    assert inspect.signature(st.render_until).parameters["adaptive"].default is False


def test_reset_returns_to_the_uniform_state_and_divergence_is_tracked():
    rng = np.random.default_rng(3)
    a = adaptive_ref.Accum(19, 21, 0.75)
    b = adaptive_ref.Accum(19, 21, 0.75)
    means = [rng.random((19, 21, 4)).astype(np.float32) for _ in range(4)]
    a.frame(means[0])
    assert not a.diverged
    a.frame(means[1], np.arange(a.n_tiles))            # every tile: still uniform
    assert not a.diverged
    a.frame(means[2], [0, 4])
    assert a.diverged
    a.reset()
    assert not a.diverged and a.frames_done == 0 and not a.n.any() and not a.fb.any() and not a.S.any()
    for m in means[:2]:
        a.frame(m)
        b.frame(m)
    assert np.array_equal(a.fb.view(np.uint32), b.fb.view(np.uint32)) and np.array_equal(a.S.view(np.uint32), b.S.view(np.uint32))
