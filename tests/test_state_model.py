"""Host tests of the context model (tests/state_model.py) and of the sequence generator and runner (tests/state_sequences.py):
the model against the references the suite already trusts, the generator's determinism and coverage over the in-suite cases,
and the runner's power -- eight defective models, one host-logic defect each, must all be caught within the in-suite cases."""
import numpy as np
import pytest

import adaptive_ref
import noise_ref
import state_sequences as SS
from common import oracle_render
from state_model import INVALID_ARG, NO_SCENE, STATE, Model, Refused


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _model(mrt, oracle, w, h, spp, depth, max_w, seed, cls=Model):
    return cls(oracle, mrt._lib.load(), mrt.Args(w, h, spp, depth, max_w), seed)


# ------------------------------------------------------------------ the model against the existing references

@pytest.mark.parametrize("max_w", [1.0, 0.75])
@pytest.mark.parametrize("rng_mode", [0, 1])
def test_whole_frames_are_the_oracles_progressive_render(mrt, oracle, max_w, rng_mode):
    spheres, cam = mrt.scene_cover(1, True)
    w, h, spp, depth, seed = 48, 27, 3, 8, 11                         # (tests/test_gpu_adaptive.py's case)
    m = _model(mrt, oracle, w, h, spp, depth, max_w, seed)
    m.set_world(spheres)
    m.set_camera(cam)
    m.set_rng_mode(rng_mode)
    m.redraw()
    m.render(4)
    cnt = oracle.Counters()
    ref = oracle_render(oracle, spheres, cam, w, h, spp, depth, seed, frames=5, max_w=max_w, counters=cnt, rng_mode=rng_mode)
    assert np.array_equal(_bits(m.read_framebuffer()), _bits(ref))
    assert m.frames_done == 5
    assert m.read_counters() == {"samples": cnt.samples, "world_hit_calls": cnt.world_hit_calls, "rng_draws": cnt.rng_draws}


def test_every_tile_before_divergence_is_a_whole_frame_and_tiles_as_rectangles_count_alike(mrt, oracle):
    spheres, cam = mrt.scene_cover(1, False)
    a = _model(mrt, oracle, 43, 21, 2, 5, 1.0, 4)
    b = _model(mrt, oracle, 43, 21, 2, 5, 1.0, 4)
    for m in (a, b):
        m.set_world(spheres)
        m.set_camera(cam)
    a.render_tiles(np.arange(a.n_tiles)[::-1], 3)
    b.render(3)
    assert not a.acc.diverged and np.array_equal(_bits(a.read_framebuffer()), _bits(b.read_framebuffer()))
    assert a.read_counters() == b.read_counters() and (a.tile_frames() == 3).all()
    # two complementary lists make one whole frame's image and counts (a pixel's samples do not depend on the rectangle)
    half = np.arange(a.n_tiles)[::2]
    a.render_tiles(half, 1)
    a.override = tuple(oracle.frame_shuffle(4, 3))                    # (the same frame number's shuffle for the other half)
    a.render_tiles(np.setdiff1d(np.arange(a.n_tiles), half), 1)
    b.render(1)
    assert a.acc.diverged and np.array_equal(_bits(a.read_framebuffer()), _bits(b.read_framebuffer()))
    assert a.read_counters() == b.read_counters()


def test_reports_are_noise_refs_in_the_uniform_case_and_on_a_shard(mrt, oracle):
    spheres = mrt.scene_default()
    m = _model(mrt, oracle, 29, 19, 2, 5, 0.75, 6)
    m.set_noise_tracking(True)
    m.set_world(spheres)
    means = []
    for k in range(4):
        means.append(oracle.render_frame(29, 19, 2, 5, m.packed, m.cam_raw, m.seeds, oracle.frame_shuffle(6, k), 0.0))
        m.redraw()
    fb, S, K = noise_ref.accumulate(means, [adaptive_ref.frame_weight(k, 0.75) for k in range(4)])
    assert np.array_equal(_bits(m.read_noise()), _bits(S)) and np.array_equal(_bits(m.read_framebuffer()), _bits(fb))
    m.noise_query(0.1, 0.05)
    rep = m.noise_result()
    want = noise_ref.report(S, fb, K, 0.1, 0.05)
    assert all(rep[k] == want[k] for k in want) and rep["seq"] == 1 and rep["frames_done"] == 4
    assert np.array_equal(_bits(m.read_noise_tiles()), _bits(noise_ref.tiles(S, fb, K, 0.1, 0.05)))
    # the shards' reports add up to the image's, their rows are the image's rows
    m.reset()
    pixels = above = 0
    for rank in range(3):
        m.reset()
        m.set_shard(rank, 3)
        m.render(4)
        g = noise_ref.shard_rows(19, rank, 3)
        assert np.array_equal(_bits(m.read_framebuffer()[g >= 0]), _bits(fb[g[g >= 0]]))
        assert not m.read_framebuffer()[g < 0].any()
        m.noise_query(0.1, 0.05)
        r = m.noise_result()
        pixels, above = pixels + r["pixels"], above + r["above"]
        assert m.read_noise_tiles().shape == m.tile_frames().shape == (1, 4)
    assert (pixels, above) == (want["pixels"], want["above"])


def test_statuses_follow_the_header(mrt, oracle):
    m = _model(mrt, oracle, 20, 12, 1, 3, 1.0, 1)

    def status(f, *a, **kw):
        try:
            f(*a, **kw)
            return 0
        except Refused as e:
            return e.status

    assert status(m.redraw) == status(m.render_tiles, [0]) == NO_SCENE
    assert status(m.render_tiles, []) == 0 and status(m.render, 0) == 0
    assert status(m.noise_query) == status(m.read_noise) == status(m.render_adaptive) == status(m.read_denoised) == STATE
    assert status(m.acquire_presented) == status(m.release_presented) == STATE
    m.set_world(mrt.scene_default())
    m.set_noise_tracking(True)
    assert status(m.read_noise_tiles) == STATE
    m.render(2)
    assert status(m.set_noise_tracking, False) == status(m.set_shard, 0, 2) == STATE
    assert status(m.render_tiles, [6]) == status(m.render_tiles, [1, 1]) == INVALID_ARG
    assert status(m.render_adaptive, 1, 1) == STATE                   # not queued
    for _ in range(9):
        m.noise_query()
    assert status(m.render_adaptive, 1, 1) == STATE                   # older than the ring of eight
    assert status(m.read_denoised) == 0
    m.render_tiles([0, 1])
    assert status(m.read_denoised) == status(m.present, "rgba8", True, denoise=True) == STATE
    m.set_rng_mode(1)
    m.set_samples_per_frame(65)
    assert status(m.render_tiles, [0]) == INVALID_ARG
    m.reset()
    assert m.noise_result() is None and status(m.read_noise_tiles) == STATE
    m.set_shard(1, 2)
    m.set_samples_per_frame(1)
    assert status(m.render_tiles, [0]) == STATE and status(m.present, "rgba8", True) == INVALID_ARG
    assert status(m.present, "bgra8", False) == 0


def test_present_numbering_fifo_and_drops(mrt, oracle):
    m = _model(mrt, oracle, 20, 12, 1, 3, 1.0, 1)
    m.set_world(mrt.scene_default())
    for _ in range(3):
        m.redraw()
        m.present("rgba8", True)
    img, info = m.acquire_presented(newest=False)
    assert (info["seq"], info["frames_done"], info["dropped"]) == (1, 1, 0)
    img, info = m.acquire_presented(newest=True)
    assert (info["seq"], info["frames_done"], info["dropped"]) == (3, 3, 1)
    assert m.acquire_presented() is None
    m.present("bgra8", False)
    m.reset()                                                         # discards the queued image, keeps the numbering
    assert m.acquire_presented() is None
    m.present("bgra8", False)
    assert m.acquire_presented()[1]["seq"] == 5


# ------------------------------------------------------------------ the generator: determinism and coverage

def test_the_boundary_scene_sizes_are_the_last_small_and_the_first_large_layout(mrt):
    """world.cpp takes the large-scene layout when the hierarchy's n_members > 1024."""
    from test_hierarchy_host import build
    for seed in (0, 1):
        assert build(mrt, SS.make_scene(SS.SMALL_MAX, seed))["n_members"] <= 1024
        assert build(mrt, SS.make_scene(SS.SMALL_MAX + 1, seed))["n_members"] > 1024
    assert SS.SMALL_MAX in SS.SPHERE_COUNTS and SS.SMALL_MAX + 1 in SS.SPHERE_COUNTS


def test_a_case_number_reproduces_its_sequence():
    for case in (0, 5, 12345):
        assert SS.sequence(case) == SS.sequence(case)
    assert SS.sequence(3) != SS.sequence(4)


@pytest.fixture(scope="module")
def suite_runs(oracle):
    """Every in-suite case run once on the model: (ops, per-op statuses, the model's state flags before every op)."""
    out = {}
    for case in SS.SUITE_CASES:
        p, ops = SS.sequence(case)
        m = SS.new_model(oracle, p)
        trace = []
        for op in ops:
            before = dict(diverged=m.acc.diverged, frames=m.frames_done, n=None if m.spheres is None else len(m.spheres), mode=m.rng_mode,
                          spp=m.spp, world=m.world, tracking=m.tracking, override=m.override is not None)
            st, _ = SS.apply(m, op)
            trace.append((op, st, before))
        out[case] = (p, trace)
    return out


def test_the_in_suite_cases_cover_the_vocabulary(suite_runs):
    count, refusals = dict.fromkeys(SS.VOCABULARY, 0), set()
    modes, crossings, spps, hints, shapes, shards = set(), set(), set(), set(), set(), set()
    reset_after_divergence_then_scene = batches_over_32 = override_into_batch = fifo = newest = ring_overrun = 0
    for case, (p, trace) in suite_runs.items():
        shapes.add("one tile wide" if p["width"] <= 8 else "one row high" if p["height"] == 1 else "ragged")
        assert p["width"] % 8 and (p["height"] % 8 or p["height"] == 1)
        since_reset_of_diverged = None
        queries_unread = 0
        for op, st, b in trace:
            count[op[0]] += 1
            if st:
                refusals.add((op[0], st, "no scene" if b["n"] is None else "shard" if b["world"] > 1 else "diverged" if b["diverged"] else ""))
                continue
            if op[0] in ("redraw", "render", "render_tiles", "render_adaptive"):
                modes.add(b["mode"])
                spps.add((b["mode"], b["spp"]))
            if op[0] == "render" and op[1] > 32:
                batches_over_32 += 1
            if op[0] == "render" and op[1] >= 2 and b["override"]:
                override_into_batch += 1
            if op[0] == "set_world" and b["n"] is not None and b["frames"] > 0:
                if b["n"] <= SS.SMALL_MAX < op[1]:
                    crossings.add("small to large")
                if op[1] <= SS.SMALL_MAX < b["n"]:
                    crossings.add("large to small")
            if op[0] == "reset":
                since_reset_of_diverged = 0 if b["diverged"] else None
            elif since_reset_of_diverged is not None:
                if op[0] == "set_world":
                    reset_after_divergence_then_scene += 1
                    since_reset_of_diverged = None
            if op[0] == "set_schedule_hint":
                hints.add(op[1:])
            if op[0] == "set_shard":
                shards.add(op[2])
            if op[0] == "acquire_presented":
                fifo, newest = fifo + (not op[1]), newest + bool(op[1])
            if op[0] == "noise_query":
                queries_unread += 1
                ring_overrun += queries_unread == 9
            elif op[0] == "noise_result":
                queries_unread = 0
    missing = [k for k, v in count.items() if v == 0]
    assert not missing, missing
    assert modes == {0, 1} and crossings == {"small to large", "large to small"}, (modes, crossings)
    assert reset_after_divergence_then_scene >= 1 and batches_over_32 >= 2 and override_into_batch >= 2
    assert fifo >= 2 and newest >= 2 and ring_overrun >= 1
    assert shapes == {"one tile wide", "one row high", "ragged"}
    assert {0, 1, 2, 3, 5} <= {s for _, s in spps} and {(1, 64), (1, 65), (1, 130)} <= spps, spps
    assert (0, 0) in hints and len(hints) >= 6 and len(shards - {1}) >= 3, (hints, shards)
    plain = {(a, st) for a, st, _ in refusals}
    for want in (("set_noise_tracking", STATE), ("set_shard", STATE), ("render_adaptive", STATE), ("render_tiles", INVALID_ARG),
                 ("release_presented", STATE), ("read_noise", STATE), ("acquire_presented", STATE)):
        assert want in plain, want
    for want in (("read_denoised", STATE, "diverged"), ("present", STATE, "diverged"), ("render_tiles", STATE, "shard"),
                 ("read_denoised", STATE, "shard")):
        assert want in refusals, want
    assert any(s == NO_SCENE for _, s, _ in refusals)
    # a report older than the ring, and the counter mode's refusal of more than MRT_COUNTER_BLOCK samples by tiles
    old = counter = 0
    for case, (p, trace) in suite_runs.items():
        seq = 0
        for op, st, b in trace:
            seq += op[0] == "noise_query" and st == 0
            old += op[0] == "render_adaptive" and st == STATE and 1 <= op[2] <= seq - 8
            counter += op[0] == "render_tiles" and st == INVALID_ARG and b["mode"] == 1 and b["spp"] > 64
    assert old >= 1 and counter >= 1, (old, counter)


# ------------------------------------------------------------------ the runner detects defects of a model

class SceneOneFrameEarly(Model):
    """An upload that overtakes a frame in flight: the last frame before a set_world is rendered with the new scene."""
    def _frame(self, tiles=None, batched=False):
        self._undo = (self.acc.fb.copy(), self.acc.S.copy(), self.acc.n.copy(), self.acc.frames_done, self.acc.diverged, dict(self.counters),
                      self.override, tiles)
        super()._frame(tiles, batched)

    def set_world(self, spheres):
        super().set_world(spheres)
        u = getattr(self, "_undo", None)
        if u is not None and self.acc.frames_done == u[3] + 1:
            a = self.acc
            a.fb, a.S, a.n, a.frames_done, a.diverged, self.counters, self.override = u[0], u[1], u[2], u[3], u[4], u[5], u[6]
            super()._frame(u[7])
        self._undo = None


class CameraOneFrameLate(Model):
    def set_camera(self, cam):
        self._late = cam

    def _after_frame(self):
        if getattr(self, "_late", None) is not None:
            super().set_camera(self._late)
            self._late = None

    def _guides_key(self):                  # (the guides are not what this defect is about)
        if getattr(self, "_late", None) is not None:
            super().set_camera(self._late)
            self._late = None
        return super()._guides_key()


class GuidesNotRebuiltAfterSetCamera(Model):
    def set_camera(self, cam):
        stale = getattr(self, "_guide_cam", None) or (self.cam_raw, self.cam_key)
        super().set_camera(cam)
        self._guide_cam = stale

    def set_world(self, spheres):
        super().set_world(spheres)
        self._guide_cam = None

    def _guides(self):
        if getattr(self, "_guide_cam", None) is None:
            return super()._guides()
        now = (self.cam_raw, self.cam_key)
        self.cam_raw, self.cam_key = self._guide_cam
        try:
            return super()._guides()
        finally:
            self.cam_raw, self.cam_key = now


class ResetKeepsTileFrames(Model):
    def _reset_accum(self):
        n = self.acc.n.copy()
        super()._reset_accum()
        self.acc.n[:] = n


class ResetKeepsS(Model):
    def _reset_accum(self):
        S = self.acc.S.copy()
        super()._reset_accum()
        self.acc.S[:] = S


class ResetLeavesOneFramebuffer(Model):
    """Of the two ping-pong buffers only one is zeroed: after an odd number of frames the read-back shows the old accumulation."""
    def _reset_accum(self):
        fb, odd = self.acc.fb.copy(), self.acc.frames_done % 2 == 1
        super()._reset_accum()
        if odd:
            self.acc.fb[:] = fb


class BatchIgnoresOverriddenShuffle(Model):
    def _take_shuffle(self, batched):
        if batched:
            self.override = None
        return super()._take_shuffle(batched)


class UnlistedTilesUpdateS(Model):
    def _blend(self, mean, tiles):
        a = self.acc
        if tiles is not None and len(tiles) < a.n_tiles:
            S = a.S.copy()
            for t in np.setdiff1d(np.arange(a.n_tiles), tiles):
                m = a.tile == t
                S[m] = noise_ref.s_update(a.S[m], mean[m], a.fb[m], adaptive_ref.frame_weight(int(a.n[t]), a.max_w))
            super()._blend(mean, tiles)
            listed = np.isin(a.tile, tiles)
            a.S[~listed] = S[~listed]
        else:
            super()._blend(mean, tiles)


DEFECTS = [SceneOneFrameEarly, CameraOneFrameLate, GuidesNotRebuiltAfterSetCamera, ResetKeepsTileFrames, ResetKeepsS,
           ResetLeavesOneFramebuffer, BatchIgnoresOverriddenShuffle, UnlistedTilesUpdateS]


def test_the_correct_model_passes_its_own_runner(oracle):
    stats = {}
    for case in SS.SUITE_CASES:
        p, _ = SS.sequence(case)
        SS.run(case, SS.new_model(oracle, p), SS.new_model(oracle, p), stats)
    assert stats["ops"] > 400 and stats["frames"] > 200, stats


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda c: c.__name__)
def test_the_runner_catches_a_defective_model(oracle, defect):
    caught = []
    for case in SS.SUITE_CASES:
        p, _ = SS.sequence(case)
        try:
            SS.run(case, SS.new_model(oracle, p, defect), SS.new_model(oracle, p))
        except SS.SequenceMismatch as e:
            msg = str(e)
            assert msg.startswith(f"case {case}, op ") and "ops so far" in msg
            caught.append(msg.split(":")[0])
    print(f"{defect.__name__}: caught in {len(caught)} of {len(SS.SUITE_CASES)} cases: {caught}")
    assert len(caught) >= 2, caught                 # (room to spare: no defect hangs on a single case)
