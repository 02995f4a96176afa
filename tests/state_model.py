"""A host model of one context (include/myraytracer_amd.h): what a sequence of calls on one `myraytracer_amd.State` must return,
composed from the oracle's frames and the float32 restatements -- adaptive_ref (blend, S, n_t, reports after divergence),
noise_ref (reports, tile maps, shard packing), denoise_ref (guides, filter) and present_ref (the 8-bit encode).  No arithmetic of
its own.  `Model` has State's method names for the vocabulary of tests/state_sequences.py; a call the header refuses raises
`Refused(status)`.  The model is synchronous: every call sees the frames before it finished, which is what the header promises
of the library whatever it keeps in flight.

What the model holds is what the header says a context holds: scene, camera, seed texture, samples per frame, RNG mode, the
shuffle override, frames_done (in the Accum), max weight, tracking, shard, the Accum, the counters, the report ring's and the
present ring's numbering."""
import math
from types import SimpleNamespace

import numpy as np

import adaptive_ref
import denoise_ref
import noise_ref
from common import to_oracle_camera, to_oracle_spheres
from present_ref import encode_host

OK, INVALID_ARG, NO_SCENE, STATE = 0, 1, 4, 7
COUNTER_BLOCK = 64
NOISE_RING = 8
COUNTER_KEYS = ("samples", "world_hit_calls", "rng_draws")
PRESENT_FORMATS = {"rgba8": 1, "bgra8": 2}
FLIP_Y, DENOISED = 1, 8


class Refused(Exception):
    def __init__(self, status, where):
        super().__init__(f"{where}: status {status}")
        self.status = status


# Oracle frames and guides are pure functions of their inputs; one cache serves the model and, in the host tests, the defective
# models run against it (they differ in which inputs they pass, not in what a frame of given inputs is).
_FRAMES, _GUIDES = {}, {}
CACHE_LIMIT = 6000


def _key(a) -> int:
    return hash(np.ascontiguousarray(a).tobytes())


class Model:
    def __init__(self, O, L, args, seed: int):
        """O: oracle.pyoracle; L: the loaded library, for the host-only mrt_srgb8 of present_ref; args: width, height,
        samples_per_frame, ray_depth, max_framebuffer_weight (resolved)."""
        self.O, self.L, self.seed = O, L, seed
        self.w, self.h, self.depth, self.max_w = args.width, args.height, args.ray_depth, args.max_framebuffer_weight
        self.spp, self.rng_mode = args.samples_per_frame, 0
        self.spheres = self.packed = self.scene_key = None
        self._set_cam(None)
        self._fill_seeds()
        self.override = None                       # mrt_set_rng_shuffle since the last frame
        self.acc = adaptive_ref.Accum(self.h, self.w, self.max_w)
        self.tracking = False
        self.rank, self.world = 0, 1
        self.counters = dict.fromkeys(COUNTER_KEYS, 0)
        self.noise_seq, self.noise_first, self.reports = 0, 1, {}
        self.present_seq, self.queue, self.held, self.dropped = 0, [], False, 0
        self.frames_total = 0                      # (a statistic of the runner's, not state)

    # ---- pieces the defective models of tests/test_state_model.py override
    def _frame_scene(self):
        return self.packed, self.scene_key

    def _frame_camera(self):
        return self.cam_raw, self.cam_key

    def _take_shuffle(self, batched: bool):
        s = self.override if self.override is not None else self.O.frame_shuffle(self.seed, self.acc.frames_done)
        self.override = None
        return tuple(int(x) for x in s)

    def _blend(self, mean, tiles):
        self.acc.frame(mean, tiles)

    def _reset_accum(self):
        self.acc.reset()

    def _guides_key(self):
        return (self.scene_key, self.cam_key, self.w, self.h)

    def _after_frame(self):
        pass

    # ---- helpers
    def _set_cam(self, cam):
        self.cam = to_oracle_camera(self.O, cam)
        self.cam_raw = self.O.camera_derive(self.cam)
        self.cam_key = hash(bytes(self.cam_raw))

    def _fill_seeds(self):
        self.seeds = self.O.fill_seeds(self.seed, self.w, self.h)
        self.seeds_key = _key(self.seeds)

    @property
    def n_tiles(self):
        return self.acc.n_tiles

    def _rects(self, tiles):
        """The rectangles one frame renders: the image, a shard's bands, or the listed tiles."""
        if tiles is not None:
            tx = self.acc.tx
            return [((t % tx) * 8, min((t % tx) * 8 + 8, self.w), (t // tx) * 8, min((t // tx) * 8 + 8, self.h)) for t in tiles]
        if self.world == 1:
            return [(0, self.w, 0, self.h)]
        bands = -(-self.h // 8)
        return [(0, self.w, b * 8, min(b * 8 + 8, self.h)) for b in range(self.rank, bands, self.world)]

    def _render(self, shuffle, rect):
        packed, scene_key = self._frame_scene()
        cam_raw, cam_key = self._frame_camera()
        k = (scene_key, cam_key, self.seeds_key, self.w, self.h, self.spp, self.depth, self.rng_mode, shuffle, rect)
        if k not in _FRAMES:
            if len(_FRAMES) > CACHE_LIMIT:
                _FRAMES.clear()
            cnt = self.O.Counters()
            x0, x1, y0, y1 = rect
            img = self.O.render_frame(self.w, self.h, self.spp, self.depth, packed, cam_raw, self.seeds, shuffle, 0.0,
                                      rows=(y0, y1), cols=(x0, x1), counters=cnt, rng_mode=self.rng_mode)
            _FRAMES[k] = (img[y0:y1, x0:x1].copy(), tuple(int(getattr(cnt, c)) for c in COUNTER_KEYS))
        return _FRAMES[k]

    def _frame(self, tiles=None, batched=False):
        shuffle = self._take_shuffle(batched)
        mean = np.zeros((self.h, self.w, 4), np.float32)
        for rect in self._rects(tiles):
            img, cnt = self._render(shuffle, rect)
            x0, x1, y0, y1 = rect
            mean[y0:y1, x0:x1] = img
            for c, v in zip(COUNTER_KEYS, cnt):
                self.counters[c] += v
        self._blend(mean, tiles)
        self.frames_total += 1
        self._after_frame()

    def _packed(self, a):
        return a.copy() if self.world == 1 else noise_ref.pack_rows(a, self.rank, self.world)

    def _K(self):
        return adaptive_ref.k_table(self.acc.frames_done, self.max_w)[-1]

    def _oldest(self):
        return max(self.noise_first, self.noise_seq - NOISE_RING + 1 if self.noise_seq >= NOISE_RING else 1)

    def _denoise_check(self, where, tracking=True):
        if tracking and not self.tracking:
            raise Refused(STATE, where)
        if self.world != 1:
            raise Refused(STATE, where)
        if self.packed is None:
            raise Refused(NO_SCENE, where)
        if self.acc.diverged:
            raise Refused(STATE, where)

    def _guides(self):
        k = self._guides_key()
        if k not in _GUIDES:
            if len(_GUIDES) > 64:
                _GUIDES.clear()
            rays = denoise_ref.centre_rays(self.w, self.h, self.cam_raw)
            hit, t, normal, albedo = denoise_ref.expected_guides(self.O, self.spheres, rays)
            _GUIDES[k] = {"rays": rays, "index": hit.reshape(self.h, self.w).astype(np.int32), "t": t.reshape(self.h, self.w),
                          "normal": normal.reshape(self.h, self.w, 3), "albedo": albedo.reshape(self.h, self.w, 3)}
        return _GUIDES[k]

    def _denoised(self):
        return denoise_ref.denoise(self.acc.fb, self.acc.S, self._K(), self._guides())

    def _discard_presents(self):
        self.queue, self.held, self.dropped = [], False, 0

    # ---- scene
    def set_world(self, spheres):
        self.spheres = np.array(spheres, copy=True)
        self.packed = self.O.pack_world(to_oracle_spheres(self.O, self.spheres))
        self.scene_key = (_key(self.spheres), len(self.spheres))

    def set_camera(self, cam):
        self._set_cam(cam)

    def set_seeds(self, seeds):
        self.seeds = np.ascontiguousarray(seeds, np.uint32).reshape(self.h, self.w, 4).copy()
        self.seeds_key = _key(self.seeds)

    def read_seeds(self):
        return noise_ref.pack_rows(self.seeds, self.rank, self.world)       # (always the packed rows, padding included)

    def set_shard(self, rank, world):
        if world == 0 or rank >= world:
            raise Refused(INVALID_ARG, "set_shard")
        if self.acc.frames_done != 0:
            raise Refused(STATE, "set_shard")
        self._discard_presents()
        self.rank, self.world = rank, world
        self._fill_seeds()                          # the seed texture is derived again from the creation seed
        self._reset_accum()
        if self.tracking:
            self.noise_first = self.noise_seq + 1

    def shard_info(self):
        return self.rank, self.world, len(noise_ref.shard_rows(self.h, self.rank, self.world)), self.w

    # ---- frame loop
    def redraw(self):
        self.render(1)

    def render(self, frames=1):
        for i in range(frames):
            if self.packed is None:
                raise Refused(NO_SCENE, "render")
            self._frame(None, batched=frames >= 2)

    def render_tiles(self, tiles, frames=1):
        tiles = [int(t) for t in np.asarray(tiles).ravel()]
        if not tiles or frames == 0:
            return
        if self.world != 1:
            raise Refused(STATE, "render_tiles")
        if self.packed is None:
            raise Refused(NO_SCENE, "render_tiles")
        if self.rng_mode == 1 and self.spp > COUNTER_BLOCK:
            raise Refused(INVALID_ARG, "render_tiles")
        if len(tiles) > self.n_tiles or max(tiles) >= self.n_tiles or len(set(tiles)) != len(tiles):
            raise Refused(INVALID_ARG, "render_tiles")
        if len(tiles) == self.n_tiles:
            return self.render(frames)
        for _ in range(frames):
            self._frame(tiles, batched=frames >= 2)

    def render_adaptive(self, frames=1, report_seq=0):
        if not self.tracking:
            raise Refused(STATE, "render_adaptive")
        if report_seq == 0:
            seq = self.noise_seq if self.noise_seq >= self._oldest() else 0
        else:
            if report_seq > self.noise_seq or report_seq < self._oldest():
                raise Refused(STATE, "render_adaptive")
            seq = report_seq
        if seq == 0:
            sel = np.arange(len(noise_ref.shard_rows(self.h, self.rank, self.world)) // 8 * self.acc.tx, dtype=np.uint32)
        else:
            sel = adaptive_ref.select(self.reports[seq]["map"], self.reports[seq]["report"]["threshold"])
        if len(sel):
            self.render_tiles(sel, frames)
        return seq, len(sel)

    def sync(self):
        pass

    def reset(self):
        self._discard_presents()
        self._reset_accum()
        self.noise_first = self.noise_seq + 1
        self.counters = dict.fromkeys(COUNTER_KEYS, 0)
        self.override = None

    @property
    def locals(self):
        n = self.acc.frames_done
        shuffle = self.override if self.override is not None else self.O.frame_shuffle(self.seed, n)
        return SimpleNamespace(shape=(self.w, self.h), samples_per_frame=self.spp, ray_depth=self.depth,
                               rng_shuffle=tuple(int(x) for x in shuffle),
                               framebuffer_weight=float(adaptive_ref.frame_weight(n, self.max_w)), rng_mode=self.rng_mode)

    def set_rng_shuffle(self, shuffle):
        self.override = tuple(int(x) for x in shuffle)

    def set_rng_mode(self, mode):
        if mode > 1:
            raise Refused(INVALID_ARG, "set_rng_mode")
        self.rng_mode = mode

    def set_samples_per_frame(self, spp):
        self.spp = spp

    @property
    def frames_done(self):
        return self.acc.frames_done

    # ---- scheduling: the images are the same whatever the schedule
    def set_schedule_hint(self, div, mult=1):
        if (div, mult) != (0, 0) and not (1 <= div <= 8 and 1 <= mult <= 8 and max(2, div) * mult <= 16):
            raise Refused(INVALID_ARG, "set_schedule_hint")

    def debug_set_frames_in_flight(self, slots):
        pass

    def debug_set_frame_batching(self, enabled):
        pass

    # ---- output
    def read_framebuffer(self):
        return self._packed(self.acc.fb)

    def read_counters(self):
        return dict(self.counters)

    def tile_frames(self):
        if self.world == 1:
            return self.acc.tile_frames()
        return np.full((len(noise_ref.shard_rows(self.h, self.rank, self.world)) // 8, self.acc.tx), self.acc.frames_done, np.uint32)

    # ---- noise estimate
    def set_noise_tracking(self, enabled):
        if self.acc.frames_done != 0:
            raise Refused(STATE, "set_noise_tracking")
        if bool(enabled) == self.tracking:
            return
        self.tracking = bool(enabled)
        self.noise_first = self.noise_seq + 1

    def noise_query(self, threshold=0.02, floor=0.01):
        if not self.tracking:
            raise Refused(STATE, "noise_query")
        if not (math.isfinite(threshold) and math.isfinite(floor) and floor >= 0):
            raise Refused(INVALID_ARG, "noise_query")
        a = self.acc
        if a.diverged:
            rep, tmap = a.report(threshold, floor), a.tiles(threshold, floor)
        elif self.world == 1:
            rep, tmap = a.report(threshold, floor, diverged=False), a.tiles(threshold, floor, diverged=False)
        else:
            valid = noise_ref.shard_rows(self.h, self.rank, self.world) >= 0
            S, fb = self._packed(a.S), self._packed(a.fb)
            rep = noise_ref.report(S[valid], fb[valid], self._K(), threshold, floor)
            tmap = noise_ref.tiles(S, fb, self._K(), threshold, floor, valid=valid)
        self.noise_seq += 1
        rep.update(seq=self.noise_seq, frames_done=a.frames_done, threshold=float(np.float32(threshold)), floor=float(np.float32(floor)))
        self.reports[self.noise_seq] = {"report": rep, "map": tmap}
        self.reports.pop(self.noise_seq - NOISE_RING, None)

    def noise_result(self, wait=True):
        if self.noise_seq < self.noise_first:
            return None
        return dict(self.reports[self.noise_seq]["report"])

    def read_noise(self):
        if not self.tracking:
            raise Refused(STATE, "read_noise")
        return self._packed(self.acc.S)

    def read_noise_tiles(self):
        if not self.tracking or self.noise_seq < self.noise_first:
            raise Refused(STATE, "read_noise_tiles")
        return self.reports[self.noise_seq]["map"].copy()

    # ---- present pass
    def present(self, fmt="rgba8", flip=True, gathered=False, denoise=False):
        assert not gathered
        if denoise:
            self._denoise_check("present")
        elif self.world > 1 and flip:
            raise Refused(INVALID_ARG, "present")
        assert len(self.queue) + self.held <= 2, "the sequence outruns the smallest ring (3 entries): what is dropped is not defined"
        src = self._denoised() if denoise else self._packed(self.acc.fb)
        img = encode_host(self.L, src, fmt, flip)
        self.present_seq += 1
        info = {"seq": self.present_seq, "frames_done": self.acc.frames_done, "width": self.w, "rows": img.shape[0],
                "row_bytes": 4 * self.w, "format": PRESENT_FORMATS[fmt], "flags": (FLIP_Y if flip else 0) | (DENOISED if denoise else 0)}
        self.queue.append((img, info))

    def acquire_presented(self, newest=True, wait=True, copy=True):
        if self.present_seq == 0:
            raise Refused(STATE, "acquire_presented")
        self.held = False
        if not self.queue:
            return None
        if newest:
            self.dropped += len(self.queue) - 1
            img, info = self.queue[-1]
            self.queue = []
        else:
            img, info = self.queue.pop(0)
        info = dict(info, dropped=self.dropped)
        self.dropped, self.held = 0, True
        return img, info

    def release_presented(self):
        if not self.held:
            raise Refused(STATE, "release_presented")
        self.held = False

    # ---- denoiser
    def read_denoised(self):
        self._denoise_check("read_denoised")
        return self._denoised()

    def debug_read_guides(self):
        self._denoise_check("debug_read_guides", tracking=False)
        return {k: v.copy() for k, v in self._guides().items()}
