// The frame loop: the launch-width controller and the frames in flight, putting a frame on a slot (mrt_redraw / mrt_render,
// and adaptive sampling's subset frames: mrt_render_tiles), and the scheduling diagnostics.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mrt_ctx.h"

using mrt::fail, mrt::local_texels, mrt::create_slot_streams, mrt::fill_scene_params, mrt::alloc_frame_buffers;

namespace mrt {

// the side stream of a frame slot and its three events (those it does not have yet)
int create_slot_streams(mrt_ctx* c, mrt_ctx::FrameSlot& S) {
    if (!S.stream) HIP_TRY(c, hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
    if (!S.render_done) HIP_TRY(c, hipEventCreateWithFlags(&S.render_done, hipEventDisableTiming));
    if (!S.finalize_done) HIP_TRY(c, hipEventCreateWithFlags(&S.finalize_done, hipEventDisableTiming));
    if (!S.stats_ready) HIP_TRY(c, hipEventCreateWithFlags(&S.stats_ready, hipEventDisableTiming));
    return MRT_OK;
}

// adaptive sampling's per-tile state (mrt_render_tiles): back to a uniform accumulation
void free_tile_frames(mrt_ctx* c) {
    free_device(c->d_tile_frames, c->d_k_f32, c->d_k_f64);
    c->k_len = 0;
    c->k_table.clear(); c->k_c2 = 1.0;
    c->tiles_diverged = false;
    c->tile_frames.clear();
}

}  // namespace mrt

// How many of `k` side streams of this process really run at a time: one clock-bounded single-wave kernel per stream (0.5 ms
// each; launch_hold) stamps its start and end on the device's wall clock; the answer is the largest number of them resident at
// one instant.  HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless the host set the variable
// before its first HIP call) and kernels of streams that share one serialise: round 4 measured 8 frames in flight running 2.7
// at a time on the default, all 8 on 16 queues (C5's 1/8 share 1,050 -> 2,370 Msamples/s).  Called once per context, with
// nothing in flight, when the schedule first asks for more than two frames.
static int probe_stream_concurrency(mrt_ctx* c, uint32_t k, float* out) {
    if (k < 2u) k = 2u;
    if (k > mrt_ctx::kMaxFrameSlots) k = mrt_ctx::kMaxFrameSlots;
    for (uint32_t i = 0; i < k; i++) MRT_TRY(create_slot_streams(c, c->slot[i]));
    MRT_TRY(mrt::wait_all(c, "probe_stream_concurrency"));
    unsigned long long* const stamps = c->h_stats + 3 * mrt_ctx::kMaxFrameSlots;      // pinned, device-visible: 2 per stream
    uint32_t best = 0;
    for (int pass = 0; pass < 2; pass++) {           // (the first pass also pays for the code object and the queues' creation)
        std::memset(stamps, 0, 2 * mrt_ctx::kMaxFrameSlots * sizeof(unsigned long long));
        for (uint32_t i = 0; i < k; i++) {
            const int e = mrt::launch_hold(50000ull, 1u << 14, stamps + 2 * i, c->slot[i].stream);
            if (e) return fail(c, MRT_ERR_HIP, "probe_stream_concurrency: launch failed: %s", hipGetErrorString((hipError_t)e));
        }
        for (uint32_t i = 0; i < k; i++) MRT_TRY(mrt::wait_stream(c, c->slot[i].stream, "probe_stream_concurrency"));
        best = 0;
        for (uint32_t i = 0; i < k; i++) {           // at the start of kernel i: how many are resident?
            uint32_t n = 0;
            for (uint32_t j = 0; j < k; j++) n += (stamps[2 * j] <= stamps[2 * i] && stamps[2 * i] < stamps[2 * j + 1]) ? 1u : 0u;
            best = std::max(best, n);
        }
    }
    *out = (float)best;
    return MRT_OK;
}

// The most frames in flight this process can really run side by side: kMaxFrameSlots where the probe says so, else the largest
// power of two it supports (>= 2), with ONE line of warning behind mrt_last_error(NULL).  Asked once per context
// (WidthController::wants_probe, after_probe).
static int probe_max_slots(mrt_ctx* c, uint32_t* max_slots) {
    float conc = 0.0f;
    MRT_TRY(probe_stream_concurrency(c, mrt_ctx::kMaxFrameSlots, &conc));
    // (all sixteen or eight: with 15 of 16 -- what GPU_MAX_HW_QUEUES=16 gives, the context's own stream holds a queue too -- two
    // of the sixteen frames take turns on one queue, and C5's 1/8 share renders 2,790 Msamples/s instead of 3,750, less than
    // with eight frames in flight)
    uint32_t cap = mrt_ctx::kMaxFrameSlots;
    while (cap > 2u && conc < (cap == 8u ? 7.0f : (float)cap)) cap /= 2u;
    *max_slots = cap;
    if (cap < mrt_ctx::kMaxFrameSlots) {
        char buf[256];
        std::snprintf(buf, sizeof buf, "myraytracer_amd: only %.0f of %u side streams run at a time in this process: at most %u frames in flight "
                      "(set GPU_MAX_HW_QUEUES=20 before the process' first HIP call: INTEGRATION.md 2a)", conc, mrt_ctx::kMaxFrameSlots, cap);
        mrt::set_global_error(buf);
        static const bool trace = std::getenv("MRT_TRACE_WIDTH") != nullptr;
        if (trace) std::fprintf(stderr, "%s\n", buf);
    }
    return MRT_OK;
}

static mrt::WidthWorkload width_workload(const mrt_ctx* c, bool counter) {
    mrt::WidthWorkload w;
    w.n_tiles = c->n_tiles; w.n_waves = c->n_waves; w.max_slots = c->width.max_slots;
    w.spp = c->locals.samples_per_frame; w.n_members = c->n_members; w.counter = counter ? 1u : 0u;
    w.n_spheres = c->n_spheres;
    return w;
}

// The device's side of the launch-width controller for the frame about to be launched (adaptive launches only: one frame per
// launch, no diagnostic override): what is still running, the back-pressure, the lane-utilisation samples that have landed, the
// clocks and the probe.  Every rule -- the setting for a new workload, the measurement windows, the trials -- is the
// controller's (c->width: width_policy.h).  *want = frames in flight, *frames_running = earlier frames whose render kernels
// are still queued or running, as the controller sees them.
static int schedule_frame(mrt_ctx* c, bool counter, uint32_t* want, uint32_t* frames_running) {
    static const bool trace = std::getenv("MRT_TRACE_WIDTH") != nullptr;      // diagnostics: every decision, on stderr
    mrt::WidthController& W = c->width;
    const mrt::WidthWorkload w = width_workload(c, counter);
    W.begin_workload(w, c->frame_seq);
    // The host may not run further ahead than the frames in flight: before a slot is used again, its previous frame's
    // render kernel has completed (a swap-chain's back-pressure; the GPU still holds a full set of frames, queued or
    // running).  It bounds the queued work and is what lets the samples below arrive while they can still matter -- a
    // caller that issues its redraws in one burst would otherwise see none of them before its last call.
    // The frames still queued or running beside the slot this frame takes are counted HERE, before that wait: what the caller
    // keeps in flight is what it has issued when it calls.  Counted after the wait the number is taken at the one moment a
    // convoy of frames has just ended -- frames launched together end within a fraction of a millisecond of each other -- and
    // says 0 to 2 of a caller that was a full set of frames ahead; which of the frames' events had landed by then is a race.
    uint32_t running = 0;
    {
        const uint32_t own = (uint32_t)(c->frame_seq % c->frame_slots);
        for (uint32_t i = 0; i < c->frame_slots; i++)
            if (i != own && c->slot[i].render_pending && hipEventQuery(c->slot[i].render_done) != hipSuccess) running++;
        (void)hipGetLastError();        // (hipEventQuery's hipErrorNotReady is not an error)
        mrt_ctx::FrameSlot& Own = c->slot[own];
        if (Own.stats_pending) {
            char what[160];
            std::snprintf(what, sizeof what, "mrt_redraw: back-pressure of slot %u (render kernel of frame %llu, next frame %llu, %u frames in flight)",
                          own, (unsigned long long)Own.stats_seq, (unsigned long long)c->frame_seq, c->frame_slots);
            MRT_TRY(mrt::wait_event(c, Own.stats_ready, what));
        }
    }
    // lane-utilisation samples that have landed (an event that is not ready yet is looked at next time)
    for (uint32_t i = 0; i < c->frame_slots; i++) {
        mrt_ctx::FrameSlot& T = c->slot[i];
        if (T.render_pending && hipEventQuery(T.render_done) == hipSuccess) T.render_pending = false;
        if (!T.stats_pending || hipEventQuery(T.stats_ready) != hipSuccess) continue;
        T.stats_pending = false;
        W.add_sample(T.stats_seq, c->h_stats[3 * i], c->h_stats[3 * i + 2]);
    }
    (void)hipGetLastError();        // (hipEventQuery's hipErrorNotReady is not an error)
    *frames_running = W.note_running(c->frame_seq, running);
    const double now = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    W.open_window(c->frame_seq, now);
    if (W.window_due(c->frame_seq, now)) {
        // start-to-start times of the window's frames, whole frames on the DEVICE's clock: the start events of frame f and of
        // frame f + slots, the next on the same slot (what the controller prefers to the host's count: close_window)
        const uint32_t slots = c->frame_slots;
        double sum_ms = 0.0;
        uint32_t n = 0;
        for (uint64_t f = W.t0_seq; f + slots < c->frame_seq; f++) {
            if (c->frame_seq - f > mrt_ctx::kEventRing) continue;               // (overwritten since)
            hipEvent_t a = c->ev_start[f % mrt_ctx::kEventRing], b = c->ev_start[(f + slots) % mrt_ctx::kEventRing];
            if (hipEventQuery(b) != hipSuccess) break;                          // (not started yet, nor are the later ones)
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, a, b) == hipSuccess && ms > 0.0f) { sum_ms += ms; n++; }
        }
        (void)hipGetLastError();
        const mrt::WidthState tried = W.s;
        const mrt::WidthWindow m = W.close_window(w, c->frame_seq, now, slots, n, sum_ms);
        if (trace) std::fprintf(stderr, "mrt width: frame %llu: div %u x %u, window %llu frames, utilisation %.4f, %.2f frames/s%s\n",
                                (unsigned long long)c->frame_seq, tried.div, tried.mult, (unsigned long long)(c->frame_seq - W.t0_seq),
                                m.util, m.rate, tried.prev_div != 0 ? " (trial)" : "");
        if (trace && W.s.settled) std::fprintf(stderr, "mrt width: settled at div %u x %u\n", W.s.div, W.s.mult);
    }
    // more than two frames in flight only where they really run side by side (measured once, when a setting first asks for them)
    if (W.wants_probe()) {
        uint32_t max_slots = 0;
        MRT_TRY(probe_max_slots(c, &max_slots));
        W.after_probe(max_slots, w, c->frame_seq);
    }
    *want = W.frames_in_flight();
    return MRT_OK;
}

// `want` frame slots in use from the next frame on: a change waits for the frames under way
static int set_frame_slots(mrt_ctx* c, uint32_t want) {
    if (want == c->frame_slots) return MRT_OK;
    MRT_TRY(mrt::wait_all(c, "mrt_redraw: change of the frames in flight"));
    // the further slots' streams and colour sums now, in one go: allocated on first use each would wait for the frames in flight
    // (frame_slots only once every slot below it is complete: if a creation fails, the next redraw comes back here)
    for (uint32_t i = 0; i < want; i++) {
        mrt_ctx::FrameSlot& T = c->slot[i];
        MRT_TRY(create_slot_streams(c, T));
        T.stats_pending = false;
        T.render_pending = false;
        if (T.pix_acc_layers != 0) continue;
        MRT_TRY(mrt::alloc_first_colour_sums(c, T));
    }
    c->frame_slots = want;
    return MRT_OK;
}

// ---- putting a frame on a slot: the steps redraw_frames and render_subset share, each written once ---------------------------

// the kernel arguments that do not depend on the caller: scene, shard, seeds, counters, the slot's tile queue and costs
static void frame_params(const mrt_ctx* c, const mrt_ctx::FrameSlot& S, uint32_t n_tiles, mrt::KParams& p) {
    std::memset(&p, 0, sizeof p);
    p.locals = c->locals;
    fill_scene_params(c, p);
    p.shard_rank = c->shard_rank; p.shard_world = c->shard_world;
    p.seeds = c->d_seeds;
    p.counters = c->d_counters;
    p.count_draws = c->count_draws ? 1u : 0u;
    p.wave_log = nullptr;            // (stamps builds: redraw_frames passes the frame's part of the log ring)
    p.tiles_x = c->tiles_x; p.n_tiles = n_tiles;
    p.pilot_spp = c->pilot_spp;
    p.tile_queue = S.d_sort_scratch + 1024;
    p.tile_cost = S.d_tile_cost;
}

// The slot's colour sums grow on demand to `layers` layers (a frame of this slot that is still in flight is waited for first);
// side_wait / ctx_wait name the two waits in the caller's words.
static int grow_colour_sums(mrt_ctx* c, mrt_ctx::FrameSlot& S, uint32_t layers, const char* side_wait, const char* ctx_wait) {
    if (S.pix_acc_layers >= layers) return MRT_OK;
    MRT_TRY(mrt::wait_stream(c, S.stream, side_wait));
    MRT_TRY(mrt::wait_stream(c, c->stream, ctx_wait));
    void* grown = nullptr;          // (the larger sums first: if they cannot be had, the slot keeps the ones it has)
    HIP_TRY(c, hipMalloc(&grown, (size_t)layers * mrt::local_texels_min1(c) * 16));
    mrt::free_device(S.d_pix_acc);
    S.d_pix_acc = grown;
    S.pix_acc_layers = layers;
    return MRT_OK;
}

// stream mode: every frame of a batch with the rng_shuffle it would have had on its own (lib.rs:305's stand-in)
static void batch_shuffles(const mrt_ctx* c, uint32_t batch, mrt::KParams& p) {
    for (uint32_t b = 0; b < batch; b++) {
        if (b == 0) std::memcpy(p.layer_shuffle[0], c->locals.rng_shuffle, 16);
        else mrt_frame_shuffle(c->seed, c->frames_done > UINT32_MAX - b ? UINT32_MAX : c->frames_done + b, p.layer_shuffle[b]);   // saturating, as :300
    }
}

// Camera-ray cluster masks and sphere lists (cam_mask.hip, one table of each from one build): which of the two this launch gets,
// the tables rebuilt first when they are stale and a build pays.
// The tables apply to a small scene of at most kCamMaskRecords top records whose table holds the shard, and to launches whose
// `texel` is the pixel's own: the stream mode's queue layers add a layer offset to it and run without them.
// A launch they apply to gets ONE of the two.  The lists (its camera rays are resolved in the lane: the SC = 3 instantiations of
// render_kernel) take a third of the wave iterations away and make each about a sixth longer: that pays where the launch is
// bound by throughput, and costs where it is bound by its longest pixel chains, whose many bounces per sample lose one slot in
// ten and pay the longer iteration on every one (C2, 2.5 pixels per resident lane: a quarter less work for the same frame time).  So a launch
// with fewer than kCamListMinPixelsPerLane pixels (tiles x queue layers x 64) per lane the chip holds gets the masks and runs
// the kernel it ran before the lists existed.  Measured on C3's scene at 64 spp (profiles/cam_list_rates.txt, "shapes around
// the rule"): up to 4.4 pixels per lane the frame takes the 8 ms of its longest chains whatever its size and the lists run 0.99 -
// 1.03 x the masks' time; at 5.3 they run 0.86 x, at 6.3 (1080p) 0.83 x.  The rule reads the calls and the device alone.
// mrt_debug_set_camera_masks can force either table.
// A stale table is rebuilt always from a threshold of samples per pixel and launch on, otherwise once the generation has survived a
// frame (a viewer that moves its camera every frame below that never pays a build).  The threshold is the measured build time over
// the measured saving per sample, both proportional to the pixel count: kCamListAlwaysSpp for a launch that gets the lists (2.4 -
// 2.9 ms at 1080p against 26 - 38 us per sample per pixel: a lone frame breaks even at about 96; profiles/cam_list_rates.txt),
// kCamMaskAlwaysSpp for one that gets the masks (3.2 ms against 5.7 - 6.6 us; profiles/cam_mask_rates.txt).
// The build runs on the frame's own side stream, behind enter_slot (the scene's uploads and refits are visible there) and ahead
// of the render launch, and every slot builds for itself before its first frame of a generation (they write the same words; a
// slot of a generation that some slot has built follows at once): a frame reads what its own stream has written, no stream
// waits for another one's build -- a wait would start the waiting frames as a convoy -- and no frame in flight is held back.
// Only a build for a NEW generation waits, for the other slots' frames that may still be reading the previous one.  Which
// launches run with the tables depends on the calls alone, never on timing.
static constexpr uint32_t kCamListAlwaysSpp = 96, kCamMaskAlwaysSpp = 512;
static constexpr uint64_t kCamListMinPixelsPerLane = 5;
static int camera_masks(mrt_ctx* c, mrt_ctx::FrameSlot& S, mrt::KParams& p) {
    p.cam_masks = nullptr;
    p.cam_lists = nullptr;
    c->cam_masks_in_force = false;
    c->cam_lists_in_force = false;
    if (!S.render_pending) { S.cam_used_gen = 0; S.cam_stale_reader = false; }
    const uint64_t gen = c->cam_mask_gen;
    const bool survived = c->cam_mask_seen == gen;
    c->cam_mask_seen = gen;
    const size_t need = (local_texels(c) + 7) / 8;
    const bool own_texel = p.queue_layers == 1u || c->locals.rng_mode == MRT_RNG_COUNTER;
    if (!c->cam_masks_on || !c->d_cam_masks || !mrt::scene_is_small(c->n_members) || c->n_padded > mrt::kCamMaskRecords || need == 0 ||
        need > c->cam_mask_entries || !own_texel)
        return MRT_OK;
    const bool lists = c->cam_prefer == 1u ||
                       (c->cam_prefer == 0u && (uint64_t)p.n_tiles * p.queue_layers * 64u >= kCamListMinPixelsPerLane * c->n_waves * 64u);
    if (S.cam_built != gen) {
        if (c->cam_mask_built != gen && !survived &&
            (uint64_t)c->locals.samples_per_frame * p.lane_frames < (lists ? kCamListAlwaysSpp : kCamMaskAlwaysSpp))
            return MRT_OK;
        for (mrt_ctx::FrameSlot& T : c->slot)
            if (&T != &S && T.render_pending && (T.cam_stale_reader || (T.cam_used_gen != 0 && T.cam_used_gen != gen)))
                HIP_TRY(c, hipStreamWaitEvent(S.stream, T.render_done, 0));
        mrt::KParams b = p;             // (a subset frame's p.n_tiles is its list's length: the masks cover the shard)
        b.tiles_x = c->tiles_x; b.n_tiles = c->n_tiles;
        const int e = mrt::launch_cam_masks(b, c->d_cam_masks, c->cam_lists(), (uint32_t)need, S.stream);
        if (e) return fail(c, MRT_ERR_HIP, "camera mask launch failed: %s", hipGetErrorString((hipError_t)e));
        S.cam_built = gen;
        c->cam_mask_built = gen;
    }
    if (S.cam_used_gen != 0 && S.cam_used_gen != gen) S.cam_stale_reader = true;      // (an earlier frame of this slot, still pending)
    S.cam_used_gen = gen;
    if (lists) p.cam_lists = c->cam_lists();
    else p.cam_masks = c->d_cam_masks;
    c->cam_lists_in_force = lists;
    c->cam_masks_in_force = true;
    return MRT_OK;
}

// side stream: wait for the scene / seeds uploads and for this slot's previous frame (n-2) to
// have been finalized (its colour sums and tile costs are about to be overwritten / used)
static int enter_slot(mrt_ctx* c, mrt_ctx::FrameSlot& S, const mrt::KParams& p) {
    if (c->inputs_dirty) {
        HIP_TRY(c, hipEventRecord(c->ev_inputs, c->stream));
        c->inputs_dirty = false;
    }
    HIP_TRY(c, hipStreamWaitEvent(S.stream, c->ev_inputs, 0));
    HIP_TRY(c, hipStreamWaitEvent(S.stream, S.finalize_done, 0));
    // (an earlier frame of this slot failed half way: its queue counter was never reset -- before the pilot launch, which
    // pulls from the same queue)
    if (S.queue_dirty) HIP_TRY(c, hipMemsetAsync(p.tile_queue, 0, sizeof(uint32_t), S.stream));
    return MRT_OK;
}

// launches outside the controller's reach -- batches, overrides, subset frames -- whose chains are a handful of bounces (fewer
// than 4 samples per pixel and launch): 8 waves per CU, round 3's rule for such frames
static uint32_t few_bounce_launch_waves(const mrt_ctx* c, uint32_t chain_spp) {
    return chain_spp < 4u && c->waves_per_cu_override == 0 ? std::min(c->n_waves, c->cus * 8u) : c->n_waves;
}

// the render launch on the slot's stream between its timing events, and the ctx's stream made to wait for it
static int launch_frame(mrt_ctx* c, mrt_ctx::FrameSlot& S, const mrt::KParams& p, uint32_t launch_waves) {
    const uint32_t ev = (uint32_t)(c->frame_seq % mrt_ctx::kEventRing);       // (the ring is indexed by the frame: schedule_frame reads it back)
    S.queue_dirty = true;                        // until this frame's last finalize pass has been queued
    HIP_TRY(c, hipEventRecord(c->ev_start[ev], S.stream));
    int e = mrt::launch_render(p, false, launch_waves, S.stream, &c->last_launch[0]);
    if (e) return fail(c, MRT_ERR_HIP, "render launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipEventRecord(c->ev_stop[ev], S.stream));
    HIP_TRY(c, hipEventRecord(S.render_done, S.stream));
    S.render_pending = true;
    S.render_seq = c->frame_seq;
    // caller's stream: blend into the accumulated framebuffer (shader.wgsl:383-385) once the render is done -- frame by frame
    HIP_TRY(c, hipStreamWaitEvent(c->stream, S.render_done, 0));
    return MRT_OK;
}

// one frame blended: the tail of State::redraw
static void advance_frame(mrt_ctx* c) {
    if (c->frames_done != UINT32_MAX) c->frames_done++;                   // saturating_add, lib.rs:300
    c->locals.framebuffer_weight = mrt_frame_weight(c->frames_done, c->args.max_framebuffer_weight);  // :301-304
    mrt_frame_shuffle(c->seed, c->frames_done, c->locals.rng_shuffle);    // :305 (deterministic stand-in)
}

// the launch's last blend has been queued on the ctx's stream
static int end_frame(mrt_ctx* c, mrt_ctx::FrameSlot& S) {
    HIP_TRY(c, hipEventRecord(S.finalize_done, c->stream));
    S.queue_dirty = false;
    c->frame_seq++;
    c->shuffle_overridden = false;
    return MRT_OK;
}

// Adaptive sampling's blend of one frame (after the render on the slot's stream): the n tiles of the slot's device list (list
// null: every tile) at their own weights, in place on the current framebuffer, on the ctx's stream; the host's copy of the
// counts follows.  p: the frame's parameters (its colour sums: p.pix_acc / p.n_blocks).
static int blend_tiles(mrt_ctx* c, const mrt::KParams& p, mrt_ctx::FrameSlot& S, const uint32_t* d_list, uint32_t n) {
    mrt::TileBlendArgs a{};
    a.pix_acc = p.pix_acc; a.pix_stride = p.pix_stride; a.n_blocks = p.n_blocks;
    a.fb = c->d_fb[c->target ^ 1];
    a.noise_s = c->d_noise_s;
    a.tile_frames = c->d_tile_frames;
    a.list = d_list;
    a.tile_cost = S.d_tile_cost;
    a.tile_queue = S.d_sort_scratch + 1024;
    a.n = n; a.width = c->args.width; a.height = c->args.height; a.tiles_x = c->tiles_x;
    a.spp = c->locals.samples_per_frame;
    a.max_w = c->args.max_framebuffer_weight;
    const int e = mrt::launch_tile_blend(a, c->stream);
    if (e) return fail(c, MRT_ERR_HIP, "per-tile blend launch failed: %s", hipGetErrorString((hipError_t)e));
    return MRT_OK;
}

extern "C" {

// State::redraw, lib.rs:241-307 (raytrace pass + swap + weight/shuffle update; the present
// pass needs a window surface and is out of scope)
// `batch` >= 1 consecutive frames with ONE render launch (batch > 1: stream mode only, see mrt_render): the raytrace pass
// of State::redraw for each of them, then per frame -- in order -- the blend, the swap and the weight / shuffle update.
static int redraw_frames(mrt_ctx* c, uint32_t batch, bool frames_in_lane = false) {
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_redraw: no scene (call mrt_set_world first)");
    HIP_TRY(c, hipSetDevice(c->device));
    const bool counter = c->locals.rng_mode == MRT_RNG_COUNTER;
    if (batch < 1 || batch > mrt::kMaxFrameBatch || (counter && batch != 1)) return fail(c, MRT_ERR_INVALID_ARG, "redraw_frames: batch %u", batch);
    // Launch width and frames in flight (the controller: schedule_frame below); a change waits for the frames under way.
    const bool adaptive = batch == 1 && c->waves_per_cu_override == 0 && c->frame_slots_override == 0 && c->n_tiles != 0 &&
                          c->locals.samples_per_frame != 0u;
    uint32_t frames_running = 0;
    {
        uint32_t want = c->frame_slots_override > 0 ? (uint32_t)c->frame_slots_override : 2u;
        if (adaptive) MRT_TRY(schedule_frame(c, counter, &want, &frames_running));
        MRT_TRY(set_frame_slots(c, want));
    }
    c->last_slot = (uint32_t)(c->frame_seq % c->frame_slots);
    mrt_ctx::FrameSlot& S = c->slot[c->last_slot];
    mrt::KParams p;
    frame_params(c, S, c->n_tiles, p);
    p.tile_order = nullptr;
    // Layers of colour sums.  Counter-RNG mode: one per block of MRT_COUNTER_BLOCK samples of the frame.  Stream
    // mode: one per frame of the batch, each with the rng_shuffle the frame would have had on its own (lib.rs:305's stand-in).
    const size_t n = mrt::local_texels_min1(c);
    {
        const uint32_t spp = c->locals.samples_per_frame;
        uint32_t layers = batch;
        if (counter && spp > MRT_COUNTER_BLOCK) layers = (spp + MRT_COUNTER_BLOCK - 1) / MRT_COUNTER_BLOCK;
        if ((uint64_t)layers * n >= (1ull << 32) || (uint64_t)layers * c->n_tiles >= (1ull << 26))
            return fail(c, MRT_ERR_INVALID_ARG, "mrt_redraw: %u layers of colour sums over %zu pixels exceed the tile queue's range", layers, n);
        MRT_TRY(grow_colour_sums(c, S, layers, "mrt_redraw: regrowing a slot's colour sums (its side stream)", __func__));
        // what mrt_debug_read_pixel_costs reads back: a counter-mode frame's cost is the sum over its blocks, a batch's last
        // frame is its last layer
        S.cost_first_layer = counter ? 0u : batch - 1u;
        S.cost_layers = counter ? layers : 1u;
        p.n_blocks = layers;
        p.pix_stride = (uint32_t)n;
        // a batch of SHORT frames: the queue holds every tile once, a lane renders its pixel for all frames of the batch
        const bool in_lane = frames_in_lane && !counter && batch > 1 && spp != 0;
        p.queue_layers = in_lane ? 1u : layers;
        p.lane_frames = in_lane ? batch : 1u;
        batch_shuffles(c, batch, p);
    }
    p.pix_acc = S.d_pix_acc;
    MRT_TRY(enter_slot(c, S, p));
    MRT_TRY(camera_masks(c, S, p));
    // The tile queue is ordered by the per-tile cost this slot measured two frames ago, heaviest
    // first; before the slot's first frame of a scene a small pilot launch (no output) provides
    // the estimate when the frame is long enough to pay for it.  Without an estimate: index order.
    // With no more tiles than persistent waves every tile starts at once and the order cannot matter: no pilot, no sort.
    // ... nor when a pixel's chain is a handful of bounces (fewer than 4 samples per pixel and launch): three launches saved.
    const uint32_t chain_spp = c->locals.samples_per_frame * p.lane_frames;
    uint32_t launch_waves = few_bounce_launch_waves(c, chain_spp);
    if (adaptive) {
        // (above: launch width) -- a share of the waves the chip HOLDS for this scene's kernel: a large scene's 16 per CU, not
        // the 20 of n_waves.  Shares of n_waves had made the frames in flight ask for a quarter more waves than fit: the 1/8
        // share of C5 ran at 0.82 lane utilisation instead of 0.92, C5 itself 4 % slower
        // ... and never a smaller share than the frames that really share the chip leave (width_policy.h, width_launch_div): a
        // caller that waits for every frame gets all of it
        const uint32_t whole = std::min(c->n_waves, mrt::render_resident_waves(p));
        launch_waves = std::max(whole / c->width.launch_div(frames_running), 1u);
    }
    bool piloted = false;
    if (c->lpt_enabled && c->n_tiles > launch_waves && chain_spp >= 4u) {
        if (!S.cost_valid && c->locals.samples_per_frame >= 8u * c->pilot_spp) {
            int pe = mrt::launch_render(p, true, launch_waves, S.stream, &c->last_launch[1]);
            if (pe) return fail(c, MRT_ERR_HIP, "pilot launch failed: %s", hipGetErrorString((hipError_t)pe));
            S.cost_valid = true;
            piloted = true;
        }
        if (S.cost_valid) {
            int se = mrt::launch_sort_tiles(S.d_tile_cost, S.d_tile_order, S.d_sort_scratch, c->n_tiles, S.stream);
            if (se) return fail(c, MRT_ERR_HIP, "tile sort launch failed: %s", hipGetErrorString((hipError_t)se));
            p.tile_order = S.d_tile_order;
        }
    }
    if (c->d_wave_log) {            // diagnostic (mrt_debug_wave_log): the frame's own part of the ring, cleared (a narrow launch leaves most of it unwritten)
        p.wave_log = c->d_wave_log + (size_t)(c->frame_seq % mrt_ctx::kWaveLogFrames) * c->wave_log_waves * 4;
        HIP_TRY(c, hipMemsetAsync(p.wave_log, 0, c->wave_log_waves * 4 * sizeof(unsigned long long), S.stream));
    }
    MRT_TRY(launch_frame(c, S, p, launch_waves));
    S.order_kind = p.tile_order ? MRT_TILE_ORDER_SORTED : MRT_TILE_ORDER_INDEX;     // (mrt_debug_read_tile_schedule)
    S.order_n = c->n_tiles;
    S.order_pilot = piloted;
    // (on the slot's stream right behind render_done, as ever: the ctx's stream waits for that event, already recorded)
    if (adaptive) {         // the launch-width controller's sample: cumulative world_hit calls and lane slots after this kernel
        // (counters 1 .. 3 in ONE copy: world_hit calls and lane slots of the same instant)
        HIP_TRY(c, hipMemcpyAsync(c->h_stats + 3 * c->last_slot, c->d_counters + 1, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, S.stream));
        HIP_TRY(c, hipEventRecord(S.stats_ready, S.stream));
        S.stats_seq = c->frame_seq;
        S.stats_pending = true;
    }
    for (uint32_t b = 0; b < batch; b++) {
        p.out = c->d_fb[c->target];              // framebuffers.target  (lib.rs:250)
        p.prev = c->d_fb[c->target ^ 1];         // framebuffers.secondary (lib.rs:265)
        p.locals.framebuffer_weight = c->locals.framebuffer_weight;
        if (!counter) { p.pix_acc = (char*)S.d_pix_acc + (size_t)b * n * 16; p.n_blocks = 1; }
        if (c->tiles_diverged) {                 // adaptive sampling has begun: every tile at its own weight, in place (no swap)
            MRT_TRY(blend_tiles(c, p, S, nullptr, c->n_tiles));
        } else {
            int fe = mrt::launch_finalize(p, c->stream, c->d_noise_s);
            if (fe) return fail(c, MRT_ERR_HIP, "finalize launch failed: %s", hipGetErrorString((hipError_t)fe));
            c->noise_c2 = mrt::noise_c2_next(c->noise_c2, p.locals.framebuffer_weight);   // (the weight this blend used)
            c->target ^= 1;                                                   // framebuffers.swap(), lib.rs:299
        }
        advance_frame(c);
        if (c->tiles_diverged)
            for (uint32_t& t : c->tile_frames) t += t != UINT32_MAX ? 1u : 0u;
    }
    MRT_TRY(end_frame(c, S));
    S.cost_valid = true;
    return MRT_OK;
}

int mrt_redraw(mrt_ctx* c) {
    if (!c) return MRT_ERR_INVALID_ARG;
    return redraw_frames(c, 1);
}

// `frames` x State::redraw.  Frames are independent until their blend (each has its own rng_shuffle and its own colour
// sums), so when the shard has too few pixels to fill the GPU -- a pixel is one sequential chain of samples -- one launch
// renders up to kMaxFrameBatch consecutive frames: a lane that finishes a pixel of frame f takes one of frame f+1.  Every
// frame's image is the one mrt_redraw would have produced.
static constexpr uint64_t kBatchBytes = 1ull << 30;     // colour sums of one launch's frames (x 2 slots): 32 frames of 1080p, 8 of 4K
int mrt_render(mrt_ctx* c, uint32_t frames) {
    if (!c) return MRT_ERR_INVALID_ARG;
    while (frames != 0) {
        uint32_t batch = 1;
        if (c->batch_frames && frames >= 2 && c->locals.rng_mode == MRT_RNG_PIXEL_STREAM && !c->shuffle_overridden && c->n_tiles != 0) {
            // too few pixels to fill the GPU (fewer than two per lane): about six pixel chains per lane (they differ 10 x in length)
            // -- for SHORT chains only: from 64 samples per pixel on, frames launched one by one run eight at a time on an eighth
            // of the waves each (redraw_frames), which packs the lanes better than the layers of a batch do (C5's 1/8 share:
            // 2,380 Msamples/s at 0.68 lane utilisation in batches of 7, 2,660 at 0.92 frame by frame)
            uint32_t want = (c->n_tiles < 2u * c->n_waves && c->locals.samples_per_frame < 64u) ? (6u * c->n_waves + c->n_tiles - 1u) / c->n_tiles : 1u;
            // too short a frame (1 spp interactive accumulation: 0.2 ms of work behind six launches): about 128 M samples per launch
            const uint64_t per_frame = (uint64_t)c->n_tiles * 64u * std::max(c->locals.samples_per_frame, 1u);
            want = std::max<uint64_t>(want, ((128ull << 20) + per_frame - 1) / per_frame);
            batch = std::min(std::min(frames, (uint32_t)mrt::kMaxFrameBatch), std::max(want, 1u));
            // every frame of a batch parks its colour sums in a layer of its own (16 B per pixel): at most kBatchBytes per slot
            const uint64_t layer_bytes = (uint64_t)std::max<size_t>(local_texels(c), 1) * 16u;
            batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(batch, kBatchBytes / layer_bytes));
        }
        // Two reasons to batch, two forms (kernels.hip): a shard with too few pixels needs more pixel chains at once -- the
        // frames of the batch become layers of the tile queue; a frame that is merely short has pixels enough -- the lane that
        // takes a pixel renders it for every frame of the batch (one queue atomic / seed fetch per pixel and batch).
        // (In-lane only below 4 samples per frame: it makes a pixel's chain `batch` times longer, which costs the launch's tail
        // more than the acquisitions cost from 8 samples up -- measured, DESIGN.md: 1 spp 5,470 -> 10,360 Msamples/s, 8 spp
        // 11,260 -> 11,050, C2's 64 spp 11,640 -> 10,650.)
        const bool starved = c->n_tiles < 2u * c->n_waves;
        const bool in_lane = !starved && c->locals.samples_per_frame < 4u;      // (a batch of 1 is a plain redraw, whatever its form)
        int st = redraw_frames(c, batch, c->batch_form == 0 ? in_lane : c->batch_form == 1);
        if (st != MRT_OK) return st;
        frames -= batch;
    }
    return MRT_OK;
}

// ---- adaptive sampling (include/myraytracer_amd.h, "adaptive sampling") ------------------------------------------------------
// A subset frame renders its listed tiles through the unchanged render kernel: n_tiles = the list's length (the queue's length;
// with one queue layer it is never a layer stride, hence no counter mode beyond MRT_COUNTER_BLOCK samples), tile_order = the list,
// heaviest first by the slot's tile costs when the render has more tiles than waves.  No pilot launch, and the launch-width
// controller neither sees nor restarts for these frames (their sizes vary): they use the setting in force.  Then blend_tiles.

// the first subset frame since create / reset: every tile's count starts at frames_done (behind everything on the ctx's stream)
static int begin_tile_frames(mrt_ctx* c) {
    if (c->tiles_diverged) return MRT_OK;
    if (!c->d_tile_frames) HIP_TRY(c, hipMalloc((void**)&c->d_tile_frames, (size_t)c->n_tiles * sizeof(uint32_t)));
    HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)c->d_tile_frames, (int)c->frames_done, c->n_tiles, c->stream));
    c->tile_frames.assign(c->n_tiles, c->frames_done);
    c->tiles_diverged = true;
    return MRT_OK;
}

// mrt_debug_load_accumulation's bound on a loaded n_t: the K tables have an entry per count (12 bytes each on the device)
static constexpr uint32_t kMaxLoadedTileFrames = 1u << 20;

// the slot's tile list on the device and its pinned staging copy, on first use
static int alloc_tile_list(mrt_ctx* c, mrt_ctx::FrameSlot& S) {
    if (!S.d_tile_list) HIP_TRY(c, hipMalloc((void**)&S.d_tile_list, (size_t)c->n_tiles * sizeof(uint32_t)));
    if (!S.h_tile_list) HIP_TRY(c, hipHostMalloc((void**)&S.h_tile_list, (size_t)c->n_tiles * sizeof(uint32_t), hipHostMallocDefault));
    return MRT_OK;
}

// `batch` consecutive subset frames over the n tiles of `tiles` in ONE render launch (batch > 1: the in-lane form only)
static int render_subset(mrt_ctx* c, const uint32_t* tiles, uint32_t n, uint32_t batch) {
    c->last_slot = (uint32_t)(c->frame_seq % c->frame_slots);
    mrt_ctx::FrameSlot& S = c->slot[c->last_slot];
    mrt::KParams p;
    frame_params(c, S, n, p);
    {   // back-pressure, as a frame of mrt_render: the slot's previous render kernel has completed (its list copy with it)
        char what[128];
        std::snprintf(what, sizeof what, "mrt_render_tiles: back-pressure of slot %u (next frame %llu)", c->last_slot,
                      (unsigned long long)c->frame_seq);
        if (S.render_pending) MRT_TRY(mrt::wait_event(c, S.render_done, what));
        S.render_pending = false;
    }
    MRT_TRY(alloc_tile_list(c, S));
    std::memcpy(S.h_tile_list, tiles, (size_t)n * sizeof(uint32_t));
    const size_t texels = mrt::local_texels_min1(c);
    MRT_TRY(grow_colour_sums(c, S, batch, "mrt_render_tiles: regrowing a slot's colour sums (its side stream)", __func__));
    S.cost_first_layer = batch - 1u;
    S.cost_layers = 1u;
    p.n_blocks = batch;
    p.pix_stride = (uint32_t)texels;
    p.queue_layers = 1u;
    p.lane_frames = batch;
    batch_shuffles(c, batch, p);
    p.pix_acc = S.d_pix_acc;
    MRT_TRY(enter_slot(c, S, p));
    MRT_TRY(camera_masks(c, S, p));
    HIP_TRY(c, hipMemcpyAsync(S.d_tile_list, S.h_tile_list, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, S.stream));
    // launch width: the setting in force (the controller's last launch), and round 3's 8 waves per CU for chains of a few bounces
    const uint32_t chain_spp = c->locals.samples_per_frame * batch;
    uint32_t launch_waves = few_bounce_launch_waves(c, chain_spp);
    if (c->width.s.div != 0 && c->waves_per_cu_override == 0 && c->frame_slots_override == 0) {
        const uint32_t whole = std::min(c->n_waves, mrt::render_resident_waves(p));
        launch_waves = std::max(whole / std::max(c->width.last_launch_div, 1u), 1u);
    }
    p.tile_order = S.d_tile_list;                // (a subset launch always passes its list: null would mean tiles 0 .. n - 1)
    if (c->lpt_enabled && S.cost_valid && n > launch_waves && chain_spp >= 4u) {
        int se = mrt::launch_sort_tile_list(S.d_tile_cost, S.d_tile_list, S.d_tile_order, S.d_sort_scratch, n, S.stream);
        if (se) return fail(c, MRT_ERR_HIP, "tile list sort launch failed: %s", hipGetErrorString((hipError_t)se));
        p.tile_order = S.d_tile_order;
    }
    MRT_TRY(launch_frame(c, S, p, launch_waves));
    S.order_kind = p.tile_order == S.d_tile_order ? MRT_TILE_ORDER_SORTED_LIST : MRT_TILE_ORDER_LIST;     // (mrt_debug_read_tile_schedule)
    S.order_n = n;
    S.order_pilot = false;
    for (uint32_t b = 0; b < batch; b++) {
        p.pix_acc = (char*)S.d_pix_acc + (size_t)b * texels * 16;
        p.n_blocks = 1;
        MRT_TRY(blend_tiles(c, p, S, S.d_tile_list, n));
        for (uint32_t i = 0; i < n; i++) {
            uint32_t& t = c->tile_frames[tiles[i]];
            t += t != UINT32_MAX ? 1u : 0u;
        }
        advance_frame(c);
    }
    return end_frame(c, S);
}

int mrt_render_tiles(mrt_ctx* c, const uint32_t* tiles, size_t n, uint32_t frames) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (n == 0 || frames == 0) return MRT_OK;
    if (!tiles) return fail(c, MRT_ERR_INVALID_ARG, "mrt_render_tiles: tiles is NULL");
    if (c->shard_world != 1) return fail(c, MRT_ERR_STATE, "mrt_render_tiles: a shard (world %u) renders whole frames only", c->shard_world);
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_render_tiles: no scene (call mrt_set_world first)");
    const bool counter = c->locals.rng_mode == MRT_RNG_COUNTER;
    if (counter && c->locals.samples_per_frame > MRT_COUNTER_BLOCK)
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_render_tiles: counter mode renders at most %u samples per frame by tiles (%u)",
                    (unsigned)MRT_COUNTER_BLOCK, c->locals.samples_per_frame);
    if (n > c->n_tiles) return fail(c, MRT_ERR_INVALID_ARG, "mrt_render_tiles: %zu tiles listed, the image has %u", n, c->n_tiles);
    {
        std::vector<uint8_t> seen(c->n_tiles, 0);
        for (size_t i = 0; i < n; i++) {
            if (tiles[i] >= c->n_tiles) return fail(c, MRT_ERR_INVALID_ARG, "mrt_render_tiles: tile %u of %u", tiles[i], c->n_tiles);
            if (seen[tiles[i]]++) return fail(c, MRT_ERR_INVALID_ARG, "mrt_render_tiles: tile %u listed twice", tiles[i]);
        }
    }
    // every tile: whole frames (today's path while the accumulation is uniform; blended per tile after a subset frame)
    if (n == c->n_tiles) return mrt_render(c, frames);
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(begin_tile_frames(c));
    while (frames != 0) {
        // The frames of one call share one launch in the in-lane form (a lane renders its pixel for every frame of the batch);
        // never the layered form.  At 1080p x 1 spp the adaptive run to the same stop took 84 ms so, 119-175 ms with a launch
        // per frame (most lists are short; profiles/adaptive_rates.txt).  mrt_debug_set_frame_batching(0): a launch per frame.
        uint32_t batch = 1;
        if (c->batch_frames && c->batch_form != 2 && !counter && !c->shuffle_overridden && c->locals.samples_per_frame != 0u) {
            const uint64_t layer_bytes = (uint64_t)std::max<size_t>(local_texels(c), 1) * 16u;
            batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)frames, (uint64_t)mrt::kMaxFrameBatch, kBatchBytes / layer_bytes}));
        }
        MRT_TRY(render_subset(c, tiles, (uint32_t)n, batch));
        frames -= batch;
    }
    return MRT_OK;
}

int mrt_debug_set_frame_batching(mrt_ctx* c, int enabled) {
    if (!c) return MRT_ERR_INVALID_ARG;
    c->batch_frames = enabled != 0;
    c->batch_form = enabled == 2 ? 1 : enabled == 3 ? 2 : 0;
    return MRT_OK;
}

// diagnostic: per-pixel cost (bounce-loop trips) of the last frame, this shard's packed rows
int mrt_debug_read_pixel_costs(mrt_ctx* c, uint32_t* out, size_t cap) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    const size_t n = local_texels(c);
    if (cap < n) return fail(c, MRT_ERR_TOO_SMALL, "mrt_debug_read_pixel_costs: need %zu", n);
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, __func__));
    const mrt_ctx::FrameSlot& S = c->slot[c->last_slot];
    std::vector<uint32_t> tmp(n * 4), layer(n * 4);
    HIP_TRY(c, hipMemcpyAsync(tmp.data(), (const char*)S.d_pix_acc + (size_t)S.cost_first_layer * n * 16, n * 16, hipMemcpyDeviceToHost, c->stream));
    MRT_TRY(mrt::wait_stream(c, c->stream, __func__));
    for (uint32_t b = 1; b < S.cost_layers; b++) {       // counter mode: a pixel's cost is the sum over its blocks
        HIP_TRY(c, hipMemcpyAsync(layer.data(), (const char*)S.d_pix_acc + (size_t)(S.cost_first_layer + b) * n * 16, n * 16, hipMemcpyDeviceToHost, c->stream));
        MRT_TRY(mrt::wait_stream(c, c->stream, __func__));
        for (size_t i = 0; i < n; i++) tmp[4 * i + 3] += layer[4 * i + 3];
    }
    for (size_t i = 0; i < n; i++) out[i] = tmp[4 * i + 3];
    return MRT_OK;
}

// diagnostic: the very sort a frame's queue gets, on caller-supplied costs, staged through the last slot's own buffers
int mrt_debug_sort_tiles(mrt_ctx* c, const uint32_t* cost, size_t n_cost, const uint32_t* list, size_t n, uint32_t* order_out) {
    if (!c || !cost || !order_out) return MRT_ERR_INVALID_ARG;
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_debug_sort_tiles: no scene (call mrt_set_world first)");
    if (n_cost == 0 || n_cost > c->n_tiles) return fail(c, MRT_ERR_INVALID_ARG, "mrt_debug_sort_tiles: %zu costs, the context has %u tiles", n_cost, c->n_tiles);
    if (list ? (n == 0 || n > n_cost) : n != n_cost) return fail(c, MRT_ERR_INVALID_ARG, "mrt_debug_sort_tiles: %zu entries of %zu costs", n, n_cost);
    for (size_t i = 0; list && i < n; i++)
        if (list[i] >= n_cost) return fail(c, MRT_ERR_INVALID_ARG, "mrt_debug_sort_tiles: tile %u of %zu", list[i], n_cost);
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, __func__));
    mrt_ctx::FrameSlot& S = c->slot[c->last_slot];
    if (list) MRT_TRY(alloc_tile_list(c, S));
    // whatever comes next, the slot's costs are no estimate of a frame any more and its recorded order is gone
    S.cost_valid = false;
    S.order_kind = MRT_TILE_ORDER_NONE; S.order_n = 0; S.order_pilot = false;
    HIP_TRY(c, hipMemcpyAsync(S.d_tile_cost, cost, n_cost * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (list) HIP_TRY(c, hipMemcpyAsync(S.d_tile_list, list, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const int se = list ? mrt::launch_sort_tile_list(S.d_tile_cost, S.d_tile_list, S.d_tile_order, S.d_sort_scratch, (uint32_t)n, c->stream)
                        : mrt::launch_sort_tiles(S.d_tile_cost, S.d_tile_order, S.d_sort_scratch, (uint32_t)n, c->stream);
    if (se) return fail(c, MRT_ERR_HIP, "mrt_debug_sort_tiles: sort launch failed: %s", hipGetErrorString((hipError_t)se));
    HIP_TRY(c, hipMemcpyAsync(order_out, S.d_tile_order, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    return mrt::wait_stream(c, c->stream, __func__);
}

// diagnostic: the last slot's tile costs as its last finalize / blend left them, and the queue order of its most recent launch
int mrt_debug_read_tile_schedule(mrt_ctx* c, uint32_t* cost_out, uint32_t* order_out, size_t cap, uint32_t* n_out, uint32_t info_out[4]) {
    if (!c || !n_out || !info_out) return MRT_ERR_INVALID_ARG;
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "mrt_debug_read_tile_schedule: no scene (call mrt_set_world first)");
    const size_t n = c->n_tiles;
    *n_out = c->n_tiles;
    if (cap < n) return fail(c, MRT_ERR_TOO_SMALL, "mrt_debug_read_tile_schedule: need %zu values", n);
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, __func__));
    const mrt_ctx::FrameSlot& S = c->slot[c->last_slot];
    info_out[0] = S.order_kind; info_out[1] = S.order_n; info_out[2] = S.order_pilot ? 1u : 0u; info_out[3] = c->last_slot;
    if (cost_out && n) HIP_TRY(c, hipMemcpyAsync(cost_out, S.d_tile_cost, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (order_out && S.order_n) {
        if (S.order_kind == MRT_TILE_ORDER_INDEX) {
            for (uint32_t i = 0; i < S.order_n; i++) order_out[i] = i;           // (tile_order null: the kernel takes the queue position)
        } else {
            const uint32_t* src = S.order_kind == MRT_TILE_ORDER_LIST ? S.d_tile_list : S.d_tile_order;
            HIP_TRY(c, hipMemcpyAsync(order_out, src, (size_t)S.order_n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        }
    }
    return mrt::wait_stream(c, c->stream, __func__);
}

int mrt_debug_last_launch(mrt_ctx* c, uint32_t out[2]) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    out[0] = c->last_launch[0]; out[1] = c->last_launch[1];
    c->last_launch[1] = 0xFFFFFFFFu;            // a pilot launch is reported once
    return MRT_OK;
}

// diagnostic / A-B switch: 0 = tile queue in index order instead of heaviest-first
int mrt_debug_set_tile_sort(mrt_ctx* c, int enabled) {
    if (!c) return MRT_ERR_INVALID_ARG;
    c->lpt_enabled = enabled != 0;
    return MRT_OK;
}

// diagnostic / tuning: pilot spp, waves per CU (0 = automatic).
// Call before rendering.
int mrt_debug_set_schedule(mrt_ctx* c, uint32_t pilot_spp, int waves_per_cu) {
    if (!c) return MRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, __func__));
    if (c->frames_done != 0) return fail(c, MRT_ERR_STATE, "mrt_debug_set_schedule: frames already rendered");
    const uint32_t old_pilot = c->pilot_spp;
    const int old_waves = c->waves_per_cu_override;
    c->pilot_spp = pilot_spp ? pilot_spp : 1;
    c->waves_per_cu_override = waves_per_cu;
    const int st = alloc_frame_buffers(c, c->shard_rank, c->shard_world);
    if (st != MRT_OK) { c->pilot_spp = old_pilot; c->waves_per_cu_override = old_waves; }
    return st;
}

int mrt_get_schedule(mrt_ctx* c, uint32_t out[6]) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    const mrt::WidthController& W = c->width;
    out[0] = W.s.div; out[1] = W.s.mult; out[2] = W.s.settled;
    out[3] = W.s.div ? W.frames_in_flight() : c->frame_slots;
    out[4] = W.last_launch_div;
    out[5] = W.slots_probed ? W.max_slots : 0u;      // 0 = not measured yet (no setting has asked for more than two frames)
    return MRT_OK;
}

int mrt_set_schedule_hint(mrt_ctx* c, uint32_t div, uint32_t mult) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (!(div == 0 && mult == 0) && !mrt::width_hint_valid(div, mult))
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_set_schedule_hint: div %u x mult %u (div 1..8, mult 1..8, max(2, div) x mult <= 16)", div, mult);
    c->width.set_hint(div, mult);       // the next redraw takes the hint (or starts measuring again)
    return MRT_OK;
}

int mrt_debug_width_policy(int op, const uint32_t workload[6], uint32_t state[7], double util, double rate) {
    if (!workload || !state || op < 0 || op > 2) return MRT_ERR_INVALID_ARG;
    mrt::WidthWorkload w;
    w.n_tiles = workload[0]; w.n_waves = workload[1]; w.max_slots = workload[2]; w.spp = workload[3]; w.n_members = workload[4]; w.counter = workload[5];
    mrt::WidthState s;
    float pr;
    std::memcpy(&pr, &state[6], 4);
    s.div = state[0]; s.mult = state[1]; s.prev_div = state[2]; s.prev_mult = state[3]; s.low_windows = state[4]; s.settled = state[5]; s.prev_rate = pr;
    if (op == 0) mrt::width_policy_start(s, w);
    else if (op == 1) { mrt::WidthWindow m; m.util = util; m.rate = rate; mrt::width_policy_step(s, w, m); }
    else { state[0] = mrt::width_launch_div(s.div, (uint32_t)util); return MRT_OK; }
    pr = (float)s.prev_rate;
    state[0] = s.div; state[1] = s.mult; state[2] = s.prev_div; state[3] = s.prev_mult; state[4] = s.low_windows; state[5] = s.settled;
    std::memcpy(&state[6], &pr, 4);
    return MRT_OK;
}

// a fresh controller through the caller's synthetic frame calls: schedule_frame's sequence with the device's answers given
int mrt_debug_width_replay(uint32_t probe_slots, size_t n_calls, const uint32_t* calls, const double* times, const uint64_t* samples,
                           size_t n_samples, uint32_t* out, double* measured) {
    if (!calls || !times || !out || !measured || (n_samples && !samples) || probe_slots == 1 || probe_slots > mrt::kMaxFrameSlots) return MRT_ERR_INVALID_ARG;
    mrt::WidthController W;
    uint32_t frame_slots = 2;           // (redraw_frames: set_frame_slots(want) after every call)
    size_t next_sample = 0;
    for (size_t i = 0; i < n_calls; i++) {
        const uint32_t* in = calls + MRT_WIDTH_CALL_WORDS * i;
        mrt::WidthWorkload w;
        w.n_tiles = in[0]; w.n_waves = in[1]; w.max_slots = in[2]; w.spp = in[3]; w.n_members = in[4]; w.counter = in[5]; w.n_spheres = in[6];
        const uint32_t hint_div = in[7], hint_mult = in[8], running = in[10], n = in[11];
        if (w.n_tiles == 0 || w.n_waves == 0 || w.max_slots < 1 || w.max_slots > mrt::kMaxFrameSlots || in[12] > n_samples - next_sample ||
            (!(hint_div == 0 && hint_mult == 0) && !mrt::width_hint_valid(hint_div, hint_mult)))
            return MRT_ERR_INVALID_ARG;
        if (i == 0) W.max_slots = w.max_slots;
        if (hint_div != W.hint_div || hint_mult != W.hint_mult) W.set_hint(hint_div, hint_mult);
        if (in[9]) W.invalidate();
        const uint64_t frame_seq = i;
        const double now = times[2 * i];
        W.begin_workload(w, frame_seq);
        for (uint32_t k = 0; k < in[12]; k++, next_sample++) W.add_sample(samples[3 * next_sample], samples[3 * next_sample + 1], samples[3 * next_sample + 2]);
        const uint32_t frames_running = W.note_running(frame_seq, running);
        W.open_window(frame_seq, now);
        mrt::WidthWindow m{0.0, 0.0};
        const bool due = W.window_due(frame_seq, now);
        if (due) m = W.close_window(w, frame_seq, now, frame_slots, n, times[2 * i + 1]);
        if (W.wants_probe()) W.after_probe(probe_slots ? probe_slots : mrt::kMaxFrameSlots, w, frame_seq);
        frame_slots = W.frames_in_flight();
        uint32_t* o = out + MRT_WIDTH_DECISION_WORDS * i;
        o[0] = W.s.div; o[1] = W.s.mult; o[2] = W.s.settled; o[3] = frame_slots; o[4] = frames_running; o[5] = W.launch_div(frames_running);
        o[6] = W.timing ? 1u : 0u; o[7] = due ? 1u : 0u; o[8] = (uint32_t)W.memo.size();
        measured[2 * i] = m.util; measured[2 * i + 1] = m.rate;
    }
    return MRT_OK;
}

int mrt_debug_stream_concurrency(mrt_ctx* c, uint32_t streams, float* out) {
    if (!c || !out || streams < 2 || streams > mrt_ctx::kMaxFrameSlots) return MRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    return probe_stream_concurrency(c, streams, out);
}

int mrt_debug_set_frames_in_flight(mrt_ctx* c, int slots) {
    if (!c || slots < 0 || slots > (int)mrt_ctx::kMaxFrameSlots) return MRT_ERR_INVALID_ARG;
    c->frame_slots_override = slots;
    return MRT_OK;
}

// diagnostic of the stream ordering: one clock- and poll-bounded single-wave kernel (launch_hold) on a stream the context HAS
int mrt_debug_hold(mrt_ctx* c, uint32_t which, uint32_t index, uint64_t ticks, uint32_t max_polls) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (ticks == 0 || ticks > MRT_HOLD_MAX_TICKS || max_polls == 0 || which > MRT_HOLD_NOISE ||
        index >= (which == MRT_HOLD_SLOT ? mrt_ctx::kMaxFrameSlots : 1u))
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_debug_hold: stream %u, index %u, %llu ticks (1..%llu), %u polls (>= 1)", which, index,
                    (unsigned long long)ticks, (unsigned long long)MRT_HOLD_MAX_TICKS, max_polls);
    const hipStream_t s = which == MRT_HOLD_CONTEXT ? c->stream : which == MRT_HOLD_SLOT ? c->slot[index].stream
                          : which == MRT_HOLD_PRESENT ? c->present_stream : c->noise_stream;
    if (!s || !c->h_stats) return fail(c, MRT_ERR_STATE, "mrt_debug_hold: stream %u (index %u) does not exist yet", which, index);
    HIP_TRY(c, hipSetDevice(c->device));
    const int e = mrt::launch_hold(ticks, max_polls, c->h_stats + 5 * mrt_ctx::kMaxFrameSlots - 2, s);
    if (e) return fail(c, MRT_ERR_HIP, "mrt_debug_hold: launch failed: %s", hipGetErrorString((hipError_t)e));
    c->hold_polls = max_polls;
    return MRT_OK;
}

int mrt_debug_hold_stamps(mrt_ctx* c, uint64_t out[3]) {
    if (!c || !out || !c->h_stats) return MRT_ERR_INVALID_ARG;
    const unsigned long long* const stamps = c->h_stats + 5 * mrt_ctx::kMaxFrameSlots - 2;
    out[0] = c->hold_polls ? stamps[0] : 0; out[1] = c->hold_polls ? stamps[1] : 0; out[2] = c->hold_polls;
    return MRT_OK;
}

// n_t per tile (frames_done everywhere while the accumulation is uniform); synchronises as mrt_read_framebuffer does
int mrt_read_tile_frames(mrt_ctx* c, uint32_t* out, size_t cap, uint32_t* tiles_x, uint32_t* tiles_rows) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (tiles_x) *tiles_x = c->tiles_x;
    if (tiles_rows) *tiles_rows = c->local_bands;
    if (!out) return MRT_ERR_INVALID_ARG;
    const size_t n = c->n_tiles;
    if (cap < n) return fail(c, MRT_ERR_TOO_SMALL, "mrt_read_tile_frames: need %zu values", n);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->tiles_diverged && n) HIP_TRY(c, hipMemcpyAsync(out, c->d_tile_frames, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    MRT_TRY(mrt::wait_stream(c, c->stream, __func__));
    if (!c->tiles_diverged) std::fill(out, out + n, c->frames_done);
    return MRT_OK;
}

// diagnostic: an accumulation of the caller's in the place of the context's own (world 1; allocates nothing beyond what the first
// subset frame would)
int mrt_debug_load_accumulation(mrt_ctx* c, const float* rgba, const float* S, const uint32_t* tile_frames) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (c->shard_world != 1) return fail(c, MRT_ERR_STATE, "mrt_debug_load_accumulation: a shard (world %u)", c->shard_world);
    if (S && !c->noise_on) return fail(c, MRT_ERR_STATE, "mrt_debug_load_accumulation: S without noise tracking (mrt_set_noise_tracking)");
    for (uint32_t t = 0; tile_frames && t < c->n_tiles; t++)
        if (tile_frames[t] >= kMaxLoadedTileFrames)
            return fail(c, MRT_ERR_INVALID_ARG, "mrt_debug_load_accumulation: tile %u at %u frames (< %u)", t, tile_frames[t], kMaxLoadedTileFrames);
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, __func__));
    const size_t n = (size_t)c->args.width * c->args.height;
    if (rgba && n) HIP_TRY(c, hipMemcpyAsync(c->d_fb[c->target ^ 1], rgba, n * 16, hipMemcpyHostToDevice, c->stream));
    if (S && n) HIP_TRY(c, hipMemcpyAsync(c->d_noise_s, S, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (tile_frames && c->n_tiles) {
        MRT_TRY(begin_tile_frames(c));
        HIP_TRY(c, hipMemcpyAsync(c->d_tile_frames, tile_frames, (size_t)c->n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        c->tile_frames.assign(tile_frames, tile_frames + c->n_tiles);
    }
    return mrt::wait_stream(c, c->stream, __func__);        // (the caller's arrays are pageable: theirs again on return)
}

}  // extern "C"
