// The launch-width controller's POLICY, free of HIP and of the clock: what frames.cpp's frame loop (redraw_frames) decides
// with, and what tests/test_width_policy.py drives with synthetic measurement windows on the CPU (through
// mrt_debug_width_policy, include/myraytracer_amd_debug.h).  Scheduling only -- no decision here can change an image.
//
// The reference has one schedule: one full-screen draw per State::redraw, one frame after the other (lib.rs:241-307).  Here a
// frame is launched on 1 / div of the persistent waves the chip holds and max(2, div) x mult frames are in flight:
// narrow launches pack the lanes better (more pixels per lane in sequence) at the price of latency, and do not always pay, so
// a narrower width (or, where a frame has too few tiles to be launched any narrower, twice the frames in flight) is TRIED while
// the measured lane utilisation is low, and kept only if the measured frame rate rises by 3 %.
//
// Below the policy, the controller's BOOKKEEPING (WidthController): which workload a setting belongs to, the memo of settled
// settings, the frames the caller keeps in flight, the measurement windows and the samples they are judged by.  Free of HIP and
// of the clock as well: time enters as seconds the caller passes in, what the device measured as plain numbers.  frames.cpp's
// schedule_frame feeds it from the events and the pinned counters; tests/test_width_controller_host.py drives it with synthetic
// frame calls on the CPU (mrt_debug_width_replay).
#pragma once
#include <stdint.h>

#include <vector>

#include "mrt_internal.h"

namespace mrt {

struct WidthWorkload {
    uint32_t n_tiles;       // 8x8 tiles of the (shard of the) frame
    uint32_t n_waves;       // persistent waves of a full-width launch
    uint32_t max_slots;     // most frames that can be in flight (mrt_ctx::kMaxFrameSlots, capped by the hardware queues)
                            // (a launch is never narrower than 1 / kMaxWidthDiv, whatever max_slots)
    uint32_t spp;           // samples per pixel and frame
    uint32_t n_members;     // member slots of the scene's hierarchy (!scene_is_small: the large-scene kernels)
    uint32_t counter;       // counter-RNG mode
    uint32_t n_spheres = 0; // the scene's spheres (the memo's key only: no rule of the policy reads it)
};

constexpr uint32_t kMaxWidthDiv = 8;    // the narrowest launch: an eighth of the persistent waves
constexpr uint32_t kMaxFrameSlots = 16; // the most frames in flight (mrt_ctx::kMaxFrameSlots: the slots a context has)

struct WidthState {
    uint32_t div = 0, mult = 1;             // div 0 = not chosen yet for the current workload
    uint32_t prev_div = 0, prev_mult = 1;   // prev_div != 0: a trial is running; what it would return to
    uint32_t low_windows = 0;               // consecutive windows between the two utilisation thresholds (a trial takes two)
    uint32_t settled = 0;                   // no further trials for this workload
    double prev_rate = 0.0;                 // frames / s measured at (prev_div, prev_mult)
};

// one measurement window: lane utilisation of the frames at the current setting, their rate on the host's clock
struct WidthWindow { double util, rate; };

inline uint32_t width_min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
inline uint32_t width_max_u32(uint32_t a, uint32_t b) { return a > b ? a : b; }

// frames in flight of a setting
inline uint32_t width_frames_in_flight(uint32_t div, uint32_t mult, uint32_t max_slots) {
    return width_min_u32(width_max_u32(2u, div) * width_max_u32(mult, 1u), width_max_u32(max_slots, 1u));
}

// What is known up front.
//  * A pixel-starved launch of long chains (fewer than two pixels per lane the chip holds, one sequential chain of >= 64
//    samples each: an 8-GPU share of C5) lasts as long as its heaviest pixel while most of its waves are done far earlier, and
//    a wave's iteration takes the same time at 1 to 4 waves per SIMD: eight frames at a time, each on an eighth of the waves
//    (C5's 1/8 share, one mrt_redraw per frame: 885 Msamples/s at 0.41 lane utilisation with 2 frames in flight on all waves
//    -> 3,090 at 0.92 with 8) -- and, where the process has the hardware queues, eight MORE queued behind them: frames end out
//    of order, a frame slot is reused only when ITS frame has ended, and between a launch's end and the next launch on its
//    slot a sixth of the chip's wave slots stood empty (profiles/r05_shard_occupancy.txt); with twice the launches the chip
//    holds, every workgroup that ends is replaced at once by one that waits (3,090 -> 3,705).
//  * Chains of a few bounces (the reference's default: ONE sample per frame): a frame is bound by its longest path -- up to
//    ray_depth wave-iterations in sequence -- not by throughput, and every iteration is shorter with fewer resident waves: a
//    quarter of the waves, four frames side by side (the trials go on from there: 1080p at 1 spp ends at an eighth, sixteen
//    in flight: 7,150 -> 9,810 Msamples/s).
//  * Frames with tiles to spare (three per persistent wave and more: six per wave of a half-width launch): a half, and -- the
//    rule for every narrow launch -- TWICE the
//    frames the chip holds.  Frames end out of order and a slot is reused only when its own frame has ended, so with exactly
//    as many launches as fit, wave slots stand empty between a launch's end and the next launch on its slot; a queued launch
//    takes every workgroup slot the moment it frees (profiles/r05_schedule_sweep.txt: C5 4,134 -> 4,245 Msamples/s, its 1/2,
//    1/4, 1/8 shares 4,119 / 3,975 / 3,193 -> 4,223 / 4,101 / 3,814, C3 12,645 -> 12,851, C4's 1/8 share 12,157 -> 12,517, C2
//    13,051 -> 13,496; every (div, 2) measured beats its (div, 1); C4's 1/8 share, 3.2 tiles per wave: (1, 1) 12,195, (2, 2)
//    12,457, (4, 2) 12,185).
inline uint32_t width_mult_for(uint32_t div, uint32_t max_slots) { return (div >= 2u && 2u * div <= max_slots) ? 2u : 1u; }
inline void width_policy_start(WidthState& s, const WidthWorkload& w) {
    const uint32_t slots = width_max_u32(w.max_slots, 2u), narrowest = width_min_u32(kMaxWidthDiv, slots);
    const bool starved = !w.counter && w.spp >= 64u && (uint64_t)w.n_tiles < 2ull * w.n_waves && w.n_tiles > w.n_waves / narrowest;
    const bool short_chains = w.spp < 4u && (uint64_t)w.n_tiles * 4u >= 2ull * w.n_waves;
    s = WidthState();
    // (... a quarter for large scenes, whose pixels' chains differ 10 x: C5's 1/2 share 4,121 Msamples/s at a half x 2, 4,447 at a
    // quarter x 2; C5 and scenes of 1,297 to 4,901 spheres the same within 1 % either way: profiles/r05_schedule_sweep.txt)
    const uint32_t spare = (!scene_is_small(w.n_members) && slots >= 8u) ? 4u : 2u;
    s.div = starved ? narrowest : short_chains ? width_min_u32(4u, slots) : (!w.counter && w.n_tiles >= 3u * w.n_waves) ? spare : 1u;
    if (!short_chains) s.mult = width_mult_for(s.div, slots);
}

// A window has closed: ends a running trial (kept only if the rate rose by 3 %, else the previous setting returns and stays),
// then decides whether another one starts.  Below 0.90 one window is evidence enough (a pixel-starved share reads 0.4 to 0.8);
// between 0.90 and 0.95 a trial takes two consecutive windows (a window's utilisation scatters by a few per cent around the
// workload's own -- C3: 0.93 to 1.02 around 0.970); at 0.95 and above, or with no room left, the setting stays.
// Narrower only while a launch's waves still get at least two tiles each; else twice the frames in flight.
// (Round 5 also gave every well-utilised setting ONE exploratory trial of the next narrower width -- C4's 1/8 share reads 0.96
// at full width and renders 3 % more on a quarter of the waves, eight in flight.  Removed: a gain of 3 % cannot be told from
// the transient after the change of setting within a few dozen frames -- C3 was "measured" 4 % faster at a quarter width, where
// it renders 2 % less -- while the trials below decide on gains of 10 % and more.  Such settings are found offline instead:
// scripts/settle_schedules.py --sweep, profiles/schedules.json, mrt_set_schedule_hint.)
inline void width_policy_step(WidthState& s, const WidthWorkload& w, const WidthWindow& m) {
    uint32_t next_div = s.div, next_mult = s.mult;
    if (s.prev_div != 0u) {
        if (m.rate < 1.03 * s.prev_rate) { next_div = s.prev_div; next_mult = s.prev_mult; s.settled = 1u; }
        s.prev_div = 0u;
    }
    if (!s.settled) {
        const uint32_t in_flight = width_max_u32(2u, s.div) * s.mult;
        const uint32_t cand = s.div == 1u ? 4u : s.div * 2u;
        const bool can_narrow = cand <= width_min_u32(kMaxWidthDiv, w.max_slots) && (uint64_t)w.n_tiles * cand >= 2ull * w.n_waves && w.n_waves >= cand;
        const bool can_add = in_flight * 2u <= w.max_slots;
        if (m.util >= 0.90 && m.util < 0.95 && (can_narrow || can_add) && ++s.low_windows < 2u) {
            // measure again at the same setting
        } else if (m.util < 0.95 && (can_narrow || can_add)) {
            s.low_windows = 0u;
            s.prev_div = s.div;
            s.prev_mult = s.mult;
            s.prev_rate = m.rate;
            if (can_narrow) { next_div = cand; next_mult = width_mult_for(cand, w.max_slots); } else next_mult = s.mult * 2u;
        } else {
            s.settled = 1u;
        }
    }
    s.div = next_div;
    s.mult = next_mult;
}

// The share of the waves ONE launch gets.  The setting assumes the caller keeps its frames in flight; a caller that waits for
// every frame (a viewer that reads the framebuffer back, or gathers and presents, after each redraw) has the chip to itself
// and would run a single frame on 1 / div of it -- up to div pixels per lane in sequence, div times the latency.  So a launch
// is never narrower than the frames that really share the chip: those still queued or running when it is issued, plus itself.
inline uint32_t width_launch_div(uint32_t div, uint32_t frames_running) {
    return width_max_u32(1u, width_min_u32(div, frames_running + 1u));
}

// mrt_set_schedule_hint's range: div 1..8, mult 1..8, max(2, div) x mult frames within the slots a context has
inline bool width_hint_valid(uint32_t div, uint32_t mult) {
    return div >= 1u && div <= kMaxWidthDiv && mult >= 1u && mult <= 8u && width_max_u32(2u, div) * mult <= kMaxFrameSlots;
}

// The controller: the setting in force (s) and everything that decides when the policy above is asked.  One operation per
// concern of frames.cpp's schedule_frame, which calls them in this order for every frame of an adaptive launch: begin_workload,
// add_sample for what has landed, note_running, open_window, window_due / close_window, and -- when a setting first asks for
// more than two frames -- after_probe.  Every workload an operation takes gets ITS max_slots (capped()).
struct WidthController {
    WidthState s;                                   // div 0 = not chosen yet for the current workload
    uint32_t hint_div = 0, hint_mult = 0;           // mrt_set_schedule_hint: the caller's setting (0 = the controller decides)
    uint32_t max_slots = kMaxFrameSlots;            // frames that can really run side by side (frames.cpp, probe_max_slots)
    bool slots_probed = false;
    uint32_t last_launch_div = 1;                   // mrt_get_schedule: what the most recent launch was issued with
    uint32_t running_seen[kMaxFrameSlots] = {}, running_seen_n = 0;    // frames seen queued or running at the last calls
    uint32_t nothing_running_calls = 0;             // consecutive calls that found no earlier frame queued or running
    // Settled settings by workload, so that a change of samples per frame / scene / image and back does not start the trials
    // over.  (NOT what lets a viewer that moves its camera every frame reach a setting: every mrt_set_camera invalidates, the
    // restart below follows, and with a restart per frame no window ever opens -- such a caller stays at its start setting
    // unless the memo already knows the workload.  ADVICE.md, the item on the controller's edge cases; so is the memo's
    // growth without bound.)
    struct Memo { uint32_t n_tiles, spp, large, counter, n_spheres, div, mult; };
    std::vector<Memo> memo;
    uint64_t valid_from = 0;                        // frame_seq from which samples and timings belong to the current setting
    bool timing = false;                            // a measurement window is open: since frame t0_seq, at t0 seconds
    uint64_t t0_seq = 0;
    double t0 = 0.0;
    struct LaneStat { uint64_t seq = 0, hits = 0, slots = 0; bool valid = false; } base, last;

    // a new workload (image, shard, scene, camera, samples per frame, RNG mode): the next frame starts over
    void invalidate() { s.div = 0; }
    // the caller's setting, (0, 0) = none: the next frame takes it (or starts measuring again)
    void set_hint(uint32_t div, uint32_t mult) { hint_div = div; hint_mult = mult; invalidate(); }

    // Two counts of the frames in flight, on purpose: what a slot count is taken from is capped by the frames that really run
    // side by side (max_slots) -- the running window, the restart, the ring depth, mrt_get_schedule -- while a measurement
    // window's LENGTH is 2 x the setting's own max(2, div) x mult + 2 frames, uncapped (window_due).
    uint32_t frames_in_flight() const { return width_frames_in_flight(s.div, s.mult, max_slots); }
    // a setting asks for more than two frames and nobody has measured yet how many this process runs side by side
    bool wants_probe() const { return width_frames_in_flight(s.div, s.mult, kMaxFrameSlots) > 2u && !slots_probed; }

    // a new setting: the frames of the old one drain first; samples and timings count again from the THIRD generation of frames
    // at the new one (the first starts on an empty chip -- a change waits for everything in flight -- and the second still
    // inherits its convoys: judged on those, C3 read 4 % faster at a quarter width, where it renders 2 % less)
    void restart_measurement(uint64_t frame_seq) {
        timing = false;
        valid_from = frame_seq + 2u * frames_in_flight();
        base.valid = last.valid = false;
    }

    // The setting for a workload that has none (else nothing; returns whether it chose one): the hint, settled at once; else
    // what is known up front, or the setting this context has already settled at for the same workload, without trials.
    bool begin_workload(WidthWorkload w, uint64_t frame_seq) {
        if (s.div != 0) return false;
        w = capped(w);
        if (hint_div != 0) {
            s = WidthState();
            s.div = hint_div; s.mult = hint_mult; s.settled = 1u;
        } else {
            width_policy_start(s, w);
            for (const Memo& m : memo)
                if (same_workload(m, key(w))) { s.div = m.div; s.mult = m.mult; s.settled = 1u; }
        }
        restart_measurement(frame_seq);
        return true;
    }

    // How many frames the CALLER keeps in flight, given this call's count of earlier frames still queued or running: the most
    // seen over the last (frames in flight) calls -- not this call's count alone, which dips whenever a convoy of frames has just
    // ended (launched a little wider, the next frame then holds more of the chip and the dips feed on themselves: C5's 1/8 share
    // 3,066 -> 2,840 Msamples/s), and which is 0, 1, 2, ... while a burst of calls fills an empty pipeline.  A new setting starts
    // from "the caller keeps them all in flight".
    uint32_t note_running(uint64_t frame_seq, uint32_t running) {
        const uint32_t window = frames_in_flight();
        if (running_seen_n != window) {          // (a new setting, or the first call)
            running_seen_n = window;
            for (uint32_t i = 0; i < window; i++) running_seen[i] = window - 1u;
        }
        running_seen[frame_seq % window] = running;
        // ... except that NOTHING running at three calls in a row is a caller that waits for every frame (a pipeline that is
        // kept full never shows that): known at once, not after a window of up to sixteen slow frames
        nothing_running_calls = running == 0u ? nothing_running_calls + 1u : 0u;
        if (nothing_running_calls >= 3u)
            for (uint32_t i = 0; i < window; i++) running_seen[i] = 0u;
        uint32_t most = 0;
        for (uint32_t i = 0; i < window; i++) most = width_max_u32(most, running_seen[i]);
        return most;
    }

    // a lane-utilisation sample that has landed: the cumulative {world_hit calls, lane slots} after frame seq's render kernel
    void add_sample(uint64_t seq, uint64_t hits, uint64_t slots) {
        if (seq < valid_from) return;
        const LaneStat st{seq, hits, slots, true};
        if (!base.valid || st.seq < base.seq) base = st;
        if (!last.valid || st.seq > last.seq) last = st;
    }

    // A measurement window: from the first frame launched at the current setting with the pipeline full, over
    // 2 x (frames in flight) + 2 frames -- their lane utilisation (the samples) and, the calls being paced by the completions
    // (the caller's back-pressure), their rate -- and over at least 20 ms: frames of a fifth of a millisecond (C1, 1 spp) filled
    // a window in 2-3 ms of host time, whose jitter decided 1 trial in 9 the wrong way.
    bool open_window(uint64_t frame_seq, double now_s) {
        if (s.settled || timing || frame_seq < valid_from) return false;
        timing = true;
        t0_seq = frame_seq;
        t0 = now_s;
        return true;
    }
    bool window_due(uint64_t frame_seq, double now_s) const {
        return timing && frame_seq >= t0_seq + 2u * (width_max_u32(2u, s.div) * s.mult) + 2u && now_s - t0 >= 0.020 && base.valid &&
               last.valid && last.seq > base.seq && last.slots > base.slots && last.hits >= base.hits;
    }
    // Closes the window that is due: what it measured goes to the policy, a settled setting into the memo, and the measurement
    // starts over.  The frame rate is the host's -- the calls since the window opened over the time they took -- unless the
    // caller has at least max(2, frame_slots / 2) start-to-start intervals (n of them, sum_ms in all) of frames on the same slot
    // on the DEVICE's clock.  Frames END in convoys (the launches that share the chip start together), so a count of the calls
    // the completions let through over a window of a few convoys is off by up to a convoy -- 4 frames in 18, far beyond the 3 %
    // a trial is judged by (the first cut kept a quarter width for C3 that renders 8 % less).  Every frame slot is refilled the
    // moment its frame ends, so slots / (a slot's start-to-start time) is the rate (Little's law).
    WidthWindow close_window(WidthWorkload w, uint64_t frame_seq, double now_s, uint32_t frame_slots, uint32_t n, double sum_ms) {
        w = capped(w);
        WidthWindow m;
        m.util = (double)(last.hits - base.hits) / (double)(last.slots - base.slots);
        const double dt = now_s - t0;
        m.rate = (double)(frame_seq - t0_seq) / (dt > 1e-9 ? dt : 1e-9);
        if (n >= width_max_u32(2u, frame_slots / 2u)) m.rate = (double)frame_slots * 1e3 * (double)n / sum_ms;
        width_policy_step(s, w, m);
        if (s.settled) {
            Memo now_known = key(w);
            now_known.div = s.div; now_known.mult = s.mult;
            bool known = false;
            for (Memo& e : memo)
                if (same_workload(e, now_known)) { e = now_known; known = true; }
            if (!known) memo.push_back(now_known);
        }
        restart_measurement(frame_seq);
        return m;
    }

    // The probe has measured how many frames really run side by side: more than two in flight only within that.  Without a
    // hint the workload starts over within what the process can do (a pinned setting keeps its width and is held to the frames
    // that run side by side all the same: sixteen frames on fewer queues take turns -- C5's 1/8 share 2,790 Msamples/s, less
    // than eight in flight give).
    void after_probe(uint32_t cap, WidthWorkload w, uint64_t frame_seq) {
        max_slots = cap;
        slots_probed = true;
        if (max_slots < kMaxFrameSlots && hint_div == 0) {
            width_policy_start(s, capped(w));
            restart_measurement(frame_seq);
        }
        running_seen_n = 0;
    }

    // the share of the waves the frame about to be launched gets (width_launch_div), remembered for mrt_get_schedule and for
    // the subset frames, which are launched at the width of the controller's last launch
    uint32_t launch_div(uint32_t frames_running) { return last_launch_div = width_launch_div(s.div, frames_running); }

private:
    WidthWorkload capped(WidthWorkload w) const { w.max_slots = max_slots; return w; }
    static Memo key(const WidthWorkload& w) { return Memo{w.n_tiles, w.spp, scene_is_small(w.n_members) ? 0u : 1u, w.counter, w.n_spheres, 0u, 0u}; }
    static bool same_workload(const Memo& a, const Memo& b) {
        return a.n_tiles == b.n_tiles && a.spp == b.spp && a.large == b.large && a.counter == b.counter && a.n_spheres == b.n_spheres;
    }
};

}  // namespace mrt
