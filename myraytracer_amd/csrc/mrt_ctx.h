// Host-side state behind the opaque mrt_ctx of include/myraytracer_amd.h, and what the host files share: api.cpp (life cycle,
// buffers, read-backs), world.cpp (the scene), frames.cpp (the frame loop), present.cpp, noise.cpp, denoise.cpp and multi_gpu.cpp
// (the gather).  Internal: not installed.
#pragma once
#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "mrt_internal.h"
#include "width_policy.h"

namespace mrt {
// free device / pinned allocations (those there are) and forget them
template <typename... T> void free_device(T*&... p) { ((p ? (void)hipFree(p) : (void)0, p = nullptr), ...); }
template <typename T> void free_pinned(T*& p) { if (p) (void)hipHostFree(p); p = nullptr; }

// The filter's buffers (denoise.cpp), a float4 per pixel each, in the order they are allocated: ping, pong and the denoised frame;
// with temporal reprojection on also the history, H0 and H1 of pair 0 and of pair 1; with its response on as well the fast
// history, H2 of pair 0 and of pair 1.  The only place that knows which index is what.
struct DenoiseBuffers {
    float* buf[9] = {};
    float* ping() const { return buf[0]; }
    float* pong() const { return buf[1]; }
    float* out() const { return buf[2]; }
    float* h0(uint32_t pair) const { return buf[3 + 2 * pair]; }
    float* h1(uint32_t pair) const { return buf[4 + 2 * pair]; }
    float* h2(uint32_t pair) const { return buf[7 + pair]; }
    // how many of them a denoise needs: buf[0, wanted), allocated in this order
    static size_t wanted(bool temporal_on, bool response_on) { return !temporal_on ? 3 : response_on ? 9 : 7; }
    bool have_filter() const { return buf[0] && buf[1] && buf[2]; }
    // all / any of the history's four (fast: of the fast history's two); all that a step needs
    bool all_history(bool fast) const { return fast ? buf[7] && buf[8] : buf[3] && buf[4] && buf[5] && buf[6]; }
    bool any_history(bool fast) const { return fast ? buf[7] || buf[8] : buf[3] || buf[4] || buf[5] || buf[6]; }
    bool have_history(bool response_on) const { return all_history(false) && (!response_on || all_history(true)); }
    void free_history() { free_device(buf[3], buf[4], buf[5], buf[6], buf[7], buf[8]); }
    void free_all() { free_device(buf[0], buf[1], buf[2]); free_history(); }
};

// What mrt_present shows and the float read-backs return: one definition per source (denoise.cpp: source_check, source_queue;
// present.cpp: the flag bits).  Accumulated and Gathered are present-only in this table: their read-backs, mrt_read_framebuffer
// and mrt_read_gathered, deal with shards and packed rows (read_rows), which the other four never see.  View: the current
// diagnostic view (mrt_ctx::view), computed into den.out() as a denoise is.
enum class ImageSource { Accumulated, Gathered, Denoised, Temporal, GatheredDenoised, View };
// a source's image once queued: `rows` rows of the image's width, and the frame count the image shows
struct SourceImage { const float* img; uint32_t rows, frames_done; };
}  // namespace mrt

struct mrt_ctx {
    int device = 0;
    mrt_args args{};
    uint64_t seed = 0;
    mrt_locals locals{};
    uint32_t frames_done = 0;          // State::sample_count (lib.rs:213, 300)

    uint32_t shard_rank = 0, shard_world = 1;
    uint32_t local_bands = 0;

    mrt_world world{};
    bool have_world = false;
    uint32_t n_spheres = 0, n_padded = 0;
    mrt_camera_raw cam_raw{};

    // device memory (all owned)
    mrt::SphereRec* d_spheres = nullptr;
    mrt::SphereRec* d_clusters = nullptr;  // bounding spheres the sweep tests (up to kClusterK spheres each)
    uint16_t* d_top_mfma = nullptr;        // the top-level records as the MFMA A operand (build_top_mfma)
    bool mfma_scene_ok = false;            // the expanded test's extra slack is negligible for this scene
    double mfma_r2_ref = 0.0;              // median R^2 of the top level (camera check at launch)
    float mfma_origin[3] = {0.0f, 0.0f, 0.0f};   // the matrix-core sweep works in coordinates relative to this point
    double mfma_reach = 0.0;                      // max over ALL spheres of |centre - mfma_origin| + |radius|: no hit point lies further out
    // the sweep's space: x' = mfma_axis (x - mfma_origin) per component, entries 1, 2 or 4 (hierarchy.cpp, build_sweep_operand);
    // mfma_r2_ref and mfma_reach are measured there.  force_axis: the next scene's D is the caller's (mrt_debug_set_sweep_axes)
    float mfma_axis[3] = {1.0f, 1.0f, 1.0f};
    float force_axis[3] = {1.0f, 1.0f, 1.0f};
    bool have_force_axis = false;
    int sweep_mode = 0;                    // 0 automatic, 1 SGPR-fed VALU sweep, 2 matrix-core sweep (mrt_debug_set_sweep)
    float* d_shade = nullptr;              // 8 floats per sphere: centre, radius, material colour, fuzz | ior
    mrt::SphereRec* d_nodes = nullptr;     // hierarchy levels below the top: members (kClusterK per cluster), clusters, ...
    uint32_t* d_member_index = nullptr;    // their indices in the reference's sphere order
    // mrt_regroup_spheres (regroup.hip): the scene's regroup scratch (regroup_layout: the pool list, rank -> cluster, pref, two
    // orders, the segments' boxes, the sort's keys), the clusters made from the builder's pool and the spheres in them; the block
    // the next regroup uses (mrt_debug_set_regroup_block; 0 = kRegroupBlock) and what the last one did (mrt_debug_regroup_info)
    uint32_t* d_regroup = nullptr;
    uint32_t n_pool = 0, n_pooled = 0;
    uint32_t regroup_block = 0, regroup_last[3] = {0, 0, 0};
    // the auto-regroup policy (mrt_set_auto_regroup; regroup_policy.hip): the setting, which outlives the scene; the words of
    // d_regroup (0: the stub of a scene without a pool), whose last ones are the policy's RegroupState; the scene's successful
    // non-empty mrt_update_spheres calls since the policy or the scene was set (every check_every-th of them checks)
    mrt_auto_regroup auto_regroup = mrt::auto_regroup_defaults();
    size_t regroup_words = 0;
    uint32_t auto_updates = 0;
    // Camera-ray cluster masks (cam_mask.hip; frames.cpp, camera_masks): a scene buffer (mrt_set_world_raw makes it for a small
    // scene of at most kCamMaskRecords top records, all ones, sized for the shard as it is then; free_world frees it) of
    // cam_mask_entries entries of 4 words.  ONE staleness generation, bumped by everything the masks depend on (scene, camera,
    // geometry updates, regroups, image shape and shard); cam_mask_built: the generation the table holds (0: none yet),
    // cam_mask_seen: the generation the previous frame was launched under (a generation that survives a frame is worth a
    // build).  cam_masks_on: mrt_debug_set_camera_masks; cam_masks_in_force: the most recent render launch got the table.
    // The camera-ray sphere lists (4 words an entry, the same entries) are the second half of the same buffer -- cam_lists() --
    // written by the same build: one allocation, one generation, one switch.  A launch the tables apply to gets one of the two
    // (cam_prefer below).
    uint32_t* d_cam_masks = nullptr;
    size_t cam_mask_entries = 0;
    uint32_t* cam_lists() const { return d_cam_masks ? d_cam_masks + 4 * cam_mask_entries : nullptr; }
    uint64_t cam_mask_gen = 1, cam_mask_built = 0, cam_mask_seen = 0;
    bool cam_masks_on = true, cam_masks_in_force = false;
    // which of the two tables a launch gets (frames.cpp, camera_masks): cam_prefer 0 = the library's rule (the lists where the
    // launch has the pixels to be bound by throughput, the masks where it is bound by its longest pixel chains), 1 = the lists,
    // 2 = the masks (mrt_debug_set_camera_masks 1 / 2 / 3); cam_lists_in_force: the most recent render launch got the lists.
    uint32_t cam_prefer = 0;
    bool cam_lists_in_force = false;
    // The build runs on the side stream of the frame that needs it, and EVERY frame slot builds the table on its own stream before
    // its first frame of a generation (FrameSlot::cam_built): a slot's frames follow that slot's build in stream order, no stream
    // ever waits for another one's build, and the frames in flight are not held back.  The builds of one generation write the
    // same words.  cam_mask_built is the generation some slot has built.
    // large scenes' walk: the axis-aligned boxes of the hierarchy's nodes in the kernel's top-down numbering (KParams::boxes),
    // and the same array with every real box opened wide (a box test that never rejects: mrt_debug_set_boxes(0))
    mrt::BoxRec* d_boxes = nullptr;
    mrt::BoxRec* d_boxes_open = nullptr;
    uint32_t box_cluster_first = 0, box_cluster_parent_first = 0;
    bool box_quad = false;
    float box_kc = 0.0f;
    int boxes_mode = 1;                    // mrt_debug_set_boxes: 0 = the boxes never reject (diagnostic), 1 / 2 = they do
    float cluster_factor = 8.0f;           // grow a cluster while its enclosing radius <= factor * largest member radius
    // hierarchy depth rule (build_hierarchy): levels are added while the top has more than top_target records; 0 = automatic
    // (256, or 128 for scenes whose walk tests boxes)
    uint32_t max_levels = mrt::kMaxLevels, top_target = 0;
    uint32_t levels = 1, n_nodes = 0, n_members = 0;
    uint32_t level_base[mrt::kMaxLevels] = {0, 0, 0, 0};
    uint32_t n_direct = 0, direct_first = 0;
    mrt::SphereRec direct[mrt::kMaxDirect] = {};
    uint32_t direct_index[mrt::kMaxDirect] = {};
    float* d_vec4 = nullptr;
    float* d_f32 = nullptr;
    int32_t* d_i32 = nullptr;
    uint32_t* d_seeds = nullptr;
    float* d_fb[2] = {nullptr, nullptr};   // [target, secondary] ping-pong (lib.rs:505-543)
    int target = 0;                        // index of the buffer the NEXT redraw writes
    unsigned long long* d_counters = nullptr;
    bool count_draws = true;               // mrt_set_draw_counting
    uint32_t last_launch[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};   // mrt_debug_last_launch: the last render / pilot instantiation
    // Up to frame_slots frames may be in flight: frame n's render kernel (sort, pilot) runs on side
    // stream n % frame_slots and only its finalize pass -- the one step that needs frame n-1's framebuffer -- runs
    // on the caller's stream.  The next frame's heavy tiles thus start while this frame's last
    // pixels drain (a pixel is one sequential chain, so every frame ends on a thinning chip).
    // How many: 2 for launches that fill the chip (re-measured in round 2, LDS-free sort: C3 9,799 / 9,709 / 9,380 Msamples/s
    // with 2 / 3 / 4).  A PIXEL-STARVED shard (fewer than two pixels per resident lane, long sample chains: an 8-GPU share of
    // C5) is different: its launch is as long as its heaviest pixel's chain while most of its waves end much earlier, and a
    // wave instruction costs the same with 40 % of its lanes active as with all -- so it runs more frames at once, each on
    // fewer, better packed waves (redraw_frames; round 4).  frame_slots is the count in use, slot[] the capacity.
    static constexpr uint32_t kMaxFrameSlots = mrt::kMaxFrameSlots;
    uint32_t frame_slots = 2;
    uint32_t last_slot = 0;                         // the slot of the most recent redraw
    int frame_slots_override = 0;                   // mrt_debug_set_frames_in_flight: 0 = automatic
    struct FrameSlot {
        hipStream_t stream = nullptr;
        hipEvent_t render_done = nullptr, finalize_done = nullptr;
        void* d_pix_acc = nullptr;             // per-pixel (x per-block, counter mode) colour sums + costs, render -> finalize
        size_t pix_acc_layers = 0;             // capacity in layers of local_texels entries
        uint32_t cost_first_layer = 0, cost_layers = 1;   // the layers holding the slot's most recent frame
        uint32_t* d_tile_cost = nullptr;       // written by this slot's finalize, orders its next queue
        uint32_t* d_tile_order = nullptr;
        uint32_t* d_sort_scratch = nullptr;    // 1024 u32 of sort workspace + the queue counter
        bool cost_valid = false;               // d_tile_cost holds a usable estimate for the current scene
        // The tile queue's counter is left at zero by every finalize pass of the slot.  If anything between a render launch
        // and its last finalize launch fails, it is not: the next launch on this slot resets it itself.
        bool queue_dirty = false;
        // launch-width controller: the context's cumulative {world_hit calls, lane slots} copied to pinned host memory right
        // after this slot's render kernel (h_stats[3 slot ..]: counters 1 .. 3 in one copy), the event that says the copy has landed, the frame it was
        hipEvent_t stats_ready = nullptr;
        uint64_t stats_seq = 0;
        bool stats_pending = false;
        bool render_pending = false;           // a render kernel of this slot has been launched and not yet been seen complete
        // camera masks: the generation this slot's stream has built the table for; the generation the slot's most recent frame
        // reads it under (0: none), and whether an earlier frame of the slot that may still run reads an older one -- a build
        // for a new generation on another slot's stream waits for such frames first
        uint64_t cam_built = 0, cam_used_gen = 0;
        bool cam_stale_reader = false;
        uint64_t render_seq = 0;               // its frame (diagnostics of a stalled wait)
        // adaptive sampling: a subset frame's tile list, written by the host into pinned memory and copied on the slot's stream
        // before the render (the host rewrites it only after the slot's previous render kernel has completed)
        uint32_t* h_tile_list = nullptr;
        uint32_t* d_tile_list = nullptr;
        // mrt_debug_read_tile_schedule: how the queue of the slot's most recent render launch was ordered (MRT_TILE_ORDER_*),
        // its length, and whether a pilot launch preceded it.  Written by the launch functions, read by the diagnostic alone.
        uint32_t order_kind = 0, order_n = 0;
        bool order_pilot = false;
    } slot[kMaxFrameSlots];
    // Launch width (redraw_frames; the policy and the controller: width_policy.h): a frame is launched on 1 / width.s.div of the
    // persistent waves the chip holds and max(2, width.s.div) x width.s.mult frames are in flight, so that the chip stays full.  Narrow launches
    // pack the lanes better (more pixels per lane in sequence: the launch's tail, in which lanes idle until their wave's longest
    // pixel ends, is the same length but a smaller share) at the price of a longer frame latency -- and they do not always pay
    // (C3 / C4, 0.98 / 0.99 lane utilisation at full width, lose 1-4 % at a half; C2 loses 4 % at a half and gains 18 % at a
    // quarter).  So the setting is MEASURED: trials while the utilisation is low, kept only if the frame rate rises by 3 %.
    // Scheduling only: the images do not change.
    // All of the controller's state, the memo of settled settings included (which does NOT let a viewer that moves its camera
    // every frame reach a setting: see the comment above WidthController::Memo, and ADVICE.md).
    mrt::WidthController width;
    unsigned long long dbg_world_hit_stats[2] = {0, 0};     // mrt_debug_world_hit_stats
    unsigned long long* h_stats = nullptr;          // pinned, 3 x kMaxFrameSlots (+ 2 x kMaxFrameSlots: the concurrency probe's stamps)
    uint32_t hold_polls = 0;                        // mrt_debug_hold: the polls its most recent kernel was given (its stamps: the probe's last pair)
    hipEvent_t ev_inputs = nullptr;            // scene / seeds uploads on the caller's stream
    bool inputs_dirty = true;
    uint64_t frame_seq = 0;
    uint32_t tiles_x = 0, n_tiles = 0, n_waves = 0, cus = 0;
    uint32_t pilot_spp = 2;
    int waves_per_cu_override = 0;
    bool lpt_enabled = true;
    static constexpr uint32_t kWaveLogFrames = 32;
    unsigned long long* d_wave_log = nullptr;   // diagnostic, see mrt_debug_wave_log: a ring of kWaveLogFrames frames' logs
    size_t wave_log_waves = 0;

    // multi-GPU gather (multi_gpu.cpp): on the root, the full frame assembled from every shard's bands
    // (total_bands_padded x 8 rows x W RGBA32F, row 0 = bottom) and, for the RCCL variant, the rank-major
    // receive staging; ev_gather marks "this shard's bands have been copied out" on its stream
    float* d_gather = nullptr;
    float* d_gather_stage = nullptr;
    size_t gather_bytes = 0, gather_stage_bytes = 0;
    hipEvent_t ev_gather = nullptr;
    // on the root: "everything queued on the root's stream before this gather" -- a reader of the previous frame's
    // d_gather among it -- which every shard's stream waits for before it overwrites d_gather (write-after-read)
    hipEvent_t ev_gather_root = nullptr;
    bool gather_per_band = false;              // mrt_debug_set_gather_per_band: the cross-device copy loop on one device
    // the noise estimate across shards (mrt_set_gather_noise): with the setting on a gather also assembles the full-frame S,
    // height x width floats in the SAME allocation right behind the colour (gathered_noise()), and records the root's K and
    // frame count as they are then -- what mrt_read_gathered_denoised filters with, whatever the root renders afterwards.
    // gather_has_s: the latest gather carried S and nothing since (mrt_set_shard, a toggle of the setting) took it away.
    bool gather_noise = false, gather_has_s = false;
    double gather_k = 0.0;
    uint32_t gather_frames = 0;

    // present pass (mrt_present, present.cpp): a ring of images, each the present kernel's output on the device, its copy in pinned
    // host memory and the event that says the copy has landed.  An entry is free, queued (presented, not acquired: its copy may
    // still be in flight) or held by the caller (mrt_present_acquire); entries are added, never freed before mrt_destroy.
    struct PresentEntry {
        uint8_t* d_img = nullptr;
        uint8_t* h_img = nullptr;
        hipEvent_t copied = nullptr;
        enum { kFree, kQueued, kHeld } state = kFree;
        mrt_present_info info{};
    };
    std::vector<PresentEntry> present_ring;
    size_t present_entry_bytes = 0;                 // the capacity of every entry
    uint32_t present_depth_pin = 0;                 // mrt_set_present_ring: 0 = automatic
    uint32_t present_depth = 0;                     // the entries in use: present_ring[0, present_depth)
    uint64_t present_seq = 0;
    uint32_t present_dropped = 0;                   // since the last acquire
    int present_copy_mode = 1;                      // mrt_debug_set_present_copy: 0 = own stream, 1 = the ctx's stream (measured)
    hipStream_t present_stream = nullptr;           // the copies (mode 0), created at the first present in that mode
    hipEvent_t ev_presented = nullptr;              // "the present kernel is done", on the ctx's stream (mode 0)
    float* d_present_tables = nullptr;              // present_thresholds() on the device

    // noise estimate (mrt_set_noise_tracking / mrt_noise_query, noise.cpp): S, updated by every blend while tracking is on; the
    // reduction's scratch and tile map; a ring of reports, each the reduction's sums on the device, their copy in pinned host
    // memory and the event that says the copy has landed.  Entry seq % kNoiseRing holds query seq.
    static constexpr uint32_t kNoiseRing = 8;
    struct NoiseEntry {
        hipEvent_t copied = nullptr;
        mrt_noise_report report{};                  // what the host knows at query time (seq, frames_done, K, threshold, floor)
        bool per_tile = false;                      // reduced with K per tile (adaptive sampling): the sums' sum_s is sum_var
        // mrt_noise_query_budget: the entry carries a plan (budget.hip; k_t and the result beside the entry's map, finished when
        // `copied` fires), and n_q, the frame counts the plan was allocated for: every tile's nq_uniform while the accumulation
        // was uniform at the query (nq empty), else nq per tile
        bool has_plan = false;
        uint32_t nq_uniform = 0;
        std::vector<uint32_t> nq;
    };
    bool noise_on = false;                          // mrt_set_noise_tracking
    float* d_noise_s = nullptr;                     // local texels (allocated with the framebuffers while noise_on)
    double noise_c2 = 1.0;                          // sum of the squared normalised weights of the frames blended so far
    void* d_noise_partials = nullptr;
    // kNoiseRing x n_tiles: query seq's map at entry seq % kNoiseRing; behind the maps the entries' budget plans and the
    // selection's scratch (mrt::budget_layout, mrt_internal.h)
    float* d_noise_tiles = nullptr;
    mrt::NoiseSums* d_noise_sums = nullptr;         // kNoiseRing entries
    mrt::NoiseSums* h_noise_sums = nullptr;         // pinned, kNoiseRing entries
    NoiseEntry noise_ring[kNoiseRing];
    uint64_t noise_seq = 0;                         // queries so far
    uint64_t noise_first = 1;                       // the oldest query whose report may still be returned (mrt_reset)
    hipStream_t noise_stream = nullptr;             // mrt_read_noise_tiles' copy, created on first use

    // denoiser (mrt_read_denoised / MRT_PRESENT_DENOISED, denoise.cpp; denoise.hip): the parameters, the first-hit guides of the
    // current camera and scene (width x height pixels, y * width + x; rebuilt on the ctx's stream at the next denoise after
    // mrt_set_camera / mrt_set_world* / mrt_set_shard mark them stale) and the filter's buffers, all allocated at the first use
    mrt_denoise_params denoise = mrt::denoise_defaults();
    uint32_t denoise_var_mode = MRT_DENOISE_VAR_ACCUMULATED;   // mrt_set_denoise_variance: where the luminance stop's variance comes from
    uint32_t denoise_spatial_frames = 3;                       // SPATIAL_EARLY: the spatial estimate while frames_done < this
    bool denoise_adaptive = false;                  // mrt_set_denoise_adaptive: a diverged accumulation is filtered per tile, not refused
    mrt_denoise_mix denoise_mix = mrt::denoise_mix_defaults();  // mrt_set_denoise_mix: the blend behind every denoise of an accumulation
    mrt_view view = mrt::view_defaults();           // mrt_set_view: what mrt_read_view / MRT_PRESENT_VIEW compute (views.hip)
    bool guides_stale = true;
    float* d_guide_rays = nullptr;                  // 6 floats per pixel
    int32_t* d_guide_hits = nullptr;                // {sphere | -1, bits of t} per pixel (the DBG render kernel's output)
    // the DBG kernel's candidate bitmap, which nothing reads: one word per pixel + one per 32 spheres, every pixel's row starting
    // one word after the previous pixel's (dbg_words = 1) -- a full bitmap would be ceil(spheres / 32) words per pixel
    uint32_t* d_guide_cand = nullptr;
    size_t guide_cand_words = 0;
    uint32_t* d_guide_queue = nullptr;              // the DBG launch's tile queue counter
    float* d_guides = nullptr;                      // 2 float4 per pixel
    mrt::DenoiseBuffers den;                        // the filter's buffers and the temporal history's

    // temporal reprojection (mrt_set_temporal / mrt_temporal_step / mrt_read_temporal, denoise.cpp; temporal.hip): the history
    // the next step reads is pair temporal_cur (den.h0(cur), den.h1(cur)), the step writes the other pair and swaps.
    // temporal_clear: the pair to read holds nothing valid (just allocated, or the history was dropped): the next step
    // zeroes its H0 first.  temporal_stepped: a step since then (what the reads need).  "Previous": the spheres' (cx, cy, cz, r)
    // at the last step, a scene buffer (mrt_set_world_raw makes it, free_world frees it), and the derived camera.
    bool temporal_on = false;
    mrt_temporal_params temporal = mrt::temporal_defaults();
    uint32_t temporal_cur = 0;
    bool temporal_clear = true, temporal_stepped = false;
    float* d_prev_xyzr = nullptr;
    mrt_camera_raw temporal_prev_cam{};
    // the response (mrt_set_temporal_response): the fast history H2 of pair p is den.h2(p); zeroed with H0 where the history
    // was dropped
    mrt_temporal_response temporal_response = mrt::temporal_response_defaults();

    // adaptive sampling (mrt_render_tiles / mrt_render_adaptive, frames.cpp / noise.cpp; adaptive.hip): every tile's frame count n_t.  Until the
    // first subset frame every n_t is frames_done and nothing differs from a uniform accumulation.  From it on (tiles_diverged,
    // until mrt_reset) every blend is per tile (launch_tile_blend) and IN PLACE on d_fb[target ^ 1] (target no longer swaps), and
    // noise reports take K per tile from the tables K(n) = mrt_noise_factor(n, max_w), n < k_len, grown on demand.
    bool tiles_diverged = false;
    std::vector<uint32_t> tile_frames;              // the host's copy of n_t (what the blends queued so far make it)
    uint32_t* d_tile_frames = nullptr;              // n_t per tile, incremented by the per-tile blend
    std::vector<double> k_table;                    // K(n) for n < k_table.size(), and c2 after k_table.size() frames
    double k_c2 = 1.0;
    float* d_k_f32 = nullptr;                       // K(n) as float / double on the device, k_len entries
    double* d_k_f64 = nullptr;
    uint32_t k_len = 0;
    std::vector<float> h_select_map;                // mrt_render_adaptive: the report's tile map
    std::vector<uint32_t> selection;                // ... and the tiles it selects
    std::vector<uint32_t> h_plan;                   // mrt_read_budget_plan / mrt_render_planned: a report's result and k_t

    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // ring of HIP event pairs around the render kernel of the most recent redraws, frame f at f % kEventRing
    static constexpr uint32_t kEventRing = 64;
    hipEvent_t ev_start[kEventRing] = {}, ev_stop[kEventRing] = {};

    bool shuffle_overridden = false;       // mrt_set_rng_shuffle since the last frame
    bool batch_frames = true;              // mrt_render may render several frames per launch (mrt_debug_set_frame_batching)
    int batch_form = 0;                    // 0 automatic, 1 always "a lane keeps its pixel for the batch's frames", 2 always queue layers
    float set_world_ms = 0.0f;             // host time of the last scene upload (hierarchy build + copies)

    // Every blocking host wait of the library polls with this deadline (seconds; 0 = no deadline) and fails with
    // MRT_ERR_STALLED, naming the wait, instead of hanging (mrt_set_wait_timeout).  A context that has stalled once stays
    // failed: its queued work may never finish, so mrt_destroy then releases what it can without waiting.
    double wait_timeout_s = 120.0;
    bool stalled = false;

    std::string err;
};

namespace mrt {

// records the message behind mrt_last_error (ctx == NULL: the thread's global message) and returns `status`
int fail(mrt_ctx* ctx, int status, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

inline uint32_t total_bands(uint32_t height) { return (height + kBandRows - 1) / kBandRows; }
inline size_t local_texels(const mrt_ctx* c) { return (size_t)c->local_bands * kBandRows * c->args.width; }
// ... at least 1: the size of an allocation that an empty shard makes all the same
inline size_t local_texels_min1(const mrt_ctx* c) { return local_texels(c) ? local_texels(c) : 1; }
inline uint32_t tiles_min1(const mrt_ctx* c) { return c->n_tiles ? c->n_tiles : 1; }
// the largest n_t of the host's tile map (0 without one): what sizes the K table of a per-tile report, plan or denoise
inline uint32_t most_tile_frames(const mrt_ctx* c) {
    uint32_t most = 0;
    for (uint32_t t : c->tile_frames) most = t > most ? t : most;
    return most;
}
// the oldest noise report still held: not before the last reset, and the ring keeps the newest kNoiseRing
inline uint64_t oldest_noise_report(const mrt_ctx* c) {
    const uint64_t in_ring = c->noise_seq >= mrt_ctx::kNoiseRing ? c->noise_seq - mrt_ctx::kNoiseRing + 1 : 1;
    return c->noise_first > in_ring ? c->noise_first : in_ring;
}
// the root's gathered frame (multi_gpu.cpp): the colour's bytes -- every shard's bands, padding included -- and S behind them
inline size_t gathered_colour_bytes(const mrt_ctx* c) { return local_texels(c) * c->shard_world * 4 * sizeof(float); }
inline float* gathered_noise(const mrt_ctx* c) { return c->d_gather + gathered_colour_bytes(c) / sizeof(float); }

// Bounded host waits (api.cpp): poll the event / stream until it is complete or the context's deadline has passed; `what`
// names the wait in the error message.  Return an mrt_status.
int wait_event(mrt_ctx* c, hipEvent_t ev, const char* what);
int wait_stream(mrt_ctx* c, hipStream_t s, const char* what);
// everything this context has in flight: the side streams, then the caller's stream
int wait_all(mrt_ctx* c, const char* what);

// What one host file defines and another calls.  api.cpp: the buffers of shard `rank` of `world` allocated and, only once all of
// them exist, put in the place of the current shard's (a failure leaves the context as it was); the scene's arrays released;
// a slot's first layer of colour sums, zeroed on the ctx's stream; the tail of a read-back of this shard's texels (`who`: the entry
// point, for the messages) -- capacity check, the full bottom-up image when shard_world == 1 else the packed rows, bounded wait
int alloc_frame_buffers(mrt_ctx* c, uint32_t rank, uint32_t world);
void free_world(mrt_ctx* c);
int alloc_first_colour_sums(mrt_ctx* c, mrt_ctx::FrameSlot& S);
int read_rows(mrt_ctx* c, const char* who, const void* src, void* out, size_t cap, size_t texel_bytes);
// world.cpp: the scene / hierarchy / sweep-variant part of the kernel arguments
void fill_scene_params(const mrt_ctx* c, KParams& p);
// frames.cpp: the side stream of a frame slot and its events; adaptive sampling's per-tile state, released
int create_slot_streams(mrt_ctx* c, mrt_ctx::FrameSlot& S);
void free_tile_frames(mrt_ctx* c);
// noise.cpp: noise tracking's per-texel buffers, sized like the framebuffers; the same three for a shard of `local_bands` bands
// into the caller's pointers (all of them or, on a failure, none)
void free_noise_buffers(mrt_ctx* c);
int alloc_noise_buffers(mrt_ctx* c);
int alloc_noise_set(mrt_ctx* c, uint32_t local_bands, float** s, float** tiles, void** partials);
// ... and adaptive sampling's device tables K(n), n < k_len, grown to at least `len` entries (a per-tile noise report's and a
// per-tile denoise's: both read d_k_f32 on the ctx's stream, which is drained once before a larger table replaces the old one)
int ensure_k_table(mrt_ctx* c, uint32_t len);
// denoise.cpp: the denoiser's buffers released; the temporal history dropped (mrt_set_world*, mrt_set_shard: nothing queued,
// nothing freed)
void free_denoise_buffers(mrt_ctx* c);
void drop_temporal_history(mrt_ctx* c);
// ... and the image sources, for mrt_present and the float read-backs.  source_check: the refusals of the state, before any
// runtime call (`who`: the entry point, for the messages); source_rows: a shard's own accumulation is its packed rows;
// source_queue: what the source needs queued on the ctx's stream (nothing, or the guides where stale and a filter), and the result
int source_check(mrt_ctx* c, ImageSource source, const char* who);
inline uint32_t source_rows(const mrt_ctx* c, ImageSource source) {
    return source == ImageSource::Accumulated && c->shard_world > 1 ? c->local_bands * kBandRows : c->args.height;
}
int source_queue(mrt_ctx* c, ImageSource source, SourceImage* out);
// multi_gpu.cpp: is there a gathered S -- MRT_ERR_STATE before the first gather and when the latest carried none
int gathered_noise_check(mrt_ctx* R, const char* who);

}  // namespace mrt

#define MRT_TRY(expr)                      \
    do {                                   \
        const int st_ = (expr);            \
        if (st_ != MRT_OK) return st_;     \
    } while (0)

// a chain of HIP calls that stops at the first failure (`e`) and remembers which call that was (`what`), for a function that
// has scratch buffers to release before it reports: fail(ctx, MRT_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e))
#define HIP_CHAIN(e, what, expr)                        \
    do {                                                \
        if ((e) == hipSuccess) {                        \
            (e) = (expr);                               \
            if ((e) != hipSuccess) (what) = #expr;      \
        }                                               \
    } while (0)

#define HIP_TRY(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return mrt::fail(ctx, MRT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
