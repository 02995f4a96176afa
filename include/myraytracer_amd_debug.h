/*
 * myraytracer_amd_debug.h -- diagnostic and tuning entry points of libmyraytracer_amd.so.
 *
 * NOT part of the drop-in boundary: nothing here maps to a seam of the reference (raytracer/src/lib.rs has no
 * counterpart for any of it).  The product header is myraytracer_amd.h; this one exists for the parity tests
 * (candidate sets of the sweep + walk, the hand-rolled division / square root against hipcc's, hierarchy
 * inspection) and for the A/B switches the measurements in DESIGN_HISTORY.md were taken with.  The symbols are
 * exported by the same library; tests/test_abi.py checks both headers against it.
 */
#ifndef MYRAYTRACER_AMD_DEBUG_H
#define MYRAYTRACER_AMD_DEBUG_H

#include "myraytracer_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic, host only: the thresholds the present pass searches (mrt_present): out[k], k = 1..255, is the smallest float v
 * with mrt_srgb8(v) >= k; out[0] = -inf.  A value's code is the number of out[1..255] that are <= it (0 for NaN). */
int mrt_debug_srgb8_thresholds(float out[256]);
/* Diagnostic: the present kernel on caller-supplied texels, synchronously: rgba = rows x width RGBA32F texels (row 0 first),
 * out = rows x width x 4 bytes; format MRT_PRESENT_*_SRGB, flags 0 or MRT_PRESENT_FLIP_Y. */
int mrt_debug_present_encode(mrt_ctx* ctx, const float* rgba, uint32_t width, uint32_t rows, int format, uint32_t flags,
                             uint8_t* out);
/* Diagnostic / tuning: where mrt_present's device-to-host copy runs: 0 a stream of its own (created at the first present in
 * this mode; it shares the process' hardware queues with the render side streams), 1 (default, the faster one measured:
 * profiles/present_rates.txt) the ctx's stream, right behind the present kernel.  The images are the same. */
int mrt_debug_set_present_copy(mrt_ctx* ctx, int mode);
/* Diagnostic: the noise reduction (mrt_noise_query) on caller-supplied buffers, synchronously: S = rows x width floats, rgba =
 * rows x width RGBA32F texels (row 0 first), K the noise factor (+inf allowed); *out as a report (seq 0, frames_done 0), and
 * tiles_out (may be NULL) gets ceil(rows / 8) x ceil(width / 8) tile maxima. */
int mrt_debug_noise_reduce(mrt_ctx* ctx, const float* S, const float* rgba, uint32_t width, uint32_t rows, double K,
                           float threshold, float floor, mrt_noise_report* out, float* tiles_out);
/* Diagnostic: the denoiser's filter (include/myraytracer_amd.h, "denoiser") on caller-supplied buffers, synchronously: rgba =
 * rows x width RGBA32F texels, S = rows x width floats, K the noise factor (+inf allowed), guides = rows x width x 8 floats
 * {normal x, y, z, t, albedo r, g, b, sphere index as int32 bits}; out = rows x width RGBA32F.  params NULL: the ctx's. */
int mrt_debug_denoise(mrt_ctx* ctx, const float* rgba, const float* S, double K, const float* guides, uint32_t width, uint32_t rows,
                      const mrt_denoise_params* params, float* out);
/* Diagnostic: mrt_debug_denoise with a variance estimate ("Variance modes"): 0 accumulated (mrt_debug_denoise itself), 1
 * prefiltered, 2 prefiltered with the spatial initial variance (K is ignored); anything else: MRT_ERR_INVALID_ARG. */
int mrt_debug_denoise_variance(mrt_ctx* ctx, const float* rgba, const float* S, double K, const float* guides, uint32_t width,
                               uint32_t rows, const mrt_denoise_params* params, uint32_t variance, float* out);
/* Diagnostic: mrt_debug_denoise_variance with the blend ("Blend with the accumulation"): mix as mrt_set_denoise_mix takes it (NULL
 * or out of range: MRT_ERR_INVALID_ARG).  With mix->enabled, K is read in every variance, 2 included (v = S * K). */
int mrt_debug_denoise_mix(mrt_ctx* ctx, const float* rgba, const float* S, double K, const float* guides, uint32_t width,
                          uint32_t rows, const mrt_denoise_params* params, uint32_t variance, const mrt_denoise_mix* mix, float* out);
/* Diagnostic: the ctx's guides (rebuilt first if stale), height x width pixels, row 0 = bottom: rays 6 floats (origin,
 * direction), index 1 int32, t 1 float, normal 3 floats, albedo 3 floats per pixel; any pointer may be NULL.  cap_pixels >=
 * width * height.  Synchronous.  MRT_ERR_STATE on a shard, MRT_ERR_NO_SCENE without a scene. */
int mrt_debug_read_guides(mrt_ctx* ctx, float* rays, int32_t* index, float* t, float* normal, float* albedo, size_t cap_pixels);
/* Diagnostic: the same records of the guides mrt_read_gathered_denoised filters with -- the root's current camera and scene over
 * the FULL image, on a root that is a shard too (where mrt_debug_read_guides stays refused).  Its checks are
 * mrt_read_gathered_denoised's without the need for a gathered S: MRT_ERR_NO_SCENE without a scene, MRT_ERR_TOO_SMALL. */
int mrt_debug_read_gathered_guides(mrt_ctx* root_ctx, float* rays, int32_t* index, float* t, float* normal, float* albedo, size_t cap_pixels);

/* Diagnostic: make mrt_gather on this root use the cross-device form of the copy (one hipMemcpyPeerAsync per
 * band) even when a shard shares the root's device, so that its indexing runs on a one-GPU box. */
int mrt_debug_set_gather_per_band(mrt_ctx* root_ctx, int enabled);
/* Diagnostic: the 16 raw u64 counter slots  (0..4 = mrt_counters; 6.. are phase cycle sums
 * written only by the -DMRT_STAMPS profiling build). */
int mrt_debug_read_counters(mrt_ctx* ctx, uint64_t out[16]);
/* Diagnostic: per-pixel cost (bounce-loop trips) of the last frame, local_rows*width u32. */
int mrt_debug_read_pixel_costs(mrt_ctx* ctx, uint32_t* out, size_t cap);
/* Diagnostic / tuning: 0 = one sphere per cluster record, > 0 = clusters of up to 4 spheres (the value itself
 * is no longer used); takes effect at the next mrt_set_world* call. */
int mrt_debug_set_cluster_factor(mrt_ctx* ctx, float factor);
/* Diagnostic / tuning: depth of the bounding-sphere hierarchy built by the next mrt_set_world* call:
 * levels are added (up to max_levels, 1..4) while the top level has more than top_target records (0 = automatic: 256, or
 * 128 for scenes beyond 4,096 member slots, whose walk tests boxes below the top). */
int mrt_debug_set_hierarchy(mrt_ctx* ctx, uint32_t max_levels, uint32_t top_target);
/* Diagnostic / tuning: which variant of the conservative sweep runs: 0 = automatic (matrix cores where the
 * expanded test's slack is negligible for the scene and camera), 1 = SGPR-fed VALU sweep, 2 = matrix cores.
 * Either way the image is the same; takes effect at the next redraw. */
int mrt_debug_set_sweep(mrt_ctx* ctx, int mode);
/* Diagnostic, host only (no context, no device): builds the bounding-sphere hierarchy that mrt_set_world would
 * upload for these spheres and returns it for inspection (tests/test_host_logic.py checks its invariants):
 *   top_out    n_top x (cx, cy, cz, -R^2)          the swept level, padded to a multiple of 32 with never-hit records
 *   nodes_out  n_nodes x (cx, cy, cz, -R^2 | -r^2) levels 0 .. levels-1, level k at info[6 + k]
 *   member_index_out  n_members sphere indices (level 0; padding slots hold 0 and a never-hit record)
 *   mfma_out   n_top / 32 tiles x 512 bf16         the A operand of the matrix-core sweep, origin in mfma_origin_out
 *   info[10] = {levels, n_top, n_nodes, n_members, n_direct, direct_first, level_base[0..3]}
 * Any output pointer may be NULL (sizes are still returned in info); returns MRT_ERR_TOO_SMALL if a capacity
 * (in records / indices / bf16 values) is insufficient. */
int mrt_debug_build_hierarchy(const mrt_sphere* spheres, size_t n, uint32_t max_levels, uint32_t top_target,
                              float* top_out, size_t top_cap, float* nodes_out, size_t nodes_cap,
                              uint32_t* member_index_out, size_t member_cap, uint16_t* mfma_out, size_t mfma_cap,
                              float mfma_origin_out[3], uint32_t info[10]);
/* The same build, returning the axis-aligned boxes of the hierarchy's nodes (the walk's second bound for scenes beyond 1,024
 * member slots): boxes_out = n_boxes x (cx, cy, cz, ex, ey, ez, kc, kpad) -- centre, half extents, and the coefficients of
 * the test's slack K = kc X + kpad, X = |p|^2 (info[2] = 1) or |p|_1 (info[2] = 0) of the ray origin relative to the
 * centre; a never-hit box has extents -3e38.  info[8] = {levels, n_boxes, quadratic?, box_base[0..4]}: the boxes of level
 * k (1 <= k <= levels, the swept top last) start at box_base[k], parallel to that level's records. */
int mrt_debug_build_boxes(const mrt_sphere* spheres, size_t n, uint32_t max_levels, uint32_t top_target, float* boxes_out,
                          size_t boxes_cap, uint32_t info[8]);
/* The same boxes in the order the kernel walks them (what mrt_set_world uploads for a large scene): numbered top-down over the
 * complete 4-ary tree below the n_top swept records -- depth t at o_t = n_top (4^t - 1) / 3, so that the children of node g,
 * whatever its depth, are 4 g + n_top .. + 3; slots without a node hold never-hit boxes.  open != 0: every real box opened
 * wide (the form mrt_debug_set_boxes(0) selects).  info[5] = {levels, n_boxes, n_top, first cluster-level node, first node
 * whose children are clusters}. */
int mrt_debug_build_boxes_top_down(const mrt_sphere* spheres, size_t n, uint32_t max_levels, uint32_t top_target, int open,
                                   float* boxes_out, size_t boxes_cap, uint32_t info[5]);
/* Host-side diagnostic, no GPU needed: the ray-side factors of the matrix-core sweep for a scene and camera that keep every
 * ray origin and every bound within `reach` of the sweep's origin: scale_out[4] = {stretch K, 2 K^2,
 * -(1 - 2^-13) K^2, (4 reach)^2} with K the power of two for which |K oc.ds| <= 1/2 for every admitted ray, and
 * *neg_k2_bf16_pair_out = -K^2 as two bf16.  What mrt_redraw passes to the kernel (tests/test_host_logic.py). */
int mrt_debug_mfma_scale(double reach, float scale_out[4], uint32_t* neg_k2_bf16_pair_out);
/* Host-side diagnostic, no GPU needed: what mrt_set_world derives for the matrix-core sweep of a scene (default hierarchy
 * parameters).  The sweep runs in the space x' = D (x - origin), D = diag(axis_out) with entries 1, 2 or 4 chosen from the
 * spheres alone (force_axis != NULL: that D instead), so that flat clusters get small bounds.  records_out =
 * n_top x (cx, cy, cz, -R^2): the bound of every top record in that space (never-hit: -R^2 = +inf); mfma_out: the A operand
 * made from them, n_top / 32 x 512 bf16, laid out as mrt_debug_build_hierarchy describes -- for D = I the very operand that
 * call returns; *reach_out = max over the spheres of |D (centre - origin)| + |radius| max D, the reach to pass to
 * mrt_debug_mfma_scale.  Output pointers other than axis_out may be NULL; capacities in records / bf16 values. */
int mrt_debug_build_sweep(const mrt_sphere* spheres, size_t n, const float* force_axis, float axis_out[3], float* records_out,
                          size_t records_cap, uint16_t* mfma_out, size_t mfma_cap, float origin_out[3], double* reach_out);
/* Diagnostic: the D of the NEXT mrt_set_world* call is axis[3] (entries 1, 2 or 4) instead of the scene's own choice; NULL
 * returns to the choice.  mrt_debug_sweep_axes: the D of the current scene. */
int mrt_debug_set_sweep_axes(mrt_ctx* ctx, const float* axis);
int mrt_debug_sweep_axes(mrt_ctx* ctx, float axis_out[3]);
/* Diagnostic: ONE world_hit (shader.wgsl:314-329, range [0.001, 1e4)) for each of n caller-supplied rays -- rays[6 i ..] =
 * origin xyz, direction xyz; directions of unit length to 1e-5, as every ray of the render loop is -- through the very sweep +
 * walk the render kernel runs (the same kernel, instantiated to take its rays from this array), with the current scene,
 * hierarchy and sweep variant.  hit_out[2 i] = index of the closest sphere or -1, hit_out[2 i + 1] = the bits of its t;
 * candidates_out (optional): cand_words_per_ray >= ceil(spheres/32) words per ray, bit s set iff sphere s reached the root
 * tests, i.e. passed the conservative sweep, every level of the walk AND the exact discriminant test.  The conservativeness
 * claim of DESIGN.md 4 is that this set equals {s : discriminant_s >= 0} for every ray (tests/test_gpu_superset.py). */
int mrt_debug_world_hit(mrt_ctx* ctx, const float* rays, size_t n, int32_t* hit_out, uint32_t* candidates_out,
                        size_t cand_words_per_ray);
/* Diagnostic: what the last mrt_debug_world_hit call that asked for candidates counted -- out[0] = rays traced (lane slots of
 * its world_hit), out[1] = member tests (4 per cluster item of the walk + one per direct sphere and usable ray): the number
 * of work items the walk ran, which the winners and candidate sets alone do not show.  Zeros before such a call. */
int mrt_debug_world_hit_stats(mrt_ctx* ctx, uint64_t out[2]);
/* Diagnostic: the render kernel's own forms of division and square root -- the correctly rounded expansions of `/` and
 * sqrtf() WITHOUT their operand-scaling steps, used at every root, hit normal and normalize (shader.wgsl:286-299, :354,
 * :381) where the operands cannot need those steps -- against hipcc's `/` and sqrtf() on the device, bit for bit (two NaNs
 * count as equal):
 *   mode 0: the square root of EVERY f32 with bit pattern in [bits_range[0], bits_range[1]];
 *   mode 1: `count` quotients n / d, |n| a bit pattern drawn uniformly from [bits_range[0], bits_range[1]], |d| from
 *           [bits_range[2], bits_range[3]] (SplitMix64 of seed and index), n of either sign; mode 2: d of either sign too.
 * out[0] = operands tested, out[1] = operands whose results differ, out[2] = the smallest differing operand (mode 0: the
 * bits of x; else bits(n) | bits(d) << 32; ~0 if none). */
int mrt_debug_arith(mrt_ctx* ctx, int mode, const uint32_t bits_range[4], uint64_t count, uint64_t seed, uint64_t out[3]);
/* The same for n caller-supplied operand pairs: out[6 i ..] = bits(x / y), bits(unscaled quotient), bits(sqrtf(x)),
 * bits(unscaled root), and the render kernel's two per-wave operand tests evaluated on the pair -- hit normal: x a component
 * of (at - centre), y the radius; normalize: x the squared length, y a component -- 1 = unscaled forms, 0 = the wave takes
 * the literal `/` and sqrtf(). */
int mrt_debug_arith_pairs(mrt_ctx* ctx, const float* x, const float* y, size_t n, uint32_t* out);
/* Diagnostic: which instantiation of the render kernel the most recent redraw launched (out[0]) and, if it was preceded by
 * a cost-estimating pilot launch not yet reported, which one that was (out[1], else 0xFFFFFFFF): bit 0 = with the RNG draw
 * counter, 1 = pilot, 2 = counter-RNG mode, 3 = small-scene layout, 4 = matrix-core sweep, 5 = large-scene layout with the
 * quadratic form of the box test's slack (else the linear form), 6 = the launch got the camera-ray sphere lists (the SC = 3
 * instantiations; set for the pilot and the main launch alike)
 * (tests/test_gpu_parity.py::test_every_render_kernel_instantiation_against_the_oracle,
 * tests/test_gpu_camera_list_launches.py::test_every_list_instantiation_against_the_oracle). */
int mrt_debug_last_launch(mrt_ctx* ctx, uint32_t out[2]);
/* Diagnostic A/B switch (large scenes, > 1,024 member slots, whose walk tests the axis-aligned box of every node): 0 opens
 * every box wide, so that the box tests never reject and the walk reaches every member below the swept candidates; 1 (default)
 * and 2: the real boxes.  Either way the image is the same.  Takes effect at the next redraw. */
int mrt_debug_set_boxes(mrt_ctx* ctx, int mode);
/* Which variant the next redraw will run with the current scene, camera and mode: 1 or 2 (0 before a scene is set). */
int mrt_debug_sweep_variant(mrt_ctx* ctx);
/* Diagnostic A/B switch: 0 makes mrt_render launch every frame on its own; 1 = automatic (default); 2 / 3 force the form a
 * batch takes -- 2: the lane that takes a pixel renders it for every frame of the batch (what short frames of a large image
 * get), 3: the frames are layers of the tile queue (what a pixel-starved shard gets).  The images are the same. */
int mrt_debug_set_frame_batching(mrt_ctx* ctx, int enabled);
/* Diagnostic A/B switch: 0 queues tiles in index order instead of heaviest-first. */
int mrt_debug_set_tile_sort(mrt_ctx* ctx, int enabled);
/* Diagnostic: the tile-queue sort a frame runs, on caller-supplied costs, synchronously (it waits for the frames in flight
 * first).  cost = n_cost u32, 1 <= n_cost <= the context's tile count (pick the image size for the count wanted).  list NULL:
 * the whole-frame sort of tiles 0 .. n_cost - 1 (n must equal n_cost); else the list sort of a subset frame over the n <=
 * n_cost tile ids of list[], each < n_cost.  order_out gets the n entries of the queue, heaviest first (ties in any order).
 * Staged through the buffers of the slot of the most recent frame: afterwards that slot's cost estimate is marked invalid, so
 * the caller's costs never order a real frame (the next one gets a pilot launch or index order), and
 * mrt_debug_read_tile_schedule reports MRT_TILE_ORDER_NONE until the slot's next frame.  MRT_ERR_NO_SCENE without a scene. */
int mrt_debug_sort_tiles(mrt_ctx* ctx, const uint32_t* cost, size_t n_cost, const uint32_t* list, size_t n, uint32_t* order_out);
/* Diagnostic: the scheduling state of the slot of the most recent frame, after waiting for the frames in flight.  cost_out
 * (may be NULL): the per-tile costs as that slot's last finalize or per-tile blend left them, *n_out = the context's tile
 * count of them.  order_out (may be NULL): the queue order the slot's most recent render launch was given, info_out[1]
 * entries.  cap >= the tile count holds for both.  info_out[4] = {how the order came about (MRT_TILE_ORDER_*), its entries,
 * 1 if a cost-estimating pilot launch preceded the launch, the slot}.  MRT_ERR_NO_SCENE without a scene. */
#define MRT_TILE_ORDER_NONE 0u        /* no render launch on this slot yet (or mrt_debug_sort_tiles since) */
#define MRT_TILE_ORDER_INDEX 1u       /* whole frame, no sort: tiles 0 .. n - 1 */
#define MRT_TILE_ORDER_SORTED 2u      /* whole frame, heaviest first by the slot's costs */
#define MRT_TILE_ORDER_SORTED_LIST 3u /* subset frame, its list heaviest first by the slot's costs */
#define MRT_TILE_ORDER_LIST 4u        /* subset frame, its list as the caller gave it */
int mrt_debug_read_tile_schedule(mrt_ctx* ctx, uint32_t* cost_out, uint32_t* order_out, size_t cap, uint32_t* n_out,
                                 uint32_t info_out[4]);
/* Diagnostic / tuning: pilot samples per pixel, waves per CU (0 = automatic).  Before the first
 * redraw only. */
int mrt_debug_set_schedule(mrt_ctx* ctx, uint32_t pilot_spp, int waves_per_cu);
/* Host-side diagnostic, no GPU needed: the LDS footprint of the render kernel for a scene with this hierarchy (the sizes
 * mrt_debug_build_hierarchy reports): out[3] = {bytes per workgroup of 4 waves, workgroups resident per CU (160 KB of LDS;
 * large scenes: at most 4, the occupancy their kernels are built for), entries of a wave's top queue (small scenes) / work
 * stack (large scenes)}.  tests/test_hierarchy_host.py pins the residency of C3's and C5's layouts with it. */
int mrt_debug_lds_layout(uint32_t n_members, uint32_t n_nodes, uint32_t levels, uint32_t n_top_padded, uint32_t out[3]);
/* Diagnostic / tuning: how many frames may be in flight (each on a side stream of its own; 1..16), 0 = automatic: 2, more for
 * pixel-starved shards.  A change waits for the frames under way.  The images are the same. */
int mrt_debug_set_frames_in_flight(mrt_ctx* ctx, int slots);
/* Host only, no GPU needed: the launch-width controller's policy (csrc/width_policy.h) on synthetic input, for its CPU unit
 * tests.  workload[6] = {n_tiles, n_waves, max_slots, spp, n_members, counter-RNG?}; state[7] in / out = {div, mult, prev_div,
 * prev_mult, low_windows, settled, prev_rate as the bits of an f32}.  op 0: what is known up front (state out only);
 * op 1: one measurement window has closed with lane utilisation `util` and `rate` frames / s; op 2: state[0] out = the share a
 * launch gets under setting state[0] when `util` (as an integer) earlier frames are still queued or running. */
int mrt_debug_width_policy(int op, const uint32_t workload[6], uint32_t state[7], double util, double rate);
/* Host only, no GPU and no context needed: a FRESH launch-width controller (csrc/width_policy.h, WidthController -- the policy
 * above plus its bookkeeping: workloads, hint, memo, the caller's frames in flight, measurement windows) run through n_calls
 * synthetic frame calls, for its CPU unit tests.  Call i is frame i (one frame per call) and goes through the steps of a
 * redraw in the library's order, with what the device would have answered given by the caller:
 *   calls[13 i ..] = {workload: n_tiles, n_waves, max_slots, spp, n_members, counter-RNG?, n_spheres; hint div, mult ((0, 0) =
 *     none; a change is mrt_set_schedule_hint); invalidate? (what mrt_set_camera and the other setters do before this call);
 *     earlier frames found queued or running; device start-to-start intervals of the window's frames (0 = none); landed samples}
 *   times[2 i ..] = {the host's clock at the call (s), the sum of those intervals (ms)}
 *   samples: 3 per landed sample, in the calls' order: {frame, cumulative world_hit calls, cumulative lane slots}
 *   out[9 i ..] = {div, mult, settled, frames in flight, frames running as the controller sees them, the share the frame is
 *     launched on (1 / this), a window is open after the call?, a window closed at this call?, entries of the memo}
 *   measured[2 i ..] = {lane utilisation, frames / s} of the window that closed at this call (else 0)
 * max_slots is what the controller holds before any probe (the first call's counts; the library: 16); probe_slots is what
 * the stream-concurrency probe reports when a setting first asks for more than two frames (0 = all 16). */
#define MRT_WIDTH_CALL_WORDS 13u
#define MRT_WIDTH_DECISION_WORDS 9u
int mrt_debug_width_replay(uint32_t probe_slots, size_t n_calls, const uint32_t* calls, const double* times, const uint64_t* samples,
                           size_t n_samples, uint32_t* out, double* measured);
/* Diagnostic: how many of `streams` (2..16) side streams of this context really run side by side in this process -- identical
 * short clock-bounded kernels, one per stream, each stamping its start and end on the device's clock: *out = the most of them
 * resident at one instant (hardware queues are shared round-robin: HIP's default of 4 per process gives 4).  What caps the
 * frames in flight (mrt_get_schedule). */
int mrt_debug_stream_concurrency(mrt_ctx* ctx, uint32_t streams, float* out);
/* Diagnostic: per-wave log {t_start, t_end (100 MHz ticks), loop trips, bounces}, 4 u64 per 8x8
 * persistent wave, written only by the -DMRT_STAMPS build.  out == NULL allocates the log. */
int mrt_debug_wave_log(mrt_ctx* ctx, uint64_t* out, size_t cap_waves, size_t* n_waves);
/* The same for the frame `back` (0..31) redraws before the most recent one: the log is a ring over the last 32 frames, so that
 * the frames in flight of a narrow schedule can be laid side by side (scripts/shard_occupancy.py).  Entries of waves a launch
 * did not have are zero. */
int mrt_debug_wave_log_frame(mrt_ctx* ctx, uint32_t back, uint64_t* out, size_t cap_waves, size_t* n_waves);
/* Host wall time (ms) the most recent mrt_set_world* call spent building and uploading the bounding-sphere
 * hierarchy (a one-off per scene, outside the per-frame metric). */
int mrt_debug_last_set_world_ms(mrt_ctx* ctx, float* ms);
/* Host only, launches nothing: walks the context and returns 0 if no call it would accept -- the next frame, query, present,
 * denoise, gather or read-back -- could touch a buffer, stream or event that is not there; else 1, with the first finding in
 * `why` (cap bytes).  A part the context knows it lacks and refuses the calls for (no scene: MRT_ERR_NO_SCENE) is sound.
 * tests/test_gpu_failure_paths.py calls it after every refused resource creation, before anything else is launched; the
 * state-machine sequences (tests/state_sequences.py) end with it. */
int mrt_debug_check_context(mrt_ctx* ctx, char* why, size_t cap);
/* Diagnostic: the scene's hierarchy as the device holds it, read back behind the ctx's stream (after every mrt_update_spheres
 * queued so far).  info[16] = {levels, top records, nodes, member slots, direct spheres, direct_first, level_base[4], boxes (0 for
 * a small scene), box_quad, spheres, box_cluster_first, box_cluster_parent_first, the build's matrix-core verdict}; a first call
 * with every array NULL gives the sizes.  scalars[8] = {box_kc, the sweep's origin xyz, its axes xyz, its reach}; direct_out =
 * 4 x 4 floats, direct_index_out = 4: the direct spheres' records as the kernel arguments carry them.  Arrays (each may be
 * NULL): top 4 floats a record; nodes 4 floats; member_index; boxes and boxes_open 6 floats a box in the kernel's top-down
 * numbering; the A operand 512 u16 per tile of 32 top records; and the four copies of the spheres' geometry -- spheres (4
 * floats), shade (8 floats), the SoA's centres (4 floats) and radii.  MRT_ERR_NO_SCENE without a scene. */
int mrt_debug_read_hierarchy(mrt_ctx* ctx, uint32_t info[16], double scalars[8], float* direct_out, uint32_t* direct_index_out,
                             float* top_out, float* nodes_out, uint32_t* member_index_out, float* boxes_out, float* boxes_open_out,
                             uint16_t* mfma_out, float* spheres_out, float* shade_out, float* centres_out, float* radii_out);
/* Host only: floats 4..7 of the shade record of a sphere with this material -- the one derivation mrt_set_world_raw and
 * mrt_update_materials share.  Lambertian: albedo, 0; Metal: albedo, fuzz; Dielectric: 1/ior, ((1 - ri)/(1 + ri))^2 for ri =
 * 1/ior and for ri = ior, ior (every operation rounded to float); any other type: 1, 1, 1, 0.  MRT_ERR_INVALID_ARG for NULL. */
int mrt_debug_material_shade(const mrt_material* material, float out[4]);
/* Diagnostics of mrt_regroup_spheres.  mrt_debug_regroup_info: out[4] = {the clusters the builder made from the spheres that may
 * share one (the regroup permutes over their slots), the block capacity in force (clusters a workgroup of the block kernel
 * takes), the depths the last regroup ran over global memory, the depths it ran in LDS}; the last two are 0 before the first
 * regroup of a scene.  mrt_debug_set_regroup_block: the block capacity of the next regroups, a power of two from 4 to the
 * built-in 512, 0 = the default -- lets tiny scenes drive the global depths.  mrt_debug_pool_clusters (host only): the first of
 * those numbers for the hierarchy mrt_debug_build_hierarchy builds. */
int mrt_debug_regroup_info(mrt_ctx* ctx, uint32_t out[4]);
int mrt_debug_set_regroup_block(mrt_ctx* ctx, uint32_t clusters);
int mrt_debug_pool_clusters(const mrt_sphere* spheres, size_t n, uint32_t max_levels, uint32_t top_target, uint32_t* n_pool);
/* Camera-ray cluster masks (small scenes of at most 128 top records): mrt_debug_set_camera_masks switches them
 * off / on for the launches that follow (an A/B switch: images and the counters samples / world_hit_calls / rng_draws do not
 * depend on it, member_tests do).  mrt_debug_read_camera_masks: info[4] = {entries the table holds for the current shard (0: the
 * masks do not apply -- a large scene, more than 128 top records, a shard that outgrew the table), words per entry (4), whether the
 * most recent render launch ran with them, whether the table is built for the current scene / camera / shard}; with `out` (cap_words
 * >= entries x 4) the table itself, entry e = texels 8 e .. 8 e + 7 of the shard's row-major order, top record 32 w + i at bit
 * 31 - i of word w.  MRT_ERR_NO_SCENE without a scene, MRT_ERR_TOO_SMALL for a short buffer.
 * Camera-ray sphere lists: built with the masks and switched with them.  A launch with enough pixels to be bound by throughput gets
 * the lists instead of the masks -- its camera rays are resolved in the lane against their entry's member slots -- and info[2] is 2
 * after it (1: the masks).  mrt_debug_set_camera_masks(ctx, 2) gives every launch the tables apply to the lists, 3 the masks (1: the
 * library's rule).  mrt_debug_read_camera_lists: the same info[4], and with
 * `out` the lists' table, 4 words per entry of the same indexing: word 0 = the number of level-0 member slots a camera ray of the
 * entry's texels can touch, at most 8, or 0xFFFFFFFF for an entry with more (its rays take world_hit; so does every entry before
 * the first build); words 1 .. 3 = the slot ids in ascending order, 10 bits each, id k at bits 10 k .. 10 k + 9 of the 96 bits. */
int mrt_debug_set_camera_masks(mrt_ctx* ctx, int on);
int mrt_debug_read_camera_masks(mrt_ctx* ctx, uint32_t info[4], uint32_t* out, size_t cap_words);
int mrt_debug_read_camera_lists(mrt_ctx* ctx, uint32_t info[4], uint32_t* out, size_t cap_words);
/* Diagnostics of temporal reprojection: the context's OWN history (the pair the next step reads: h0 = (r, g, b, len), h1 = (m1,
 * m2, t, index bits), 4 floats a pixel each, y * width + x), its previous spheres (4 floats each) and, for the load, its previous
 * derived camera, read / overwritten behind the ctx's stream, so that a test can start a step from a synthetic history.  They
 * allocate nothing: MRT_ERR_STATE while temporal reprojection is off or before the first step has brought the buffers.  read: cap
 * in pixels (and at least the sphere count when prev_xyzr is given); any array may be NULL.  load: n_spheres must be the scene's
 * when prev_xyzr is given; prev_cam NULL keeps the camera; a loaded history counts as stepped (mrt_read_temporal reads it). */
int mrt_debug_read_temporal(mrt_ctx* ctx, float* h0, float* h1, float* prev_xyzr, size_t cap);
int mrt_debug_load_temporal(mrt_ctx* ctx, const float* h0, const float* h1, const float* prev_xyzr, size_t n_spheres,
                            const mrt_camera_raw* prev_cam);
/* ... and the response's fast history of that pair, H2 = (fr, fg, fb, valid), 4 floats a pixel: the refusals of the two above,
 * and MRT_ERR_STATE while the response is off or before a step with it on has brought the H2 pair (the pair comes with the
 * denoiser's buffers, so with both settings on a denoise before the first step may have brought it already: between enabling
 * and the first step the answer is either; from that step on it is defined); h2 NULL: MRT_ERR_INVALID_ARG.
 * read: cap in pixels.  load: everything else as mrt_debug_load_temporal with every array NULL leaves it. */
int mrt_debug_read_temporal_fast(mrt_ctx* ctx, float* h2, size_t cap);
int mrt_debug_load_temporal_fast(mrt_ctx* ctx, const float* h2);
/* Diagnostic of the denoiser and adaptive sampling: an accumulation of the caller's in the place of the context's own, so that a
 * test can put non-finite texels, tiles of 0 or 1 frames and any map of n_t in front of the product's denoise and noise report.
 * World 1 only (a shard: MRT_ERR_STATE).  Waits (bounded) for the frames in flight, then overwrites what mrt_read_framebuffer
 * (rgba: height * width * 4 floats, row 0 = bottom), mrt_read_noise (S: height * width floats; MRT_ERR_STATE with tracking off)
 * and mrt_read_tile_frames (tile_frames: one count per tile, each < 2^20, else MRT_ERR_INVALID_ARG and nothing changed) read;
 * any pointer may be NULL and leaves that part as it is.  tile_frames makes the accumulation adaptive if it is not yet -- as
 * the first subset frame of mrt_render_tiles would, with the one allocation of that step -- and sets the device's and the host's
 * copy of the map; nothing else is allocated.  mrt_frames_done is untouched; mrt_reset returns to the uniform state. */
int mrt_debug_load_accumulation(mrt_ctx* ctx, const float* rgba, const float* S, const uint32_t* tile_frames);
/* Diagnostic of the stream ordering (tests/order_walks.py): queues ONE single-wave kernel on a stream of the context that stays
 * resident for `ticks` of the device's 100 MHz wall clock or for `max_polls` polls of it (about a microsecond each), whichever
 * comes first -- the exit never depends on the clock alone -- so that whatever is queued behind it on that stream starts late
 * while the other streams run on.  which: MRT_HOLD_CONTEXT the context's stream (the caller's after mrt_set_stream),
 * MRT_HOLD_SLOT the side stream of frame slot `index` (a frame lands on slot frame number % frames in flight), MRT_HOLD_PRESENT
 * the present's copy stream, MRT_HOLD_NOISE the stream of the tile map's copy; index must be 0 except for MRT_HOLD_SLOT.
 * Creates nothing: MRT_ERR_STATE where the stream does not exist yet (a slot beyond the first two that no schedule has used, no present with
 * mrt_debug_set_present_copy(0), no mrt_read_noise_tiles so far).  ticks == 0, ticks > MRT_HOLD_MAX_TICKS (half a second),
 * max_polls == 0 or an unknown `which` / slot: MRT_ERR_INVALID_ARG.  Returns at once.  mrt_debug_hold_stamps (host only; after
 * the hold has ended, e.g. behind mrt_sync): out[0], out[1] = the {start, end} ticks the most recent hold wrote, out[2] = the
 * polls it was given (zeros before the first hold). */
#define MRT_HOLD_CONTEXT 0u
#define MRT_HOLD_SLOT 1u
#define MRT_HOLD_PRESENT 2u
#define MRT_HOLD_NOISE 3u
#define MRT_HOLD_MAX_TICKS 50000000ull
int mrt_debug_hold(mrt_ctx* ctx, uint32_t which, uint32_t index, uint64_t ticks, uint32_t max_polls);
int mrt_debug_hold_stamps(mrt_ctx* ctx, uint64_t out[3]);
/* Diagnostic: the allocation of mrt_noise_query_budget on caller-supplied arrays, synchronously: s = `tiles` summed-S values
 * (any float), n = `tiles` frame counts, or NULL: n_uniform for every tile; k_out gets `tiles` values, *res the plan's result
 * (used_seq 0).  The same kernels, launched the same way, in temporary buffers of its own; K is the context's table for its
 * max_framebuffer_weight, grown as the query grows it, so the yardstick is mrt_budget_allocate(s, n, that weight, ...).  Needs no
 * noise tracking, no scene and no frames.  max_frames outside 1 .. 32 or an n_t above 2^24: MRT_ERR_INVALID_ARG before anything
 * is allocated or grown (mrt_noise_query_budget's own checks); tiles 0 or above 2^28, or a NULL pointer: MRT_ERR_INVALID_ARG. */
int mrt_debug_budget_plan(mrt_ctx* ctx, const float* s, const uint32_t* n, uint32_t n_uniform, size_t tiles, uint64_t budget,
                          uint32_t max_frames, uint32_t* k_out, mrt_budget_result* res);

#ifdef __cplusplus
}
#endif
#endif /* MYRAYTRACER_AMD_DEBUG_H */
