/*
 * myraytracer_amd.h -- C ABI of the MI355X-native backend for the per-pixel render loop
 * of zetanumbers/myraytracer.
 *
 * The reference has no FFI / plugin seam for this path: the WGSL shader is
 * include_str!-embedded (raytracer/src/lib.rs:1016) and run by a wgpu draw
 * (lib.rs:262-267).  Each entry point below therefore names the reference item it
 * replaces; INTEGRATION.md shows the Rust `extern "C"` block a maintainer would add to
 * raytracer/src/lib.rs to route `State` through this library.
 *
 * Conventions
 *   - every function returns an mrt_status (0 = OK) unless stated; nothing aborts or
 *     throws across the ABI (the reference panics via expect/unwrap, lib.rs:147,270,...).
 *   - one mrt_ctx = one GPU = one caller thread at a time (the reference's State is
 *     single-threaded and !Send, lib.rs:206-215).
 *   - the caller owns every host array passed in (copied during the call) and every
 *     output buffer; the ctx owns all device memory.
 *   - framebuffer rows are bottom-up: row 0 is the BOTTOM of the picture
 *     (shader.wgsl:26 vs sample_framebuffer.wgsl:24).
 *   - all structs are plain C, 4-byte fields, no padding surprises (static_asserts in
 *     csrc/api.cpp).
 */
#ifndef MYRAYTRACER_AMD_H
#define MYRAYTRACER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: round 4 -- the diagnostic entry points (mrt_debug_*) moved to myraytracer_amd_debug.h; mrt_build_id added; since 2 the
 * library also gained mrt_set_draw_counting and the boxes / frame-batching diagnostics, and mrt_debug_set_hierarchy /
 * mrt_debug_build_hierarchy accept top_target 0 = automatic ("ABI history"). */
/* 4: round 5 -- MRT_ERR_STALLED and mrt_set_wait_timeout (every blocking host wait has a deadline), mrt_set_schedule_hint /
 * mrt_get_schedule (the launch schedule a run settled at can be read and pinned); mrt_create no longer touches the process
 * environment (GPU_MAX_HW_QUEUES is the host's to set: INTEGRATION.md 2a).  Version 4 later gained, additions only: the
 * device-side present pass (mrt_present, mrt_present_acquire, mrt_present_release, mrt_set_present_ring, mrt_present_info);
 * the noise estimate (mrt_set_noise_tracking, mrt_noise_query, mrt_noise_result, mrt_read_noise, mrt_read_noise_tiles,
 * mrt_noise_factor, mrt_noise_report); the denoiser (mrt_denoise_params, mrt_denoise_params_default, mrt_set_denoise_params,
 * mrt_get_denoise_params, mrt_set_denoise_variance, mrt_get_denoise_variance, mrt_read_denoised, MRT_PRESENT_DENOISED);
 * adaptive sampling (mrt_render_tiles, mrt_render_adaptive, mrt_read_tile_frames); temporal reprojection (mrt_temporal_params,
 * mrt_temporal_params_default, mrt_set_temporal, mrt_get_temporal, mrt_temporal_step, mrt_temporal_reset, mrt_read_temporal,
 * MRT_PRESENT_TEMPORAL); the temporal response (mrt_temporal_response, mrt_temporal_response_default,
 * mrt_set_temporal_response, mrt_get_temporal_response); the noise estimate across shards and the gathered frame's denoise
 * (mrt_set_gather_noise, mrt_read_gathered_noise, mrt_read_gathered_denoised, MRT_PRESENT_GATHERED_DENOISED); the denoise of
 * an adaptive accumulation (mrt_set_denoise_adaptive, mrt_get_denoise_adaptive); the auto-regroup policy (mrt_auto_regroup,
 * mrt_auto_regroup_default, mrt_set_auto_regroup, mrt_get_auto_regroup, mrt_regroup_stats, mrt_read_regroup_stats); the
 * denoiser's blend with the accumulation (mrt_denoise_mix, mrt_denoise_mix_default, mrt_set_denoise_mix, mrt_get_denoise_mix);
 * material edits without a rebuild (mrt_material, mrt_update_materials, MRT_MATERIALS_RESTART_HISTORY); adaptive sampling by
 * budget (MRT_TILE_MAP_MAX_REL, MRT_TILE_MAP_SUM_S, mrt_noise_query_map, mrt_budget_result, mrt_budget_allocate,
 * mrt_render_budget; mrt_noise_report::reserved carries the report's map kind); budget allocation on the device
 * (mrt_noise_query_budget, mrt_read_budget_plan, mrt_render_planned); the present pass's linear formats
 * (MRT_PRESENT_RGBA16F_LINEAR, MRT_PRESENT_RGBA32F_LINEAR, mrt_half_bits, mrt_half_from_floats); the diagnostic views
 * (mrt_view, MRT_VIEW_*, mrt_view_default, mrt_set_view, mrt_get_view, mrt_read_view, MRT_PRESENT_VIEW). */
#define MRT_ABI_VERSION 4

typedef enum {
    MRT_OK = 0,
    MRT_ERR_INVALID_ARG = 1,   /* null pointer, zero size, bad enum */
    MRT_ERR_NO_DEVICE = 2,     /* no HIP device / wrong arch: the product never falls back to CPU */
    MRT_ERR_HIP = 3,           /* a HIP runtime call failed; see mrt_last_error, and "after MRT_ERR_HIP" below */
    MRT_ERR_NO_SCENE = 4,      /* redraw before set_world */
    MRT_ERR_BAD_SCENE = 5,     /* index out of range, non-finite or out-of-range geometry */
    MRT_ERR_TOO_SMALL = 6,     /* caller buffer too small */
    MRT_ERR_STATE = 7,         /* call not allowed in this state (e.g. reshard after first frame) */
    MRT_ERR_IO = 8,
    MRT_ERR_STALLED = 9        /* a wait for the GPU passed its deadline (mrt_set_wait_timeout); mrt_last_error names the wait.
                                  The context stays failed: destroy it (mrt_destroy does not wait for a stalled context) */
} mrt_status;

/* ---- after MRT_ERR_HIP: what a caller may rely on when the runtime refuses a resource ----
 * Device memory, pinned memory, streams and events are created by mrt_create and, on demand, by most later calls.  When a
 * creation is refused (out of memory, out of handles):
 *   C1  the call returns MRT_ERR_HIP and mrt_last_error(ctx) -- mrt_last_error(NULL) for mrt_create -- names the refused
 *       runtime call ("hipMalloc(...) failed: ...");
 *   C2  nothing leaks and nothing is released twice: after mrt_destroy the process holds what it held before mrt_create.  A
 *       failed mrt_create leaves nothing behind and sets *out = NULL;
 *   C3  the context stays sound: no call it accepts afterwards touches a buffer, stream or event that is not there.  A call
 *       that replaces something keeps the old until the new exists (mrt_set_shard: the shard and its buffers are unchanged
 *       after a failure) or the context knows what it lost (mrt_set_world*: no scene, MRT_ERR_NO_SCENE from the render
 *       calls, until a mrt_set_world* succeeds);
 *   C4  the call can be repeated: once the runtime has the resource to give, the same call succeeds, and every image,
 *       counter and report from then on is bit-identical to a run in which nothing was ever refused (the schedule -- launch
 *       widths, frames in flight -- may differ, as it may between any two runs).
 * Failures of the calls that ENQUEUE work (copies, memsets, event records, launches) are reported as MRT_ERR_HIP too, but
 * are outside this contract.  tests/test_gpu_failure_paths.py holds C1-C4 at every creation site by failure injection. */

/* ---- raytracer::Args, lib.rs:18-37; flags of native-runner/src/main.rs:20-31 ---- */
typedef struct {
    uint32_t width;                 /* default 0 */
    uint32_t height;                /* default 0 */
    uint32_t samples_per_frame;     /* default 1 */
    uint32_t ray_depth;             /* default 50 */
    float    max_framebuffer_weight;/* default 1.0 */
} mrt_args;

/* Args::default(), lib.rs:27-37 */
void mrt_args_default(mrt_args* out);
/* Size rule of App::resumed, lib.rs:113-134,149-154: both 0 -> default window size
 * (MRT_DEFAULT_WIDTH x MRT_DEFAULT_HEIGHT here, there is no window); exactly one 0 ->
 * square of the other. */
#define MRT_DEFAULT_WIDTH 800
#define MRT_DEFAULT_HEIGHT 600
void mrt_args_resolve_size(mrt_args* inout);

/* ---- Locals uniform, lib.rs:368-377 / shader.wgsl:8-17 (48 bytes) ---- */
typedef struct {
    uint32_t shape[2];
    uint32_t samples_per_frame;
    uint32_t ray_depth;
    uint32_t rng_shuffle[4];
    float    framebuffer_weight;
    uint32_t rng_mode;          /* the reference's first padding word: 0 = its per-pixel stream (MRT_RNG_*) */
    uint32_t _padding[2];
} mrt_locals;

/* RNG modes.  0 is the reference: one sequential Xoshiro128+ stream per pixel per frame
 * (shader.wgsl:377-382).  1 is an extension (north_star's "counter-based RNG per lane"): every sample
 * starts from a hash of (seed texel ^ rng_shuffle, sample index), so samples are independent of how
 * many draws earlier samples consumed; within a sample the draw order is the reference's. */
enum { MRT_RNG_PIXEL_STREAM = 0, MRT_RNG_COUNTER = 1 };
/* In the counter mode a pixel's colour sum is DEFINED blockwise: S_b = the sequential sum of samples [64 b, 64 b + 64),
 * colour = ((S_0 + S_1) + S_2) ... -- up to 64 samples per frame the same expression as the stream mode's.  Blocks of
 * one pixel may then be rendered by different lanes, which is what keeps a small shard of a many-spp frame (an 8-GPU
 * share of 1920x1080 at 4,096 spp) from starving the GPU. */
#define MRT_COUNTER_BLOCK 64

/* ---- raw::World, lib.rs:641-685 / shader.wgsl:109-124,165-182 (64 bytes) plus the
 *      Dielectric extension appended after MetalRange (80 bytes total) ---- */
typedef struct {
    int32_t center_base_idx, radius_base_idx, material_ty_base_idx, material_idx_base_idx;
    int32_t length, _padding[3];
} mrt_sphere_range;
typedef struct { int32_t albedo_base_idx, length, _padding[2]; } mrt_lambertian_range;
typedef struct { int32_t albedo_base_idx, fuzz_base_idx, length, _padding; } mrt_metal_range;
typedef struct { int32_t ior_base_idx, length, _padding[2]; } mrt_dielectric_range;  /* extension */
typedef struct {
    mrt_sphere_range     spheres;
    mrt_lambertian_range lambertians;
    mrt_metal_range      metals;
    mrt_dielectric_range dielectrics;
} mrt_world;

/* raw::MaterialTy, lib.rs:644-648 / shader.wgsl:126-127; 3 is the extension */
enum { MRT_LAMBERTIAN = 1, MRT_METAL = 2, MRT_DIELECTRIC = 3 };

/* ---- api::Sphere / api::DynMaterial, lib.rs:611-639, flattened to one POD ----
 * albedo is used by Lambertian and Metal; param = fuzz (Metal) or index of refraction
 * (Dielectric). 36 bytes. */
typedef struct {
    float   center[3];
    float   radius;
    int32_t material_ty;
    float   albedo[3];
    float   param;
} mrt_sphere;

/* ---- camera (extension; mode 0 is the reference's fixed pinhole, shader.wgsl:360-381) */
typedef struct {
    int32_t mode;                  /* 0 = reference pinhole, 1 = look-at thin lens */
    float   lookfrom[3], lookat[3], vup[3];
    float   vfov_deg, defocus_angle_deg, focus_dist;
} mrt_camera;
typedef struct {                   /* what the kernel consumes; derived on the host in double */
    int32_t mode, defocus;
    float   origin[3], su[3], sv[3], fw[3], ru[3], rv[3];
} mrt_camera_raw;

typedef struct {
    uint64_t samples;              /* camera rays started */
    uint64_t world_hit_calls;      /* = bounces; sphere tests = world_hit_calls * spheres.length */
    uint64_t rng_draws;            /* xoshiro128+ outputs consumed */
    uint64_t lane_slots;           /* 64 x trips of each wave's bounce loop: world_hit_calls / lane_slots
                                      = SIMD lane utilisation of the kernel (diagnostic, not in the oracle) */
    uint64_t member_tests;         /* per-sphere discriminants evaluated (members of candidate clusters + directly tested spheres) */
    uint64_t sweep_records;        /* top-level bound records the sweep tests per world_hit (not accumulated): executed
                                      bound tests of the sweep = world_hit_calls * sweep_records */
} mrt_counters;

typedef struct mrt_ctx mrt_ctx;

/* ------------------------------------------------------------------ lifecycle */

/* App::new + State::new (lib.rs:77,217-234): allocates the seed texture (Subject::new,
 * lib.rs:389-415; seeded deterministically from `seed` instead of entropy), the two
 * ping-pong framebuffers (DoubleFramebuffers::new, lib.rs:514-538) and the Locals.
 * `device` is the HIP device ordinal.  Fails with MRT_ERR_NO_DEVICE if there is none. */
int mrt_create(const mrt_args* args, uint64_t seed, int device, mrt_ctx** out);
/* Drop of State's wgpu handles */
void mrt_destroy(mrt_ctx* ctx);

/* Deadline, in seconds, of every wait for the GPU inside this library (the back-pressure of mrt_redraw, mrt_sync, read-backs,
 * re-allocations, mrt_destroy): a wait that lasts longer fails with MRT_ERR_STALLED and names itself ("back-pressure of slot 3,
 * frame 17, 8 frames in flight") instead of hanging -- the reference's frame loop would block in wgpu's present forever
 * (lib.rs:270).  Default 120 s (or the environment's MRT_WAIT_TIMEOUT_S at mrt_create); 0 = no deadline.  Must exceed the
 * longest single frame the caller renders. */
int mrt_set_wait_timeout(mrt_ctx* ctx, double seconds);

/* Tile sharding for multi-GPU (no reference counterpart): this ctx renders the 8-row
 * bands b with b % world == rank.  Must be called before the first redraw.  Seeds are
 * keyed by global pixel index, so any sharding yields the same image.  Only while mrt_frames_done == 0 (after
 * mrt_create or mrt_reset), else MRT_ERR_STATE.  The buffers are allocated anew for the shard's rows: the seed
 * texture is filled again from mrt_create's seed (an earlier mrt_set_seeds is lost), presented images and unread
 * noise reports are discarded; scene, camera, samples per frame, RNG mode and an overridden shuffle stay.  With temporal
 * reprojection on, world > 1 is MRT_ERR_STATE and the history is dropped otherwise. */
int mrt_set_shard(mrt_ctx* ctx, uint32_t rank, uint32_t world);
/* hipStream_t to launch on (e.g. torch's current stream); NULL = the ctx's own stream. */
int mrt_set_stream(mrt_ctx* ctx, void* hip_stream);

/* ------------------------------------------------------------------ scene */

/* Object::new's upload (lib.rs:768-863): the raw::World index block and the three SoA
 * arrays, verbatim.  `world` points to world_bytes bytes: MRT_WORLD_BYTES_REFERENCE (64) = the
 * reference's raw::World exactly as lib.rs:676-684 lays it out (no dielectrics), or
 * sizeof(mrt_world) (80) = with the DielectricRange extension; nothing beyond world_bytes is
 * read.  vec4_data: n_vec4 x 4 floats, f32_data: n_f32 floats, i32_data: n_i32 ints.  All
 * base+length ranges are validated. */
#define MRT_WORLD_BYTES_REFERENCE 64
int mrt_set_world_raw(mrt_ctx* ctx, const void* world, size_t world_bytes,
                      const float* vec4_data, size_t n_vec4,
                      const float* f32_data, size_t n_f32,
                      const int32_t* i32_data, size_t n_i32);
/* api::World { spheres } (lib.rs:611-639) -> packs with mrt_pack_world, then uploads */
int mrt_set_world(mrt_ctx* ctx, const mrt_sphere* spheres, size_t n);
/* New centres and radii for spheres [first, first + count) of the current scene; xyzr = count x (cx, cy, cz, radius).
 * Materials, the sphere count and the hierarchy's grouping stay: the host does O(count) work, and everything derived from the
 * spheres (member records, every level's bounds, the boxes of large scenes, the matrix-core sweep's operand) is recomputed by
 * kernels queued on the ctx's stream.  No buffer is freed or allocated and nothing is built on the host.
 *   Refusals, each before anything is changed or queued: MRT_ERR_NO_SCENE without a scene; MRT_ERR_INVALID_ARG if first + count
 *     exceeds the sphere count or xyzr is NULL with count > 0; MRT_ERR_BAD_SCENE for a value that is not finite or beyond 1e7 in
 *     magnitude (the rule of mrt_set_world_raw).  count == 0: MRT_OK, nothing queued.
 *   Negative radii stay legal (hollow glass): bounds use |r|, the stored radius and -(r r) are the caller's value.
 *   Ordering: frames queued before the call render the old geometry, frames queued after it the new one.  The call does not
 *     wait on the host for the frames in flight; xyzr may be reused as soon as it returns.
 *   The accumulation is not restarted (only mrt_reset does that, as for mrt_set_world); the denoiser's guides are marked stale.
 *   The launch schedule is not restarted and the tile costs stay valid: a caller that updates every frame still reaches a
 *     settled schedule (mrt_get_schedule), and a pinned hint stays as it is.
 *   Regrouping: the bounds only get looser as spheres leave the groups they were built in.  The image never changes, only the
 *     speed; mrt_read_counters' member_tests per world_hit_calls is the signal to watch, and mrt_regroup_spheres regroups --
 *     or mrt_set_auto_regroup has the library judge the bounds itself and regroup when they have loosened.
 *   The matrix-core sweep runs in the world's own space (no per-scene axis scale) after an update; the scaled space comes back
 *     with the next mrt_set_world*.
 *   MRT_ERR_HIP (a launch the runtime refuses) leaves the context without a scene, as a failed mrt_set_world* does. */
int mrt_update_spheres(mrt_ctx* ctx, uint32_t first, uint32_t count, const float* xyzr);
/* New materials for spheres [first, first + count) of the current scene; geometry, the sphere count and the grouping stay.
 * mrt_material is the last five fields of mrt_sphere, same meaning: albedo for Lambertian and Metal, param = fuzz (Metal) | ior
 * (Dielectric).  The host does O(count) work; one scatter is queued on the ctx's stream.
 *   What changes: from the call on the device holds, for these spheres, exactly what a mrt_set_world of the same sphere list
 *     with these materials would hold of what shading reads -- the sphere's type word, and floats 4..7 of its shade record as bit
 *     copies, including what mrt_set_world_raw derives for a Dielectric on the host (1/ior, the two Schlick r0, ior): the build
 *     and this call share one derivation (mrt_debug_material_shade exposes it).  Any material_ty is accepted: 1..3 are the known
 *     types, anything else absorbs, as raw::World allows.  Values are not validated, as the build does not validate them.
 *     The device copies of the SoA material arrays (albedo / fuzz / ior entries, material_idx) are NOT kept up: no kernel reads
 *     them (the render kernel and the denoiser's guide fill read the shade record and the type word alone).
 *   What does not change: geometry and every hierarchy array, bit for bit.  No refit is queued; the per-scene sweep axis scale
 *     stays (unlike after mrt_update_spheres); the camera-ray masks and lists stay built (they are geometry only); the tile
 *     costs, the launch schedule and a pinned hint stay; the auto-regroup policy's update count and statistics stay; the
 *     accumulation and the noise estimate are not restarted (only mrt_reset does that); no buffer, stream or event is created
 *     or freed.
 *   Refusals, each before anything is changed or queued: MRT_ERR_INVALID_ARG for ctx NULL, first + count beyond the sphere count,
 *     materials NULL with count > 0, or a flag bit other than the one defined; MRT_ERR_NO_SCENE without a scene.  count == 0:
 *     MRT_OK, nothing queued.
 *   Ordering: as mrt_update_spheres -- frames queued before the call shade with the old materials, frames queued after it with
 *     the new ones; the call never waits on the host, and materials may be reused as soon as it returns.
 *   The denoiser's guides are marked stale (the albedo guide, and its rule for a Dielectric) and rebuilt at the next denoise.
 *   Temporal reprojection: sphere indices keep their meaning, so the history is kept: a recoloured sphere converges over
 *     max_history steps, or faster with the temporal response on.  With MRT_MATERIALS_RESTART_HISTORY every pixel whose first hit
 *     is one of the updated spheres finds no history at the next mrt_temporal_step (it starts over at length 1 from the current
 *     frame); every other pixel is untouched, bit for bit, and the step after that is an ordinary one.
 *   Shards: works on any shard; every context of a multi-GPU frame must be given the same call, as for mrt_update_spheres.
 *   MRT_ERR_HIP (a launch the runtime refuses) leaves the context without a scene, as for mrt_update_spheres. */
typedef struct { int32_t material_ty; float albedo[3]; float param; } mrt_material;      /* 20 bytes */
enum { MRT_MATERIALS_RESTART_HISTORY = 1u };
int mrt_update_materials(mrt_ctx* ctx, uint32_t first, uint32_t count, const mrt_material* materials, uint32_t flags);
/* The hierarchy's grouping made anew, on the device, from the spheres as they are now: the spheres that share clusters (all but
 * the few far larger than the rest) are permuted over the member slots they occupy -- a kd ordering whose cuts fall on
 * power-of-two blocks of clusters, so that every level's nodes are compact -- and everything derived from the grouping is refitted
 * as after an update.  The sphere count, the slot pattern, every buffer and the host builder's work stay: no buffer is freed or
 * allocated, nothing is built on the host.  The result depends on the geometry and the build's slot pattern alone, not on earlier
 * regroups: a second call changes nothing.
 *   Refusals, each before anything is queued: MRT_ERR_INVALID_ARG for NULL, MRT_ERR_NO_SCENE without a scene.  A scene whose
 *     spheres share at most one cluster (or that was built without clustering): MRT_OK, nothing queued.
 *   Ordering: as mrt_update_spheres -- frames queued before the call render with the old grouping, frames queued after it with
 *     the new one, and the call does not wait on the host for the frames in flight.
 *   The image never depends on the grouping: the framebuffer, the accumulation and the counters samples / world_hit_calls /
 *     rng_draws of every frame are what they would be without the call; node_tests and member_tests are what it lowers.
 *   The tile costs, the launch schedule and a pinned hint stay, and the denoiser's guides stay current (no geometry changed).
 *   The matrix-core sweep runs in the world's own space afterwards, as after an update: a small flat scene loses its per-scene
 *     axis scale until the next mrt_set_world*.
 *   MRT_ERR_HIP (a launch the runtime refuses) leaves the context without a scene, as for mrt_update_spheres. */
int mrt_regroup_spheres(mrt_ctx* ctx);
/* WHEN to regroup, decided by the library (opt-in; off by default, and off every call queues exactly the launches it queues
 * without this and the policy's state is never written).  With the policy on, every check_every-th successful non-empty
 * mrt_update_spheres call queues, behind its scatter, a judgement of the hierarchy and a regroup that runs only if the
 * judgement says so; the refit follows as always.  The decision is made on the device: nothing waits on the host, the host
 * never learns the verdict (mrt_read_regroup_stats reads it, and synchronises), no buffer is created or freed.
 *   The figure: for each level k = 1 .. levels, Q_k = the sum of R^2 (in double, from the records' -R^2) over the level's nodes
 *     whose span begins inside the pool of clustered spheres, never-hit nodes aside; Q = ((Q_1 + Q_2) + ..), in a fixed order of
 *     additions (tests/regroup_policy_ref.py restates it; the device matches it bit for bit).  It depends on the geometry and the
 *     grouping alone -- not on the camera -- so the ranks of a sharded frame decide alike.
 *   The rule: regroup when Q > (double)ratio x Q_ref, Q_ref being Q right after the last regroup (the policy's or the caller's
 *     own mrt_regroup_spheres), or when the policy was turned on, or -- for a scene set with the policy on -- at its first check.
 *   One update stale: the judgement reads the bounds the previous update's refit left, those the last frames were rendered
 *     with, before this update's refit replaces them (so that no second, conditional refit is needed); the regroup itself
 *     orders the spheres as this update leaves them.
 *   check_every 1 .. 1024, ratio finite and >= 1, enabled 0 or 1, size = sizeof(mrt_auto_regroup), reserved 0: anything else is
 *     MRT_ERR_INVALID_ARG with nothing changed.  ctx NULL: mrt_set_auto_regroup checks p only (host only).
 *   The defaults (check_every 8, ratio 1.5) are measured on the animated 10,001-sphere stress scene: check_every is the smallest
 *     power of two at which a check that does not fire costs under 1 % of a step, ratio the fastest of 1.5, 2, 3 and 4
 *     (profiles/animation_rates.txt, section "auto-regroup").
 *   The setting survives mrt_reset, mrt_set_world*, mrt_set_camera and mrt_set_shard; the statistics restart with every
 *     mrt_set_world*.  A scene whose spheres share at most one cluster is never checked: MRT_OK, statistics all zero.
 *   Everything mrt_update_spheres and mrt_regroup_spheres promise holds with the policy on: images, the accumulation and the
 *     counters samples / world_hit_calls / rng_draws never depend on it; tile costs, schedule and hint stay.
 *   MRT_ERR_HIP (a launch the runtime refuses) leaves the context without a scene, as for mrt_update_spheres. */
typedef struct {
    uint32_t size;          /* sizeof(mrt_auto_regroup): the version of this struct */
    uint32_t enabled;       /* 0 (default) | 1 */
    uint32_t check_every;   /* judge the hierarchy at every check_every-th update: 1 .. 1024 */
    float ratio;            /* regroup when Q > ratio x Q_ref: finite, >= 1 */
    uint32_t reserved[4];   /* 0 */
} mrt_auto_regroup;          /* sizeof 32 */
void mrt_auto_regroup_default(mrt_auto_regroup* out);      /* enabled 0 */
int mrt_set_auto_regroup(mrt_ctx* ctx, const mrt_auto_regroup* p);
int mrt_get_auto_regroup(mrt_ctx* ctx, mrt_auto_regroup* out);
typedef struct {
    uint64_t checks, regroups;      /* judgements made / regroups they let run, since mrt_set_world* */
    double q_ref, q_last;           /* Q_ref; Q as the last judgement (or reference taking) saw it */
    double q_level[4];              /* Q_1 .. Q_levels of q_last */
    uint32_t levels, pending;       /* pending 1: the next judgement takes Q_ref instead of deciding */
} mrt_regroup_stats;                /* sizeof 72 */
/* The policy's state as the device holds it; waits for the ctx's stream as mrt_read_counters does.  MRT_ERR_NO_SCENE without a
 * scene; all zeros for a scene that is never checked. */
int mrt_read_regroup_stats(mrt_ctx* ctx, mrt_regroup_stats* out);
/* The AoS -> SoA packing of lib.rs:722-799 (host only, no GPU needed).  Capacities are
 * in elements (vec4: 4 floats each); returns MRT_ERR_TOO_SMALL if any is short.
 * Needs at most 2n vec4, 2n f32, 2n i32. */
int mrt_pack_world(const mrt_sphere* spheres, size_t n, mrt_world* world,
                   float* vec4_data, size_t cap_vec4, size_t* n_vec4,
                   float* f32_data, size_t cap_f32, size_t* n_f32,
                   int32_t* i32_data, size_t cap_i32, size_t* n_i32);

int mrt_set_camera(mrt_ctx* ctx, const mrt_camera* cam);
int mrt_camera_derive(const mrt_camera* cam, mrt_camera_raw* out);   /* host only */

/* Replace the seed texture (Rgba32Uint W x H of lib.rs:397-415): seeds = W*H*4 u32,
 * row 0 = bottom.  Optional: mrt_create already fills it from `seed`. */
int mrt_set_seeds(mrt_ctx* ctx, const uint32_t* seeds, size_t n_u32);
/* This shard's packed rows, local_rows (mrt_shard_info: a multiple of 8, also when world == 1) * W * 4 u32; what the rows
 * >= height hold is unspecified. */
int mrt_read_seeds(mrt_ctx* ctx, uint32_t* out, size_t cap_u32);

/* ------------------------------------------------------------------ frame loop */

/* State::redraw (lib.rs:241-307) minus the present pass: one raytrace pass of
 * samples_per_frame spp into framebuffers.target blended with .secondary, swap,
 * sample_count += 1, framebuffer_weight = min(max_w, n/(n+1)), new rng_shuffle, Locals
 * update.  Asynchronous on the ctx's stream, like a swap chain: consecutive frames overlap on the GPU (2 to 16 in flight,
 * see mrt_get_schedule), and the call returns at once unless that many frames
 * are already queued.
 * BACK-PRESSURE: in that case the call blocks the HOST (polling, with the deadline of mrt_set_wait_timeout) until the render
 * kernel of the oldest frame in flight has completed.  That kernel runs on a side stream of the library and waits only for
 * work queued by EARLIER calls (its slot's previous blend on the ctx's stream, the scene / seed uploads), never for anything
 * the caller submits later -- but a caller that gates the ctx's stream on an event it records only AFTER further mrt_redraw
 * calls can deadlock itself here, and the call must not be made while the ctx's stream is being captured into a graph.
 * The next call's blend is ordered behind this one's on the ctx's stream. */
int mrt_redraw(mrt_ctx* ctx);
/* The launch schedule (no reference counterpart: lib.rs:241-307 has one frame after the other).  A frame's render kernel runs
 * on 1 / div of the persistent waves the chip holds and max(2, div) x mult frames are in flight -- with mult 2, twice the
 * launches the chip holds: frames end out of order, and a queued launch takes every workgroup slot the moment it frees; the
 * library measures its way to a setting over the first frames of a workload.  mrt_get_schedule: out[0] = div, out[1] = mult, out[2] = 1
 * once the setting is final for the current workload (or pinned), out[3] = frames in flight, out[4] = the share the most recent
 * launch really got (1 / out[4]: never narrower than the frames the caller really keeps in flight), out[5] = frames that can run
 * side by side in this process (hardware queues: GPU_MAX_HW_QUEUES; 0 = not measured yet).
 * mrt_set_schedule_hint pins (div, mult) -- e.g. what an earlier run of the same workload settled at, or rank 0's setting on
 * every rank of a multi-GPU run -- so that no trial runs and two runs schedule alike; (0, 0) returns to the measured
 * setting.  div 1..8, mult 1..8, max(2, div) x mult <= 16; the frames in flight are held to out[5] where that has been measured
 * (a process with too few hardware queues).  Takes effect at the next redraw (a change waits for the frames
 * under way); the images are the same whatever the schedule. */
int mrt_get_schedule(mrt_ctx* ctx, uint32_t out[6]);
int mrt_set_schedule_hint(mrt_ctx* ctx, uint32_t div, uint32_t mult);
/* `frames` x mrt_redraw: the same images.  Frames are independent until their blend, so when the (shard of the) image has
 * fewer than about two pixels per GPU lane -- a pixel is one sequential chain of samples, lib.rs:299-306's remedy for that is
 * more frames -- up to 32 consecutive frames of the stream mode share one render launch (also when a frame is very short).
 * Memory: every frame of such a launch parks its colour sums in a layer of its own (16 B per pixel); a launch is held to 1 GiB
 * of them per frame in flight (two), e.g. 32 frames of 1920x1080 or 8 of 3840x2160; the buffers are kept until mrt_destroy. */
int mrt_render(mrt_ctx* ctx, uint32_t frames);
int mrt_sync(mrt_ctx* ctx);
/* Restart accumulation: zero framebuffers, frame counter 0, weight 0, shuffle [0;4] (an overridden shuffle is discarded), counters
 * zero.  Scene, camera, seed texture, samples per frame, RNG mode, shard, noise tracking and the schedule stay; the numbering of
 * presents and noise reports goes on (presented images and unread reports are discarded). */
int mrt_reset(mrt_ctx* ctx);

/* Current Locals (what the NEXT redraw will use) */
int mrt_get_locals(mrt_ctx* ctx, mrt_locals* out);
/* Override the next frame's rng_shuffle (the reference draws it from thread_rng, lib.rs:305): the next frame of any kind -- a
 * redraw, the first frame of mrt_render(k), a subset frame -- and that one only; the frames after it take
 * mrt_frame_shuffle(seed, frames_done) as ever.  A refused call does not use it up. */
int mrt_set_rng_shuffle(mrt_ctx* ctx, const uint32_t shuffle[4]);
int mrt_set_samples_per_frame(mrt_ctx* ctx, uint32_t spp);
int mrt_set_rng_mode(mrt_ctx* ctx, uint32_t mode);          /* MRT_RNG_*; takes effect at the next redraw */
uint32_t mrt_frames_done(mrt_ctx* ctx);

/* host-only helpers exposing the schedule of lib.rs:300-305 */
float mrt_frame_weight(uint32_t frames_done, float max_framebuffer_weight);
void  mrt_frame_shuffle(uint64_t seed, uint32_t frame, uint32_t out[4]);
void  mrt_pixel_seed(uint64_t seed, uint64_t pixel_index, uint32_t out[4]);

/* ------------------------------------------------------------------ output */

/* Geometry of this shard's packed framebuffer: local_rows rows of `width` RGBA f32
 * texels; local row r is global row ((r/8)*world + rank)*8 + r%8 (rows >= height are
 * padding and hold zeros). */
int mrt_shard_info(mrt_ctx* ctx, uint32_t* rank, uint32_t* world, uint32_t* local_rows, uint32_t* width);
/* Device pointer of the most recently rendered framebuffer (local_rows*width*4 floats),
 * for zero-copy hand-off to RCCL / torch.  Valid until the next redraw/destroy. */
void* mrt_framebuffer_device_ptr(mrt_ctx* ctx);
/* Read-back (no reference counterpart; the reference only presents, lib.rs:270-297).
 * world == 1: the full image, height*width*4 floats, row 0 = bottom.
 * world  > 1: this shard's packed rows, local_rows*width*4 floats. */
int mrt_read_framebuffer(mrt_ctx* ctx, float* rgba_out, size_t cap_floats);
int mrt_read_counters(mrt_ctx* ctx, mrt_counters* out);   /* accumulated since create/reset */
/* mrt_counters::rng_draws is a per-lane counter in the kernel's rejection loop (a few VALU instructions per trip); the other
 * counters are wave totals kept on the scalar side.  0 launches the instantiation without it (rng_draws then stops
 * advancing); 1 (default) counts.  Takes effect at the next redraw; the images are the same. */
int mrt_set_draw_counting(mrt_ctx* ctx, int enabled);

/* ------------------------------------------------------------------ present pass
 *
 * The reference's pass 2 of State::redraw (lib.rs:270-297): sample_framebuffer.wgsl draws the accumulated RGBA32F texture onto
 * the window surface, rows flipped (:24), in the surface's 8-bit sRGB format (lib.rs:349-351, :1133).  mrt_present queues the
 * same conversion on the GPU -- colour through the sRGB OETF, alpha linear, both clamped and rounded to 8 bits, bit-identical
 * to mrt_srgb8 (and, for alpha, round(255 clamp(a, 0, 1)), NaN -> 0) for every float -- and an asynchronous copy of the
 * 4-byte pixels into pinned memory the library owns; mrt_present_acquire hands out a finished image without waiting for the
 * frames still in flight.  A caller that presents every frame keeps its frames in flight (mrt_read_framebuffer, the exact-float
 * read-back, waits for them).  Images live in a ring of `depth` entries, each a device staging buffer, a pinned host buffer
 * and an event: automatic depth = the frames in flight + 2 (grown at present time, never shrunk), all entries' pinned bytes
 * held to 256 MB (18 entries of 1920x1080, 7 of 3840x2160).  When every entry but the one the caller holds has a copy still
 * in flight, mrt_present waits for the oldest on the host (bounded, mrt_set_wait_timeout): a ring capped by the budget or by
 * mrt_set_present_ring thus narrows the frames in flight.
 *
 * The linear formats hand out the floats themselves through the same ring, for a caller that needs linear values of every frame
 * without draining the frames in flight (its own tone curve, exact snapshots of a long accumulation, an Rgba16Float surface):
 * no OETF, no clamp, alpha like colour, every source flag and every refusal as for the 8-bit formats.  RGBA32F_LINEAR is a bit
 * copy of the source's texels (a NaN keeps its payload), 16 bytes per pixel, what the mrt_read_* call of the same source
 * returns.  RGBA16F_LINEAR stores mrt_half_bits (image output, below) of every channel, 8 bytes per pixel.  An entry holds
 * rows x width x bytes-per-pixel bytes.  A present whose image is larger than the ring's entries -- a larger source, or the
 * first present of a wider format -- regrows them: the images queued but not acquired are discarded and counted in `dropped`,
 * the call is MRT_ERR_STATE while the caller holds an image (mrt_present_release first), and entries are never shrunk, so they
 * fit the largest format presented so far.  The 256 MB budget holds the depth to max(2, budget / entry bytes): 7 entries of
 * 1920x1080 RGBA32F, 15 of 1920x1080 RGBA16F, 2 of 3840x2160 RGBA32F -- fewer than the frames in flight + 2 a wide launch
 * schedule asks for, so such a ring narrows the frames in flight, as above. */
enum { MRT_PRESENT_RGBA8_SRGB = 1, MRT_PRESENT_BGRA8_SRGB = 2 };   /* Rgba8UnormSrgb / Bgra8UnormSrgb surfaces */
/* the linear formats (values of the same `format` argument; 3 stays invalid) */
#define MRT_PRESENT_RGBA16F_LINEAR 16   /* four IEEE binary16 per pixel, r g b a, 8 bytes (an Rgba16Float surface) */
#define MRT_PRESENT_RGBA32F_LINEAR 32   /* four float32 per pixel, r g b a, 16 bytes: the source's bits */
enum {
    MRT_PRESENT_FLIP_Y = 1,    /* rows top-down, as on the surface (sample_framebuffer.wgsl:24) and in mrt_write_ppm */
    MRT_PRESENT_GATHERED = 2   /* the root's full frame from the latest mrt_gather / mrt_gather_rccl, not this ctx's framebuffer */
};
/* the denoised frame (mrt_read_denoised's image; "denoiser" below), not the framebuffer itself */
#define MRT_PRESENT_DENOISED 8u
/* the temporal image (mrt_read_temporal's; "temporal reprojection" below), not the framebuffer itself */
#define MRT_PRESENT_TEMPORAL 16u
/* the latest gathered frame, denoised on the root (mrt_read_gathered_denoised's image; "multi-GPU" below) */
#define MRT_PRESENT_GATHERED_DENOISED 32u
/* the current diagnostic view (mrt_read_view's image; "diagnostic views" below); 4 and 64 stay undefined */
#define MRT_PRESENT_VIEW 128u
enum { MRT_ACQUIRE_NEWEST = 0, MRT_ACQUIRE_OLDEST = 1 };
typedef struct {               /* 40 bytes */
    uint64_t seq;              /* the present's number on this ctx: 1, 2, ... */
    uint32_t frames_done;      /* mrt_frames_done at the present: the accumulation the image shows */
    uint32_t width, rows, row_bytes;   /* rows of width pixels, row_bytes = 4, 8 (RGBA16F) or 16 (RGBA32F) x width apart */
    uint32_t format, flags;    /* as passed to mrt_present */
    uint32_t dropped;          /* images finished but never acquired since the previous acquire (skipped or overwritten) */
    uint32_t ring_depth;       /* the ring's current depth */
} mrt_present_info;
/* Queues the present of the most recent frame (after mrt_render(k): its last frame) on the ctx's stream, behind that frame's
 * blend, and returns at once unless the ring is full (above).  format: MRT_PRESENT_*_SRGB or MRT_PRESENT_*_LINEAR (any
 * other value: MRT_ERR_INVALID_ARG); flags: MRT_PRESENT_FLIP_Y |
 * MRT_PRESENT_GATHERED | MRT_PRESENT_DENOISED | MRT_PRESENT_TEMPORAL | MRT_PRESENT_GATHERED_DENOISED.  Source rows: world == 1, the `height` image rows; a shard (world > 1), its packed
 * local rows in mrt_read_framebuffer's order (FLIP_Y refused: MRT_ERR_INVALID_ARG); GATHERED, the `height` rows of the root's full
 * frame (MRT_ERR_STATE before the first gather); DENOISED, the `height` rows of the denoised frame, queued on the same stream
 * right before the encode (the guide rebuild if the guides are stale, then the filter; refusals as mrt_read_denoised's, and
 * DENOISED | GATHERED: MRT_ERR_INVALID_ARG); TEMPORAL, the `height` rows of the temporal image, queued the same way (refusals as
 * mrt_read_temporal's; TEMPORAL | DENOISED and TEMPORAL | GATHERED: MRT_ERR_INVALID_ARG); GATHERED_DENOISED, the `height` rows of
 * the latest gathered frame denoised on the root, queued the same way (refusals as mrt_read_gathered_denoised's; with FLIP_Y only:
 * together with GATHERED, DENOISED or TEMPORAL it is MRT_ERR_INVALID_ARG; mrt_present_info::frames_done is then the gather's);
 * VIEW, the `height` rows of the current diagnostic view, queued the same way (refusals as mrt_read_view's; with FLIP_Y only:
 * together with any other source it is MRT_ERR_INVALID_ARG).
 * Must not be called while the ctx's stream is being captured into a graph. */
int mrt_present(mrt_ctx* ctx, int format, uint32_t flags);
/* A finished image: *pixels = rows x row_bytes bytes, valid until mrt_present_release, the next acquire, mrt_reset,
 * mrt_set_shard or mrt_destroy.  MRT_ACQUIRE_NEWEST (a viewer, mailbox): the most recent finished image; older finished ones are
 * skipped (info->dropped).  MRT_ACQUIRE_OLDEST (a capture, FIFO): the oldest; nothing is skipped while the caller keeps at most
 * depth - 1 presents outstanding.  wait == 0: returns MRT_OK with *pixels = NULL when none has finished; wait != 0: polls
 * (bounded) for one that is queued (*pixels = NULL only if none is; NEWEST with an older image
 * finished returns that one at once, it does not wait for a newer one in flight).  MRT_ERR_STATE before the context's first present
 * (numbering and this rule span mrt_reset: after a reset the call is MRT_OK with *pixels = NULL).  info may be
 * NULL.  Releases the image held before.  The bytes are info->format's: the caller reinterprets *pixels as uint16_t
 * (RGBA16F_LINEAR) or float (RGBA32F_LINEAR) texels; the pinned buffer is aligned for either. */
int mrt_present_acquire(mrt_ctx* ctx, int mode, int wait, const uint8_t** pixels, mrt_present_info* info);
int mrt_present_release(mrt_ctx* ctx);            /* MRT_ERR_STATE if no image is held */
/* Pins the ring's depth (2..18, held to the 256 MB budget); 0 = automatic.  Waits (bounded) for the copies in flight and
 * discards the images not yet acquired; MRT_ERR_STATE while the caller holds one. */
int mrt_set_present_ring(mrt_ctx* ctx, uint32_t depth);

/* ------------------------------------------------------------------ noise estimate (no reference counterpart)
 *
 * Frames are independent draws (each has its own rng_shuffle, lib.rs:305).  With noise tracking on, the blend also keeps, per
 * framebuffer texel, S: the weighted population variance of the frames' mean luminances, by West's recursion with the blend's
 * own weights w (float32, in this order):
 *     lum(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b
 *     d      = lum(mean) - lum(prev.rgb)                  prev = the framebuffer texel the blend reads
 *     S'     = (w == 0.0f) ? 0.0f : w * (S + (1.0f - w) * (d * d))
 * The host tracks c2 = sum of the squared normalised frame weights in double, from the float weights actually used:
 * c2' = w^2 c2 + (1 - w)^2, 1 at w == 0.  The estimated variance of the displayed luminance is S * K, K = c2 / (1 - c2):
 * 1 / (n - 1) for uniform accumulation (max_framebuffer_weight 1), -> (1 - w) / (2 w) for the EMA at a saturated weight w,
 * +inf for n < 2 ("no estimate yet": rmse = rel_rmse = max_se = +inf, every finite pixel is above the threshold).
 * Per finite pixel of a report, in float32: var = S * (float)K, se = sqrtf(var), L = lum(framebuffer), rel = se / fmaxf(L, floor),
 * above = rel > threshold; a pixel whose S or L is not finite counts in non_finite only.
 * Assumptions: a caller who pins the same shuffle for every frame (mrt_set_rng_shuffle) makes the frames identical and the
 * estimate reads 0; mrt_set_camera / mrt_set_world do not restart the accumulation (mrt_reset does), so after such a change
 * without a reset the image blends two pictures and the estimate counts their difference as noise ("not converged"). */
typedef struct {                 /* 96 bytes */
    uint64_t seq;                /* the query's number on this ctx: 1, 2, ...; 0 = no report */
    uint32_t frames_done;        /* mrt_frames_done at the query: the accumulation the report describes */
    uint32_t reserved;           /* the kind of this report's tile map (mrt_noise_query_map): 0 for mrt_noise_query's */
    uint64_t pixels;             /* finite pixels (image rows of this ctx; shard padding excluded) */
    uint64_t non_finite;         /* pixels whose S or luminance is NaN / Inf (in nothing else) */
    uint64_t above;              /* finite pixels with rel > threshold */
    float threshold, floor;      /* as passed to mrt_noise_query */
    double noise_factor;         /* K */
    double sum_var;              /* sum of S * K over the finite pixels (double) */
    double sum_lum;              /* sum of L over the finite pixels */
    double rmse;                 /* sqrt(sum_var / pixels) */
    double rel_rmse;             /* rmse / (sum_lum / pixels) */
    float max_se;                /* the largest se */
    uint32_t reserved2;
} mrt_noise_report;
/* Turns noise tracking on (allocates S, zeroed) or off (frees it).  Only while mrt_frames_done == 0 (after mrt_create or
 * mrt_reset), else MRT_ERR_STATE; a call that changes nothing is MRT_OK, one that does discards the unread reports.  Tracking survives mrt_reset (S is zeroed with the framebuffers, unread reports are
 * discarded) and mrt_set_shard (S is reallocated for the new shard's rows, zeroed). */
int mrt_set_noise_tracking(mrt_ctx* ctx, int enabled);
/* Queues the noise report of the most recent frame on the ctx's stream, behind that frame's blend -- the reduction and a copy
 * into pinned memory the library owns -- and returns at once.  Reports live in a ring of 8; when the oldest is still in
 * flight the call waits for it (bounded, mrt_set_wait_timeout).  rel_threshold, rel_floor: finite, rel_floor >= 0.
 * MRT_ERR_STATE if tracking is off.  Must not be called while the ctx's stream is being captured into a graph. */
int mrt_noise_query(mrt_ctx* ctx, float rel_threshold, float rel_floor);
/* mrt_noise_query with the kind of tile map the report's ring entry gets.  MRT_TILE_MAP_MAX_REL is mrt_noise_query exactly: the
 * same launches, the same bits.  MRT_TILE_MAP_SUM_S differs in one way only: every scalar field of the report is bit for bit
 * what kind 0 gives on the same state (uniform or per-tile, a shard, K = +inf), and the map entry of tile t is (float)s_t, s_t the
 * tile's summed S in double: a pixel counts if it is inside the image (shard padding rows excluded) and its S and
 * lum(framebuffer) are finite -- the report's own rule -- and contributes (double)S_p, any other pixel +0.0; per tile row the
 * eight columns are added as ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), then the eight row sums one after the other
 * from the tile's bottom row, starting at 0.0.  No K and no n_t enter it: s_t * K(n_t) is the tile's summed variance in a
 * uniform and in an adaptive accumulation alike (mrt_budget_allocate).  The report's `reserved` field holds map_kind.  Any other
 * map_kind: MRT_ERR_INVALID_ARG; everything else as mrt_noise_query. */
enum { MRT_TILE_MAP_MAX_REL = 0, MRT_TILE_MAP_SUM_S = 1 };
int mrt_noise_query_map(mrt_ctx* ctx, float rel_threshold, float rel_floor, uint32_t map_kind);
/* The newest finished report.  wait == 0: out->seq == 0 when none has finished; wait != 0: polls (bounded) for the newest
 * queued report first.  Never waits for frames queued after that query.  out->seq == 0 before the first query. */
int mrt_noise_result(mrt_ctx* ctx, int wait, mrt_noise_report* out);
/* S in mrt_read_framebuffer's texel order (world 1: height rows of width; a shard: its packed local rows), one float per
 * texel; synchronises as mrt_read_framebuffer does.  MRT_ERR_STATE if tracking is off. */
int mrt_read_noise(mrt_ctx* ctx, float* out, size_t cap);
/* The tile map of the latest queued query, whatever its kind -- the per-8x8-tile maximum of rel (mrt_noise_query,
 * MRT_TILE_MAP_MAX_REL) or the tile's summed S (MRT_TILE_MAP_SUM_S; that query's report names the kind in `reserved`) -- as
 * tiles_rows rows of tiles_x (tile = band x tiles_x + column, a shard's packed bands); waits for that query only.
 * MRT_ERR_STATE before the first query. */
int mrt_read_noise_tiles(mrt_ctx* ctx, float* out, size_t cap, uint32_t* tiles_x, uint32_t* tiles_rows);
/* Host only: K after frames_done uninterrupted frames with the weights of mrt_frame_weight (+inf for frames_done < 2). */
double mrt_noise_factor(uint32_t frames_done, float max_framebuffer_weight);

/* ------------------------------------------------------------------ adaptive sampling (no reference counterpart)
 *
 * More frames where the noise estimate says the image is still noisy.  Tiles are the 8x8 tiles of mrt_read_noise_tiles:
 * tile = band * tiles_x + column, band = row / 8, row 0 at the bottom.  Each tile has a frame count n_t: the frames blended into
 * it since mrt_create or mrt_reset.
 *   Subset frame: renders every pixel of the listed tiles at samples_per_frame and blends them.  It takes the next frame number
 *     as mrt_redraw does (frames_done += 1, shuffle mrt_frame_shuffle(seed, frames_done)).  In tile t the blend weight is
 *     w = mrt_frame_weight(n_t, max_framebuffer_weight), the weight a uniform accumulation of n_t frames would use; S is updated
 *     with the same w by the noise estimate's recursion; then n_t += 1 (saturating).  Tiles not listed keep their framebuffer
 *     texels and S bit for bit.
 *   Divergence: until the first subset frame of an accumulation every n_t == frames_done and nothing differs from a uniform
 *     accumulation.  After it, mrt_redraw / mrt_render frames are whole frames blended per tile; mrt_reset returns to the
 *     uniform state.
 *   Noise reports after divergence: per finite pixel var_p = S_p * (float)K(n_t), K(n) = mrt_noise_factor(n, max_w) (K = +inf:
 *     se_p = +inf); se, rel, above and the tile map follow as before; sum_var = sum of S_p * K(n_t) in double; noise_factor = the
 *     largest K over the tiles (the least-sampled tile's).  Before divergence reports are unchanged.
 *   Denoising after divergence (mrt_read_denoised, MRT_PRESENT_DENOISED) is refused with MRT_ERR_STATE unless
 *   mrt_set_denoise_adaptive has turned the per-tile filter on ("denoiser" below, "Adaptive accumulations"); presents and
 *   read-backs work unchanged.  Shards (world > 1) are refused with MRT_ERR_STATE. */
/* Queues `frames` consecutive subset frames over the n tiles of `tiles` (asynchronous, with mrt_render's back-pressure).
 * n == 0 or frames == 0: MRT_OK, nothing queued (before any other check).  An id >= the tile count, a duplicate id or tiles == NULL: MRT_ERR_INVALID_ARG; a shard:
 * MRT_ERR_STATE; no scene: MRT_ERR_NO_SCENE; counter-RNG mode with samples_per_frame > MRT_COUNTER_BLOCK: MRT_ERR_INVALID_ARG.
 * A list of every tile renders whole frames: while the accumulation is uniform, exactly mrt_render's. */
int mrt_render_tiles(mrt_ctx* ctx, const uint32_t* tiles, size_t n, uint32_t frames);
/* Selects the tiles whose tile-map entry in one noise report is > that report's threshold (the tiles holding a pixel counted in
 * its `above`) and renders `frames` subset frames over them (mrt_render_tiles).  report_seq == 0: the newest finished report
 * whose map holds the maximum of rel (MRT_TILE_MAP_MAX_REL: reports of mrt_noise_query_map's other kind are passed over),
 * without waiting (none finished: every tile); report_seq == k: report k, waiting (bounded) for that query only.  A report not
 * queued, older than the ring of 8, or of the kind MRT_TILE_MAP_SUM_S: MRT_ERR_STATE; tracking off: MRT_ERR_STATE.  *used_seq = the report used (0: none),
 * *tiles_selected = the selection's size (either may be NULL).  No tile selected: MRT_OK and nothing queued (converged). */
int mrt_render_adaptive(mrt_ctx* ctx, uint32_t frames, uint64_t report_seq, uint64_t* used_seq, uint32_t* tiles_selected);
/* n_t per tile, tiles_rows rows of tiles_x (frames_done everywhere while the accumulation is uniform); synchronises as
 * mrt_read_framebuffer does. */
int mrt_read_tile_frames(mrt_ctx* ctx, uint32_t* out, size_t cap, uint32_t* tiles_x, uint32_t* tiles_rows);

/* ---- adaptive sampling by budget: a fixed number of tile-frames, spent where they lower the estimated variance most ----
 * Model: a tile with n frames shows the summed variance s_t * K(n), s_t its entry in a MRT_TILE_MAP_SUM_S map and K(n) =
 * mrt_noise_factor(n, max_framebuffer_weight) in double.  One tile-frame is one subset frame over one tile.
 *
 * mrt_budget_allocate (host only) gives tile t k_t of at most `budget` tile-frames, k_t <= max_frames:
 *   s'_t = s[t], a NaN or a negative value read as 0.  Candidate (t, j), j = 0 .. max_frames - 1, is tile t's j-th extra frame.
 *   Mandatory frames come first and cost 1 each: a tile with n[t] < 2 (K = +inf: no estimate yet) gets m_t = min(2 - n[t],
 *     max_frames) of them (m_t = 0 for the others), served in the order j ascending, then t ascending, until the budget ends.
 *   Gains, for a tile with n[t] + m_t >= 2 and j >= m_t:  g(t, j) = s'_t * (K(n[t] + j) - K(n[t] + j + 1)) -- one difference, one
 *     product, in double -- and g'(t, j) = the minimum of g(t, i) over m_t <= i <= j, which never increases with j.  Only
 *     candidates with g' > 0 and a finite s'_t count.
 *   Selection: what is left of the budget takes that many candidates in the order g' descending, then j ascending, then t
 *     ascending (all of them if there are fewer).  k_t = the candidates of tile t taken, its mandatory frames included: a prefix
 *     in j by construction.
 *   Result: tile_frames = the sum of k_t; tiles = the tiles with k_t > 0; frames = the largest k_t; var_before = the sum of
 *     s'_t * K(n[t]) and var_after = the sum of s'_t * K(n[t] + k_t), both over the tiles with n[t] >= 2 (K finite before and
 *     after), t ascending, in double; size = sizeof(mrt_budget_result); used_seq and the reserved words 0.
 *   tiles >= 1, max_frames 1 .. 32, every n[t] <= 2^24, max_framebuffer_weight finite and > 0; s, n,
 *   k_out or res NULL or a value outside these: MRT_ERR_INVALID_ARG with nothing written.  The sums are over the tiles as given:
 *   the caller's maps need not be a context's.
 *
 * mrt_render_budget allocates from one MRT_TILE_MAP_SUM_S report and renders the allocation through mrt_render_tiles.
 *   The report: mrt_render_adaptive's rule over the reports of that kind.  report_seq == 0: the newest finished one, without
 *     waiting; none: MRT_OK, nothing queued, res->used_seq 0.  report_seq == k: report k, waiting (bounded) for that query only;
 *     a report not queued, older than the ring of 8, or of the kind MRT_TILE_MAP_MAX_REL: MRT_ERR_STATE.  Tracking off:
 *     MRT_ERR_STATE.
 *   The allocation: mrt_budget_allocate(s = that report's map, n = the host's current n_t -- mrt_frames_done everywhere while
 *     the accumulation is uniform --, the ctx's max_framebuffer_weight, budget, max_frames).  The map is as old as its report:
 *     frames queued since the query are in n but not in s.
 *   The frames: L_j = {t : k_t >= j} in ascending tile id, j = 1 .. the largest k_t; consecutive j with the same list are one
 *     mrt_render_tiles(L_j, run length) call, so that those frames share a launch.  A list of every tile renders whole frames
 *     (mrt_render_tiles' rule): a budget that gives every tile the same count leaves a uniform accumulation uniform.  The
 *     framebuffer, S, n_t, mrt_frames_done and the counters are exactly those of that sequence of mrt_render_tiles calls.
 *   Every refusal of mrt_render_tiles applies and is returned before anything is queued: a shard (MRT_ERR_STATE), no scene
 *     (MRT_ERR_NO_SCENE), counter-RNG mode above MRT_COUNTER_BLOCK samples per frame (MRT_ERR_INVALID_ARG).  max_frames outside
 *     1 .. 32: MRT_ERR_INVALID_ARG.  budget == 0, or no candidate with a gain and no mandatory frame: MRT_OK, nothing queued.
 *   *res (may be NULL) = the allocation's result with used_seq = the report used; k_out (may be NULL; cap >= the tile count,
 *     else MRT_ERR_TOO_SMALL) = k_t per tile.  The call creates nothing of its own: the report's map is read back as
 *     mrt_render_adaptive reads it. */
typedef struct {
    uint32_t size;               /* sizeof(mrt_budget_result), written by the library */
    uint32_t frames;             /* the largest k_t: the subset frames the allocation takes */
    uint32_t tiles;              /* tiles with k_t > 0 */
    uint32_t reserved0;          /* 0 */
    uint64_t tile_frames;        /* the sum of k_t (<= budget) */
    uint64_t used_seq;           /* mrt_render_budget: the report used (0: none); mrt_budget_allocate: 0 */
    double var_before, var_after;
    uint32_t reserved[4];        /* 0 */
} mrt_budget_result;             /* sizeof 64 */
int mrt_budget_allocate(const float* s, const uint32_t* n, size_t tiles, float max_framebuffer_weight, uint64_t budget,
                        uint32_t max_frames, uint32_t* k_out, mrt_budget_result* res);
int mrt_render_budget(mrt_ctx* ctx, uint64_t budget, uint32_t max_frames, uint64_t report_seq, mrt_budget_result* res,
                      uint32_t* k_out, size_t cap);

/* ---- budget allocation on the device: plan with the query, render the plan ----
 * mrt_noise_query_budget is mrt_noise_query_map(ctx, rel_threshold, rel_floor, MRT_TILE_MAP_SUM_S) exactly -- the same launches,
 * the same report bits, `reserved` = 1; mrt_render_budget and mrt_read_noise_tiles use the report as before -- and queues, on the
 * ctx's stream behind the reduction and ahead of the report's copy, the allocation of `budget` tile-frames from the map the query
 * has just written: the report carries a plan, finished when the report is.  Nothing waits on the host.
 *   The plan: k_t = mrt_budget_allocate(s = the report's map, n, the ctx's max_framebuffer_weight, budget, max_frames)'s, bit for
 *     bit, with n = n_q: the n_t of every frame queued before the call and of none after (mrt_frames_done everywhere while the
 *     accumulation is uniform).  The device selects it as one total order: candidate (t, j) has the key (class, G, j, t), class 0
 *     a mandatory frame (n_t + j < 2 and j < min(2, max_frames); G = 0), class 1 a gain with G = the bits of g'(t, j) as an
 *     unsigned 64-bit integer, complemented; ascending keys are mrt_budget_allocate's order, the keys are unique, and the plan is
 *     the `budget` smallest (all if there are fewer).  It does not depend on launch shape, dispatch order or timing.
 *   The result: tile_frames, tiles and frames are mrt_budget_allocate's.  var_before and var_after are its sums in a blocked
 *     order: per tile a_t = s'_t * K(n_t) (var_before) or s'_t * K(n_t + k_t) (var_after), +0.0 for a tile with n_t < 2; P_b = the
 *     sequential sum from 0.0 of a_t over t = 64 b .. 64 b + 63, ascending; the field = the sequential sum from 0.0 of P_b over
 *     ascending b.  (mrt_budget_allocate adds all tiles in one chain; the two agree to rounding.)
 *   Refusals, each before anything is queued: mrt_noise_query_map's; max_frames outside 1 .. 32: MRT_ERR_INVALID_ARG; a shard:
 *     MRT_ERR_STATE; an n_t above 2^24: MRT_ERR_INVALID_ARG.  budget == 0 is legal: a plan of zeros.  Must not be called while
 *     the ctx's stream is being captured.  The call may grow the device's table of K(n) first, which waits (bounded) for the
 *     ctx's stream: a handful of times per accumulation, as for a noise query of a diverged accumulation.
 * mrt_read_budget_plan returns the plan of report `report_seq` as allocated: k_out (may be NULL; cap >= the tile count, else
 *   MRT_ERR_TOO_SMALL) and *res (may be NULL) with used_seq = the report.  report_seq == 0: the newest finished report that
 *   carries a plan, without waiting; none: MRT_OK, res->used_seq 0, k_out zeroed.  report_seq == k: report k, waiting (bounded)
 *   for that query only; a report that is not held (not queued, older than the ring of 8, discarded by mrt_reset) or that
 *   carries no plan: MRT_ERR_STATE.  Tracking off: MRT_ERR_STATE.  It reads back k_t and the 64-byte result, nothing else.
 * mrt_render_planned reads the plan as mrt_read_budget_plan does and renders it as mrt_render_budget renders its allocation.
 *   A plan is a target: tile t should reach n_q[t] + k_t frames, and frames queued since the query count towards it:
 *     k'_t = max(0, n_q[t] + k_t - n_now[t]), n_now the host's n_t at this call; with nothing queued in between k' = k.
 *   The frames: L_j = {t : k'_t >= j} in ascending tile id; consecutive equal lists are one mrt_render_tiles call; a list of
 *     every tile renders whole frames.
 *   k_out and *res report k' and its tile_frames, tiles and frames; var_before and var_after stay the plan's.
 *   Every refusal of mrt_render_tiles applies before anything is queued (mrt_render_budget's list).  Nothing to render -- no
 *     plan finished, or a plan already met --: MRT_OK. */
int mrt_noise_query_budget(mrt_ctx* ctx, float rel_threshold, float rel_floor, uint64_t budget, uint32_t max_frames);
int mrt_read_budget_plan(mrt_ctx* ctx, uint64_t report_seq, uint32_t* k_out, size_t cap, mrt_budget_result* res);
int mrt_render_planned(mrt_ctx* ctx, uint64_t report_seq, mrt_budget_result* res, uint32_t* k_out, size_t cap);

/* ------------------------------------------------------------------ denoiser (no reference counterpart)
 *
 * A variance-guided edge-aware a-trous filter (the spatial filter of SVGF; for a static picture the accumulation is its temporal
 * part, for a moving one "temporal reprojection" below is) over the most recent frame, for a preview of a progressive render.  It needs noise tracking (mrt_set_noise_tracking: var = S * K below) and an
 * unsharded context (world == 1: a shard's rows are interleaved bands without spatial neighbours); else MRT_ERR_STATE.
 *
 * Guides, per pixel, from ONE ray through the mean of the render's sample positions: the camera ray of u = v = 0.5
 * (fs_main :373-381) through the look-at camera's lens centre (no defocus offset), normalised as the render normalises (MRT-F32),
 * and its closest hit over [0.001, 1e4) found by the render kernel's own sweep and walk (mrt_debug_world_hit's):
 *     index   the sphere hit, -1 on a miss
 *     t       the hit's distance; +inf on a miss
 *     normal  sphere_hit's normal facing the ray: (o + t d - centre) / radius, negated unless dot(normal, d) <= 0; -d on a miss
 *     albedo  Lambertian / Metal: the material's albedo; Dielectric: (1, 1, 1); an unknown type: (0, 0, 0); a miss: (1, 1, 1)
 * They are marked stale by mrt_set_camera, mrt_set_world* and mrt_set_shard and rebuilt, queued on the ctx's stream, at the next
 * denoise (no host wait).
 *
 * Filter (float32, in this order; only + - * /, sqrtf, fminf, fmaxf).  Per texel, c = (r, g, b) and var: iteration 0 reads the
 * framebuffer and var = S * (float)K.  Iteration i (0 .. iterations - 1) has step h = 2^i and taps q = p + h (dx, dy), dy then dx
 * from -2 to 2, with k = {1/16, 1/4, 3/8, 1/4, 1/16}; a tap outside the image or not finite (a channel of c or var) is skipped:
 *     tukey(x)   = x < 1 ? (1 - x * x)^2 : 0
 *     L(c)       = (0.2126f * r + 0.7152f * g) + 0.0722f * b
 *     w_lum      = tukey(|L_p - L_q| * (1 / (sigma_l * sqrtf(var_p) + 1e-6f)))           (1 when K = +inf)
 *     w_normal   = max(0, (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z), squared normal_exp times
 *     w_depth    = 1 if both miss, 0 if exactly one does, else tukey(|t_p - t_q| * (1 / (sigma_z * t_p)))
 *     w_albedo   = tukey(max(|dr|, |dg|, |db|) * (1 / sigma_a))
 *     w          = ((((k_x * k_y) * w_lum) * w_normal) * w_depth) * w_albedo;  the centre tap: k_2 * k_2 = 9/64, no stops
 *     c'  = sum w c_q / sum w,   var' = sum (w * w) var_q / (sum w * sum w)     (sums in tap order, from 0)
 * Passed through unchanged (c and var): a texel that is not finite, and -- K finite only -- a texel whose var is 0.  K = +inf (fewer
 * than 2 frames) has no luminance stop and var = 0 for every finite S (no 0 * inf is formed).  Alpha is the framebuffer's.
 *
 * Variance modes (mrt_set_denoise_variance; the default, MRT_DENOISE_VAR_ACCUMULATED, is exactly the filter above).  A 2- to
 * 4-frame variance estimate of ONE pixel is nearly worthless, and the luminance stop is scaled by it; both estimates below are
 * float32 in the stated order with the same operations.
 *   Prefilter (PREFILTERED and SPATIAL_EARLY; every iteration; only when a luminance stop exists).  For a texel p that is finite
 *   in iteration i's input: taps q = p + (dx, dy), dy then dx from -1 to 1 -- distance 1 whatever the iteration's step -- with
 *   k3 = {1/4, 1/2, 1/4}; a tap outside the image or whose c or var is not finite is skipped:
 *     g_p   = (sum (k3[dx] * k3[dy]) * var_q) / (sum k3[dx] * k3[dy])                  (both sums in tap order, from 0)
 *     w_lum = tukey(|L_p - L_q| * (1 / (sigma_l * sqrtf(g_p) + 1e-6f)))
 *   g_p replaces var_p in the luminance stop and in the pass-through rule (a finite texel passes through when g_p == 0, not when
 *   its own var is 0).  The propagated variance is unchanged: var' = sum (w * w) var_q / (sum w * sum w) over the unfiltered var_q.
 *   With K = +inf there is no luminance stop and no prefilter: PREFILTERED is then bit for bit ACCUMULATED.
 *   Spatial initial variance (SPATIAL_EARLY, while mrt_frames_done < spatial_frames; 1 frame, where K = +inf, included).  It
 *   replaces S * K as iteration 0's variance, and the luminance stop is on.  For a texel p whose colour and S are finite: taps
 *   q = p + (dx, dy), dy then dx from -3 to 3; a tap outside the image or whose colour or S is not finite is skipped; the weights
 *   are the filter's own stops with the ctx's parameters, the centre tap's weight is 1:
 *     w_q   = (w_normal * w_depth) * w_albedo
 *     m0    = sum w_q;   m1 = sum w_q * L_q;   mean = m1 / m0
 *     m2    = sum w_q * ((L_q - mean) * (L_q - mean))                                   (a second pass over the same taps)
 *     var_p = m2 / m0
 *   A texel with a finite S and a colour that is not finite gets var 0; a texel whose S is not finite keeps S as its var: both
 *   pass through as above.  From frames_done >= spatial_frames on, SPATIAL_EARLY is PREFILTERED.
 *
 * Adaptive accumulations (mrt_set_denoise_adaptive; off by default, and then a denoise after divergence is refused).  After the
 * first subset frame every tile has its own n_t, hence its own K.  With the setting on the filter is defined per pixel, float32
 * in the stated order with the same operations.  For pixel p = (x, y) of tile t = (y / 8) * tiles_x + x / 8:
 *     n_p       = n_t
 *     K_p       = (float)mrt_noise_factor(n_p, max_framebuffer_weight), as the per-tile noise report takes it (+inf for n_p < 2)
 *     spatial_p = the mode is SPATIAL_EARLY and n_p < spatial_frames           (n_p in the place of mrt_frames_done)
 *     stop_p    = spatial_p, or K_p finite                                      (constant over the iterations)
 *   Iteration 0's variance: with spatial_p the spatial initial variance above, unchanged -- its taps need a finite colour and S,
 *   whatever their own tile's count; otherwise S_p * K_p for a finite K_p; otherwise 0 for a finite S_p and S_p itself if it is
 *   not finite (no 0 * inf is formed).
 *   Every iteration, for the centre p: without stop_p, w_lum = 1 for all its taps, no prefilter, and a variance of 0 does not pass
 *   through (only a texel that is not finite does); with stop_p, the luminance stop and the pass-through rule above, and in
 *   PREFILTERED / SPATIAL_EARLY g_p -- over the 3 x 3 finite taps var_q, whatever their tiles' stop -- replaces var_p in both.  A
 *   tap's own stop is never read: the centre decides.  The propagated variance, the centre tap, skipped taps and alpha are as
 *   above.
 *   A tile with n_t = 0 (black, S = 0, no stop) is therefore not left black: its neighbours' colour is filtered into it through
 *   the edge stops alone, as far as the taps reach (in SPATIAL_EARLY it is in its spatial phase and has a stop: its estimate is 0
 *   over a black tile, so its interior passes through until its border has been filled).  When every n_t equals n, the image is bit for bit the uniform filter's for n frames in the same mode.
 *   The first such denoise, and the first after a tile has passed the K table's length, may wait once (bounded) for the ctx's
 *   stream while the device's table of K(n) is made (the table of the per-tile noise report; nothing else is created).
 *
 * Blend with the accumulation (mrt_set_denoise_mix; off by default, and then every launch and bit is what it is without it).  The
 * filter trades noise for bias, and the accumulation's noise falls with the frame count while the filter's bias does not: from
 * some count on -- scene dependent -- the accumulated image is the better one.  With the setting on, one more pass behind the last
 * iteration mixes the two per pixel by how much of their difference the noise estimate explains (a local Wiener shrinkage): where
 * the noise dominates the result is the filter, where the filter's bias dominates it is the accumulation.  Float32 in this order;
 * only + - * /, fminf, fmaxf and comparisons.  Per pixel p:
 *     c_p          the input frame's texel (the framebuffer, or the gathered frame)
 *     (f_p, u_p)   the colour and the propagated variance of the last iteration, before alpha replaces the variance
 *     v_p        = S_p * (float)K, the accumulated estimate in every variance mode; an adaptive accumulation: S_p * K_p
 *     d_p        = L(f_p) - L(c_p)
 *     n_p        = fmaxf(v_p - u_p, 0.0f)
 *     valid_p    = r, g, b of c_p, S_p, r, g, b of f_p and u_p are all finite (an adaptive accumulation: and K_p is finite)
 *   n_p is the noise variance of f - c: an averaging filter contains its own centre, so Var(f - c) = v - u, not v + u.  Window:
 *   the 5 x 5 pixels q around p, dy then dx from -2 to 2, the centre included; q counts if it lies inside the image, valid_q holds
 *   and the guides' sphere-index bits of q equal those of p.  In tap order, from 0: e += d_q * d_q, m += n_q.
 *     a          = e > 0.0f ? fminf(m / (gain * e), 1.0f) : 0.0f
 *     out.rgb    = c_p + a * (f_p - c_p)        (per channel);   out.a = the frame's alpha
 *   A pixel that is not valid gets out.rgb = f_p (the filter has passed it through, or it has no v).  Where K = +inf (fewer than 2
 *   frames) there is no v: the image is the filter's, and for a uniform accumulation the launches are exactly those without the
 *   setting.  gain: the luminance stop picks neighbours that resemble the noisy centre, so f follows c's noise and d^2
 *   underestimates the true difference; gain corrects that (default 1: the smallest worst case over profiles/denoise_mix_quality.txt).
 *   It applies to every denoise of an accumulation -- mrt_read_denoised, MRT_PRESENT_DENOISED, mrt_read_gathered_denoised and
 *   MRT_PRESENT_GATHERED_DENOISED (with the gather's snapshot of K), the per-tile filter -- and not to the temporal image, whose
 *   history has no accumulated alternative: mrt_read_temporal and MRT_PRESENT_TEMPORAL stay bit for bit.  It needs no buffer, stream
 *   or event of its own (the pass reads the filter's idle scratch), and every refusal of every denoise is what it is without it. */
typedef struct {                 /* 48 bytes */
    uint32_t size;               /* sizeof(mrt_denoise_params): the version of this struct */
    uint32_t iterations;         /* 1 .. 8 (default 5: steps 1 .. 16) */
    float sigma_l;               /* luminance stop, in standard deviations: finite, > 0 (default 8) */
    uint32_t normal_exp;         /* 0 .. 16 squarings: w_normal = dot^(2^normal_exp) (default 7: dot^128) */
    float sigma_z;               /* relative distance stop: finite, > 0 (default 0.05) */
    float sigma_a;               /* albedo stop: finite, > 0 (default 0.1) */
    uint32_t reserved[6];        /* 0 */
} mrt_denoise_params;
/* Host only: the defaults. */
void mrt_denoise_params_default(mrt_denoise_params* out);
/* The parameters every later denoise of this ctx uses (MRT_ERR_INVALID_ARG outside the ranges above, size or reserved wrong).
 * ctx NULL: checks the parameters only (host only). */
int mrt_set_denoise_params(mrt_ctx* ctx, const mrt_denoise_params* params);
int mrt_get_denoise_params(mrt_ctx* ctx, mrt_denoise_params* out);
/* Where the luminance stop's variance comes from ("Variance modes" above). */
enum { MRT_DENOISE_VAR_ACCUMULATED = 0,   /* default: var = S * K, the filter above exactly */
       MRT_DENOISE_VAR_PREFILTERED = 1,
       MRT_DENOISE_VAR_SPATIAL_EARLY = 2 };
/* mode 0 .. 2; spatial_frames 1 .. 64 in every mode (default 3; only SPATIAL_EARLY reads it).  Anything else, or ctx NULL:
 * MRT_ERR_INVALID_ARG, nothing changed.  The setting lives as long as the denoise parameters do (it survives mrt_reset,
 * mrt_set_shard, mrt_set_world* and mrt_set_camera), takes effect at the next denoise and creates no resource.  Every refusal of
 * a denoise holds in every mode. */
int mrt_set_denoise_variance(mrt_ctx* ctx, uint32_t mode, uint32_t spatial_frames);
int mrt_get_denoise_variance(mrt_ctx* ctx, uint32_t* mode, uint32_t* spatial_frames);   /* either pointer may be NULL */
/* Whether an adaptive accumulation is denoised ("Adaptive accumulations" above) or refused; off by default.  On, mrt_read_denoised
 * and MRT_PRESENT_DENOISED of a diverged accumulation run the per-tile filter instead of returning MRT_ERR_STATE; every other
 * refusal stays (tracking off, a shard, no scene, DENOISED | GATHERED, the gathers' refusal of an adaptive accumulation,
 * everything temporal), and an accumulation that has not diverged is denoised exactly as with the setting off: the same launches,
 * the same bits.  The setting creates nothing, lives as long as the denoise parameters do (it survives mrt_reset, mrt_set_shard,
 * mrt_set_world* and mrt_set_camera) and takes effect at the next denoise.  ctx NULL, or enabled NULL: MRT_ERR_INVALID_ARG. */
int mrt_set_denoise_adaptive(mrt_ctx* ctx, int enabled);
int mrt_get_denoise_adaptive(mrt_ctx* ctx, int* enabled);
/* The blend with the accumulation ("Blend with the accumulation" above). */
typedef struct {
    uint32_t size;               /* sizeof(mrt_denoise_mix): the version of this struct */
    uint32_t enabled;            /* 0 (default) | 1 */
    float gain;                  /* finite, 0.25 .. 16 (default 1: profiles/denoise_mix_quality.txt) */
    uint32_t reserved[5];        /* 0 */
} mrt_denoise_mix;               /* sizeof 32 */
/* Host only: the defaults (enabled 0). */
void mrt_denoise_mix_default(mrt_denoise_mix* out);
/* Anything out of range, size or reserved wrong: MRT_ERR_INVALID_ARG with nothing changed.  ctx NULL: checks p only (host only).
 * The setting creates nothing, takes effect at the next denoise and lives as long as the denoise parameters do (it survives
 * mrt_reset, mrt_set_shard, mrt_set_world* and mrt_set_camera). */
int mrt_set_denoise_mix(mrt_ctx* ctx, const mrt_denoise_mix* p);
int mrt_get_denoise_mix(mrt_ctx* ctx, mrt_denoise_mix* out);
/* Denoises the most recent frame (queued on the ctx's stream behind its blend) and reads it back: height * width * 4 floats,
 * row 0 = bottom, as mrt_read_framebuffer; synchronises as mrt_read_framebuffer does.  MRT_ERR_STATE with tracking off or on a
 * shard, or after divergence without mrt_set_denoise_adaptive; MRT_ERR_NO_SCENE without a scene. */
int mrt_read_denoised(mrt_ctx* ctx, float* rgba_out, size_t cap_floats);

/* ------------------------------------------------------------------ temporal reprojection (no reference counterpart)
 *
 * The accumulation assumes a static picture: after mrt_update_spheres or mrt_set_camera it blends two pictures, and a caller who
 * resets every step looks at raw noise.  With temporal reprojection on, the context keeps a per-pixel HISTORY that follows the
 * spheres' and the camera's motion (SVGF's temporal part): mrt_temporal_step reprojects it, blends the newest frame into it and
 * keeps luminance moments; mrt_read_temporal / MRT_PRESENT_TEMPORAL hand the history, with a variance, to the denoiser's a-trous
 * iterations.  A hit point rides its sphere, so the motion vector is analytic: the guides hold the first-hit sphere index and
 * distance per pixel, the device the spheres as they are and -- a copy made by every step -- as they were.
 *
 * The intended loop: a context with max_framebuffer_weight = 0 (every blend weight is then 0: the framebuffer is the newest frame
 * alone); per animation step mrt_update_spheres and / or mrt_set_camera, mrt_redraw, mrt_temporal_step, mrt_present(fmt,
 * MRT_PRESENT_TEMPORAL | ...).  The step's input is the current framebuffer, whatever it holds: a caller who resets and renders k
 * frames per step gives it those k frames' mean, which is why mrt_reset does not touch the history.
 *
 * Contract.  Everything is queued on the ctx's stream behind the newest blend; nothing waits on the host (mrt_read_temporal, a
 * read-back, aside); none of these calls may be made while the ctx's stream is being captured into a graph.
 *   Enabling (mrt_set_temporal): MRT_ERR_STATE on a shard (world > 1); MRT_ERR_INVALID_ARG for a parameter out of range, a wrong
 *     size or a reserved word that is not 0, nothing changed.  It needs no noise tracking (the history keeps its own moments) and
 *     creates nothing: the four image-sized history buffers (16 bytes a pixel each) come with the denoiser's at the first step.
 *     Disabling frees them (after a bounded wait for the ctx's stream).  mrt_set_shard to world > 1 while enabled: MRT_ERR_STATE,
 *     nothing changed.  New parameters apply from the next step / read on; the history stays.
 *   mrt_temporal_step: MRT_ERR_STATE if disabled, on a shard, or before the first frame since mrt_create / mrt_reset;
 *     MRT_ERR_NO_SCENE without a scene.  It rebuilds the guides if they are stale, runs the reprojection, and then snapshots
 *     "previous" as the state at THIS step: the spheres' (cx, cy, cz, r) into a device copy, the derived camera on the host, and
 *     the history's two buffer pairs swap.  It advances the history exactly once.  An adaptive accumulation (mrt_render_tiles)
 *     is no obstacle: only the framebuffer is read.
 *   Invalidation: mrt_set_world* changes what the sphere indices mean and mrt_set_shard the buffers: both drop the history, as
 *     mrt_temporal_reset does (every length 0, nothing freed by the reset itself; the next step starts every pixel anew).
 *     mrt_update_spheres, mrt_regroup_spheres, mrt_set_camera and mrt_reset do not.
 *   mrt_read_temporal / MRT_PRESENT_TEMPORAL change no state: two calls without a step between them return identical bits.
 *     MRT_ERR_STATE before the first step since enabling or since the history was dropped.  The filter's parameters are the
 *     ctx's mrt_denoise_params; alpha is the framebuffer's.
 *
 * Definition (float32 in this order; only + - * /, sqrtf, floorf, fminf, fmaxf and comparisons; no fma).  History per texel:
 * H0 = (r, g, b, len), H1 = (m1, m2, t, bits of the sphere index).  For pixel p: cur = the framebuffer texel; (o, d) the guide ray;
 * (t, s) the guides' distance and sphere index (-1: a miss); (c1, r1) sphere s as it is, (c0, r0) as it was at the previous step;
 * o' the previous camera's origin and M the inverse of the 3 x 3 matrix with the columns su, sv, -fw of the previous derived
 * camera -- mode 0: su = x, sv = y, fw = +z, o' = 0 -- computed on the host in double by cofactors (M = adj / det, det =
 * (A00 C00 + A01 C01) + A02 C02, every cofactor one difference of two products) and rounded to float.  At the first step after the
 * history was dropped no tap counts, whatever "previous" holds.
 *   1 Previous position.  A hit: X = o + t * d (per component), k = r0 / r1, Xp = c0 + (X - c1) * k.  A miss: Xp = o' + d.
 *   2 Previous pixel.  v = Xp - o';  a = (M00 v.x + M01 v.y) + M02 v.z, b and l from rows 1 and 2 alike.  Unless l > 0: no
 *     history.  fx = (a / l) * (0.5f * H) + (0.5f * W - 1.0f), fy = (b / l) * (0.5f * H) + (0.5f * H - 1.0f) -- the inverse of the
 *     guide rays' vx = (x + 1 - W / 2) * 2 / H.  te = sqrtf((v.x v.x + v.y v.y) + v.z v.z).
 *   3 Taps.  x0 = floorf(fx), wx = fx - x0, y alike; the four taps (x0 + i, y0 + j), j then i, weigh bw = (i ? wx : 1 - wx) *
 *     (j ? wy : 1 - wy).  A tap q counts only if it lies inside the image, bw > 0, len_q >= 1, H0_q's r, g, b are finite, the
 *     index bits of H1_q equal s and -- for a hit -- fabsf(t_q - te) <= depth_tol * te.  In tap order, from 0: sw += bw,
 *     sc += bw * c_q, s1 += bw * m1_q, s2 += bw * m2_q; lmin = the smallest len_q.
 *   4 Blend.  Lc = lum(cur) (the noise estimate's lum).  With history (sw > 0): cp = sc / sw, m1p = s1 / sw, m2p = s2 / sw,
 *     N = fminf(lmin + 1, max_history), alpha = 1 / N, c' = cp + alpha * (cur - cp), m1' = m1p + alpha * (Lc - m1p), m2' = m2p +
 *     alpha * (Lc * Lc - m2p).  Without: c' = cur, m1' = Lc, m2' = Lc * Lc, N = 1.  Stored: H0' = (c', N), H1' = (m1', m2', t, s).
 *     A cur whose r, g or b is not finite stores H0' = (cur, 0), H1' = (0, 0, t, s): never a tap, passed through by the filter.
 *   5 Variance (at read / present time; the filter's input is (r, g, b, var)).  N >= max(2, spatial_len): var = fmaxf(0, m2' -
 *     m1' * m1') / (N - 1).  Otherwise, for a texel with N >= 1 and a finite colour, the denoiser's spatial initial variance:
 *     the same 7 x 7 taps, w_q = (w_normal * w_depth) * w_albedo with the ctx's denoise parameters, two passes, over L(c'), with
 *     "S finite" read as len >= 1.  Any other texel: var = 0.
 *   6 Filter.  The denoiser's prefiltering iterations (as SPATIAL_EARLY runs them behind its spatial estimate: luminance stop on,
 *     every iteration prefiltered) over that field. */
typedef struct {            /* 32 bytes */
    uint32_t size;          /* sizeof(mrt_temporal_params): the version of this struct */
    uint32_t max_history;   /* 1 .. 256 (default 32): the history length at which the blend becomes an EMA of weight 1 / max_history */
    uint32_t spatial_len;   /* 1 .. 16 (default 4): shorter histories take the spatial variance */
    float    depth_tol;     /* finite, > 0 (default 0.05): relative distance tolerance of a history tap */
    uint32_t reserved[4];   /* 0 */
} mrt_temporal_params;
/* Host only: the defaults. */
void mrt_temporal_params_default(mrt_temporal_params* out);
/* Turns temporal reprojection on or off; params NULL: the current ones (the defaults at first).  ctx NULL: checks the parameters
 * only (host only; MRT_ERR_INVALID_ARG with params NULL too). */
int mrt_set_temporal(mrt_ctx* ctx, int enabled, const mrt_temporal_params* params);
int mrt_get_temporal(mrt_ctx* ctx, int* enabled, mrt_temporal_params* out);   /* either pointer may be NULL */
/* Integrates the newest frame into the history; advances it exactly once. */
int mrt_temporal_step(mrt_ctx* ctx);
/* Every history length 0; nothing freed.  MRT_ERR_STATE if disabled. */
int mrt_temporal_reset(mrt_ctx* ctx);
/* The temporal image: height * width * 4 floats, row 0 = bottom, as mrt_read_framebuffer; synchronises as it does. */
int mrt_read_temporal(mrt_ctx* ctx, float* rgba_out, size_t cap_floats);

/* The temporal RESPONSE: a fast-history clamp and an anti-lag rule for what the index and depth tests of step 3 let through.
 * A reflection or a refraction moves with the spheres BEHIND the first hit, which the motion vector does not know: a pixel on a
 * mirror keeps its full history while what it shows changes, and at max_history 32 the stale colour decays by 1 / 32 a step.
 * With the response on the history carries a third texel, H2 = (fr, fg, fb, valid): a FAST history of the same taps whose length
 * stops at fast_history.  After every step the long history's colour is clamped to the local statistics of the fast one, and
 * where the clamp had to act the long history's length is pulled towards the fast length (the fast-history clamping of real-time
 * denoisers).  Off -- the default -- every bit, buffer and launch of mrt_temporal_step is what it is without it.
 *
 * Contract.  The setting lives as long as the temporal parameters do: mrt_reset, mrt_set_world*, mrt_set_camera and mrt_set_shard
 * keep it.  It may be set whether or not temporal reprojection is enabled, and setting it creates nothing.  A call that changes
 * `enabled` drops the history, as mrt_temporal_reset does (mrt_read_temporal / MRT_PRESENT_TEMPORAL: MRT_ERR_STATE until the next
 * step); a call that changes only the three numbers keeps it and applies from the next step on.  With `enabled` on, the first
 * mrt_temporal_step brings two more image-sized buffers, the H2 pair (16 bytes a pixel each), with the history's and by the same
 * means; they swap with the other two pairs, are freed when temporal reprojection is disabled or the ctx destroyed (not when
 * the response alone is turned off), and a dropped history zeroes the H2 the next step reads.  mrt_set_shard, which replaces
 * the ctx's image-sized buffers, releases the H2 pair with the history's four -- the history is dropped by that call anyway
 * (Invalidation, above) -- and the next step with the response on brings a new pair, zeroed as after any drop; the setting
 * itself stays.  While the response is off the H2 pair is neither read nor written, so what it held when the response is turned
 * on again never reaches a step: that change of `enabled` drops the history, and the drop zeroes it.  MRT_ERR_INVALID_ARG, nothing
 * changed: a wrong size, enabled above 1, fast_history outside 1 .. 16, a clamp_sigma that is not finite and > 0, an antilag
 * outside 0 .. 1 (a NaN included), a reserved word that is not 0, a NULL argument.  Every refusal of the step, the read and the
 * present is what it was; mrt_read_temporal and MRT_PRESENT_TEMPORAL read H0 and H1 as before.
 *
 * Definition (float32 in this order; only + - * /, sqrtf, floorf, fminf, fmaxf, fabsf and comparisons; no fma).  Steps 1 to 3 are
 * the ones above: the same taps count, with the same weights.
 *   3 also, for every counted tap, in tap order, from 0: sf += bw * H2_q.rgb (whatever H2_q's valid says).
 *   4 also.  With history: fp = sf / sw, Nf = fminf(N, fast_history), f' = fp + (1 / Nf) * (cur - fp).  Without: f' = cur.
 *     Stored: H2' = (f', 1).  A cur whose r, g or b is not finite stores H2' = (cur, 0).
 *   4b Clamp, after step 4 of EVERY pixel, for a pixel whose H0'.w >= 2 (one that found history).  Window: the 5 x 5 pixels around
 *     it, dy then dx from -2 to 2, the centre included.  A window tap q counts if it lies inside the image, H2'_q.w == 1, H2'_q's
 *     r, g, b are finite and the index bits of H1'_q equal the pixel's own.  Per channel, in tap order, from 0: s1 += f_q,
 *     s2 += f_q * f_q; n += 1 (a float).  Fewer than 2 counted taps: the pixel stays as step 4 left it.  Otherwise per channel
 *     mean = s1 / n, sd = sqrtf(fmaxf(0, s2 / n - mean * mean)), e = clamp_sigma * sd, c'' = fminf(fmaxf(c', mean - e), mean + e).
 *   4c Anti-lag.  d = fmaxf(fmaxf(fabsf(c''.r - c'.r), fabsf(c''.g - c'.g)), fabsf(c''.b - c'.b)), emax = fmaxf(fmaxf(e.r, e.g),
 *     e.b), r = fminf(1, d / (emax + 1e-6f)), N'' = N + (antilag * r) * (fminf(N, fast_history) - N).
 *     Stored: H0' = (c'', N'').  m1', m2' and H1' are step 4's.
 * The stored length may therefore be fractional (step 3's lmin and step 5's N take it as the float it is).  The luminance
 * moments are not clamped: a pixel that was clamped reads a wide variance for a few steps and the filter blurs it more -- a short
 * history wants more spatial support. */
typedef struct {            /* 32 bytes */
    uint32_t size;          /* sizeof(mrt_temporal_response): the version of this struct */
    uint32_t enabled;       /* 0 (default): mrt_temporal_step is exactly what it is without the response; 1: on */
    uint32_t fast_history;  /* 1 .. 16 (default 4): the length at which the fast history becomes an EMA */
    float    clamp_sigma;   /* finite, > 0 (default 2): half-width of the clamp box in standard deviations */
    float    antilag;       /* 0 .. 1 (default 1): how far a fully clamped pixel's length is pulled to the fast length */
    uint32_t reserved[3];   /* 0 */
} mrt_temporal_response;
/* Host only: the defaults (enabled = 0). */
void mrt_temporal_response_default(mrt_temporal_response* out);
/* ctx NULL: checks the setting only (host only). */
int mrt_set_temporal_response(mrt_ctx* ctx, const mrt_temporal_response* response);
int mrt_get_temporal_response(mrt_ctx* ctx, mrt_temporal_response* out);

/* ------------------------------------------------------------------ diagnostic views (no reference counterpart)
 *
 * What the renderer decides by, as pictures: the per-pixel noise estimate that stops a render and picks adaptive tiles, the per-tile
 * frame count n_t that shows where adaptive and budget sampling spent their frames, and the first-hit guides that drive the
 * denoiser and the temporal reprojection.  A view is an RGBA32F image the size of the frame, computed by one kernel (views.hip) on
 * the ctx's stream, behind the newest blend and with no host wait, from buffers the context already holds, into the denoised
 * frame's buffer.  It is one more image source: mrt_present(.., flags | MRT_PRESENT_VIEW) shows it in any format, with FLIP_Y,
 * through the ring, and mrt_read_view returns its floats.  World 1 only (a view is image-sized and the guides are unsharded).
 *
 * The definition.  Everything is float32, in the stated order, for pixel p of tile t (8 x 8 pixels).  Scalar kinds give a value q:
 *   NOISE_SE, NOISE_REL  With s = S_p and L = lum(framebuffer_p), as the noise report has them ("noise estimate"): if s or L is not
 *                finite, q is a NaN.  Otherwise se = isinf(K_p) ? +inf : sqrtf(s * K_p) and rel = se / fmaxf(L, rel_floor); q is se or
 *                rel.  K_p: for a uniform accumulation, (float) of the factor a noise report queried at this point of the stream
 *                carries; for an adaptive accumulation (mrt_render_tiles since the last reset), (float)mrt_noise_factor(n_t, max_w)
 *                of the pixel's tile.  An adaptive accumulation is not refused: showing it is the point.
 *   TILE_FRAMES  q = (float)n_t; while the accumulation is uniform, (float)mrt_frames_done.
 *   DEPTH        q = the distance t of the first hit along the pixel's centre ray, +inf on a miss.
 * A scalar is mapped by u = (q - lo) * inv, with inv = 1.0f / (hi - lo) computed once on the host:
 *   GREY   rgb = (u, u, u), not clamped: with lo 0 and hi 1 the float formats return q bit for bit for every non-NaN q.
 *   HEAT   a NaN q gives (1, 0, 1).  Otherwise v = fminf(fmaxf(u, 0), 1), x = v * 4.0f, r = c01(x - 2), g = c01(fminf(x, 4 - x)),
 *          b = c01(2 - x) with c01(y) = fminf(fmaxf(y, 0), 1): blue, cyan, green, yellow, red, and +inf is red (hi > lo).
 * Vector kinds ignore ramp, lo and hi (which are validated all the same):
 *   NORMAL  rgb = n * 0.5f + 0.5f per component of the first hit's unit normal (a miss: the guide's normal as it is).
 *   ALBEDO  rgb = the bits of the first hit's albedo as the denoiser's guides hold it (a Dielectric reads (1, 1, 1)).
 *   SPHERE  for the first hit's sphere index i: a miss (-1) gives (0, 0, 0); otherwise h = (uint32_t)(i + 1) * 2654435761u, then
 *           h ^= h >> 15, r = ((float)(h >> 24) + 0.5f) * (1.0f / 256.0f), g the same of bits 16..23 and b of bits 8..15.
 * Alpha is 1.0f in every view.  Every operation above except the report's own sqrtf and / is exact or a single rounding in
 * float32, so nothing depends on contraction.
 *
 * The guide kinds rebuild stale guides first (after mrt_set_camera, mrt_set_world*, mrt_update_spheres / _materials), as a denoise
 * does.  A view's buffers are the denoiser's, allocated at the first view or denoise, whichever comes first; a view changes no
 * accumulation, no S, no tile map and no counter, and the next denoise or view overwrites its image. */
enum { MRT_VIEW_NOISE_SE = 1, MRT_VIEW_NOISE_REL = 2, MRT_VIEW_TILE_FRAMES = 3, MRT_VIEW_DEPTH = 4,
       MRT_VIEW_NORMAL = 5, MRT_VIEW_ALBEDO = 6, MRT_VIEW_SPHERE = 7 };
enum { MRT_VIEW_RAMP_GREY = 0, MRT_VIEW_RAMP_HEAT = 1 };
typedef struct {            /* sizeof 32 */
    uint32_t size;          /* sizeof(mrt_view): the version of this struct */
    uint32_t kind;          /* MRT_VIEW_* (default NOISE_REL) */
    uint32_t ramp;          /* MRT_VIEW_RAMP_* (default HEAT) */
    float    lo, hi;        /* finite, hi != lo, 1.0f / (hi - lo) finite; hi < lo reverses the ramp (default 0 and 0.1) */
    float    rel_floor;     /* finite, >= 0: NOISE_REL's floor under the luminance (default 0.01) */
    uint32_t reserved[2];   /* 0 */
} mrt_view;
/* Host only: the defaults. */
void mrt_view_default(mrt_view* out);
/* Anything out of range, size or reserved wrong: MRT_ERR_INVALID_ARG with nothing changed.  ctx NULL: checks v only (host only).
 * The setting creates nothing, takes effect at the next view and survives mrt_reset, mrt_set_shard, mrt_set_world* and
 * mrt_set_camera. */
int mrt_set_view(mrt_ctx* ctx, const mrt_view* v);
int mrt_get_view(mrt_ctx* ctx, mrt_view* out);
/* Computes the current view of the most recent frame (queued on the ctx's stream behind its blend) and reads it back: height *
 * width * 4 floats, row 0 = bottom; synchronises as mrt_read_denoised does.  Refused, in this order and before any runtime call
 * (MRT_PRESENT_VIEW alike): MRT_ERR_STATE on a shard (world > 1), MRT_ERR_NO_SCENE without a scene, MRT_ERR_STATE for an empty
 * image, MRT_ERR_STATE for a NOISE_* kind with noise tracking off. */
int mrt_read_view(mrt_ctx* ctx, float* rgba_out, size_t cap_floats);

/* ------------------------------------------------------------------ multi-GPU (no reference counterpart)
 *
 * The reference drives one adapter (lib.rs:329-335).  The caller that owns its frame loop (State::new /
 * State::redraw, lib.rs:217-234, :241-307) uses N GPUs by holding one mrt_ctx per GPU, ctxs[i] created on
 * device i with mrt_set_shard(ctxs[i], i, N), calling mrt_redraw on each and then ONE gather per frame. */

/* One process, N contexts.  Copies every shard's most recent framebuffer into its interleaved place in the
 * root's full-frame buffer: device-to-device (peer-to-peer over xGMI) copies of the shard's bands, issued on
 * that shard's own stream (so it follows its redraw), all links at once; the root's stream then waits for all
 * of them.  Asynchronous; read the result with mrt_read_gathered / mrt_gathered_device_ptr on ctxs[root].
 * Requires ctxs[i] to be shard i of n of the same width x height. */
int mrt_gather(mrt_ctx* const* ctxs, uint32_t n, uint32_t root);
/* One process per GPU (shard rank = RCCL rank): grouped ncclSend / ncclRecv of the packed bands on
 * `nccl_comm` (an ncclComm_t the caller created with ITS librccl; this library resolves RCCL's entry points at
 * run time and does not link it), one message per peer straight to the root, then the un-permute on the
 * root, all on the ctx's stream.  Collective: every rank calls it once per frame. */
int mrt_gather_rccl(mrt_ctx* ctx, void* nccl_comm, uint32_t root);
/* Full frame on the root after a gather: height*width*4 floats, row 0 = bottom (device pointer valid until the
 * next gather on this ctx; order further work after the ctx's stream: the next gather's copies wait for
 * everything queued on the root's stream before it, so an asynchronous reader queued there is never overtaken). */
void* mrt_gathered_device_ptr(mrt_ctx* root_ctx);
int mrt_read_gathered(mrt_ctx* root_ctx, float* rgba_out, size_t cap_floats);   /* synchronises */

/* ---- the noise estimate across shards: a denoised preview of the gathered frame ----
 * A shard tracks S for its own rows (mrt_set_noise_tracking), bit for bit the unsharded context's; every shard holds the same
 * scene and camera.  With this setting on, a gather also assembles the full-frame S on the root, and the root can build the
 * guides of the full image and run the denoiser on (gathered colour, gathered S, K, guides) -- the layout of world == 1.  The
 * shards' own mrt_read_denoised / MRT_PRESENT_DENOISED stay refused (MRT_ERR_STATE), and MRT_PRESENT_DENOISED |
 * MRT_PRESENT_GATHERED stays MRT_ERR_INVALID_ARG.
 *
 * mrt_set_gather_noise(ctx, enabled): default 0, and with 0 both gathers queue exactly the calls and bytes they always have.
 * Creates nothing; takes effect at the next gather; a CHANGE of the setting drops the gathered S until then (the reads below:
 * MRT_ERR_STATE), as mrt_set_shard does, and the first gather after a change allocates the gathered frame anew, S included or
 * not (it waits for the root's stream first; mrt_gathered_device_ptr changes).  ctx NULL: MRT_ERR_INVALID_ARG.  mrt_gather reads the ROOT's setting.
 * mrt_gather_rccl reads each rank's own, and all ranks must agree: a disagreement is the caller's error, like a disagreeing
 * `root` (the messages no longer match; nothing in this library can detect it).
 *   With the setting on, mrt_gather also copies every shard's S bands into their places of a full-frame S on the root (in the
 * allocation of the gathered colour, behind it: mrt_gathered_device_ptr means what it meant), on the same streams, behind the
 * same events and under the same write-after-read rule as the colour.  Refused with MRT_ERR_STATE on the root, before anything
 * is queued and with a message that names the context: a context with noise tracking off, one whose accumulation is adaptive
 * (mrt_render_tiles since its last reset), one whose mrt_frames_done or max_framebuffer_weight differs from the root's (ONE K
 * turns the frame's S into a variance).  mrt_gather_rccl: a non-root rank sends S as a second message in the same call; the
 * root receives both in its one group and un-permutes both (a rank with noise tracking off: MRT_ERR_STATE on that rank).
 *   The snapshot: at such a gather the root records K = mrt_noise_factor of ITS accumulation and its mrt_frames_done.  The
 * gathered frame is denoised with that snapshot, whatever the root renders between the gather and the denoise.
 *
 * mrt_read_gathered_noise: the gathered S, height * width floats, row 0 = bottom; synchronises as mrt_read_gathered does.
 * MRT_ERR_STATE before the first gather and when the latest gather carried no S; MRT_ERR_TOO_SMALL.
 * mrt_read_gathered_denoised: the latest gathered frame, denoised: height * width * 4 floats, row 0 = bottom.  Queues, on the
 * root's stream behind the gather's waits, the guide rebuild if the guides are stale (the root's CURRENT camera and scene over
 * the full image; mrt_set_camera, mrt_set_world*, mrt_update_spheres and mrt_set_shard mark them stale, as for
 * mrt_read_denoised) and the filter with the root's mrt_denoise_params and variance mode -- MRT_DENOISE_VAR_SPATIAL_EARLY
 * compares the SNAPSHOT's frame count with spatial_frames; the read-back is the only host wait.  Refusals: MRT_ERR_STATE as
 * mrt_read_gathered_noise's, MRT_ERR_NO_SCENE without a scene, MRT_ERR_TOO_SMALL.  The denoiser's buffers are allocated on the
 * root at the first use, full-image sized, as mrt_read_denoised's are.  Works for world == 1 too (a gather of one): the image
 * is then mrt_read_denoised's, bit for bit -- as it is for any world, since the shards' rows and S are the unsharded ones. */
int mrt_set_gather_noise(mrt_ctx* ctx, int enabled);
int mrt_read_gathered_noise(mrt_ctx* root_ctx, float* s_out, size_t cap_floats);              /* synchronises */
int mrt_read_gathered_denoised(mrt_ctx* root_ctx, float* rgba_out, size_t cap_floats);        /* synchronises */
/* host-only index math of the interleave: local row r of shard (rank, world) is this global row; rows per
 * shard; and the un-permute of a rank-major [world][local_rows][width][4] array into [height][width][4] */
uint32_t mrt_shard_global_row(uint32_t local_row, uint32_t rank, uint32_t world);
uint32_t mrt_shard_local_rows(uint32_t height, uint32_t world);
int mrt_unshard_rows(const float* gathered, uint32_t world, uint32_t width, uint32_t height, float* out);
/* Elapsed GPU time (ms) of the most recent redraw's render kernel, from HIP events on
 * the launch stream.  Synchronises on the stop event. */
int mrt_last_kernel_ms(mrt_ctx* ctx, float* ms);
/* The same for the n <= min(cap, 64) most recent redraws, oldest first. */
int mrt_kernel_ms_history(mrt_ctx* ctx, float* ms, size_t cap, size_t* n_out);

const char* mrt_last_error(mrt_ctx* ctx);       /* never NULL; ctx may be NULL */
/* Identifies the binary: the first 16 hex digits of the sha256 over the library's sources (the Makefile computes it at
 * build time; bench.py prints it next to the hash of the sources on disk and refuses a headline from a stale build). */
const char* mrt_build_id(void);
const char* mrt_status_string(int status);
int mrt_abi_version(void);

/* ------------------------------------------------------------------ scenes (host only) */

/* The shipped 4-sphere scene, lib.rs:687-720.  Returns the sphere count (4) or a
 * negative mrt_status; writes min(cap, n) spheres. */
int mrt_scene_default(mrt_sphere* out, size_t cap);
/* RTIOW cover scene (extension): ground + 22x22 grid + 3 big spheres.
 * dielectric == 0 emits glass slots as Metal(0.9,0.9,0.9; fuzz 0) (config C2),
 * dielectric != 0 as Dielectric(1.5) (C3/C4).  cam_out (optional) gets the matching
 * camera (defocus only when dielectric != 0). */
int mrt_scene_cover(uint64_t scene_seed, int dielectric, mrt_sphere* out, size_t cap, mrt_camera* cam_out);
/* 10k-sphere stress scene (C5): ground + n_side x n_side jittered grid, 80/15/5 % L/M/D */
int mrt_scene_stress(uint64_t scene_seed, uint32_t n_side, mrt_sphere* out, size_t cap, mrt_camera* cam_out);

/* Scenes as data: a line-oriented text file holding what api::World (lib.rs:611-639,
 * hard-coded in the reference, lib.rs:687-720) and the camera extension hold:
 *     # comment
 *     camera pinhole
 *     camera lookat <from xyz> <at xyz> <up xyz> <vfov deg> <defocus angle deg> <focus dist>
 *     sphere <centre xyz> <radius> lambertian <albedo rgb>
 *     sphere <centre xyz> <radius> metal <albedo rgb> <fuzz>
 *     sphere <centre xyz> <radius> dielectric <ior>
 *     sphere <centre xyz> <radius> material <ty> <albedo rgb> <param>     (any other MaterialTy: absorbs)
 * Sphere order = the reference's sphere index order (it decides ties, shader.wgsl:291-296).  Numbers are
 * written with 9 significant digits, so save -> load reproduces every f32 bit.
 * mrt_scene_load returns the number of spheres in the file (writes min(cap, n)) or a negative mrt_status
 * (-MRT_ERR_IO, -MRT_ERR_BAD_SCENE; mrt_last_error(NULL) names the line); *has_camera = 1 if the file has a
 * camera line (cam_out filled), else 0 (cam_out = the reference's pinhole). */
int mrt_scene_save(const char* path, const mrt_sphere* spheres, size_t n, const mrt_camera* cam);
int mrt_scene_load(const char* path, mrt_sphere* out, size_t cap, mrt_camera* cam_out, int* has_camera);

/* ------------------------------------------------------------------ image output (host only) */

/* rgba: height*width*4 floats, row 0 = bottom (as read back).  PFM keeps linear floats
 * (bottom-up is PFM's native order).  PPM is what the reference's present pass puts on screen: the
 * linear value (sample_framebuffer.wgsl:38-41) stored to the sRGB surface (lib.rs:349-351, :1133), i.e.
 * clamp to [0,1], the sRGB OETF (12.92 c below 0.0031308, else 1.055 c^(1/2.4) - 0.055), round to 8 bits,
 * rows flipped to top-down (sample_framebuffer.wgsl:24). */
int mrt_write_pfm(const char* path, const float* rgba, uint32_t width, uint32_t height);
int mrt_write_ppm(const char* path, const float* rgba, uint32_t width, uint32_t height);
int mrt_write_png(const char* path, const float* rgba, uint32_t width, uint32_t height);   /* 8-bit RGB, same encoding as the PPM, + sRGB chunk */
uint8_t mrt_srgb8(float linear);      /* the per-channel conversion mrt_write_ppm / mrt_write_png apply */
/* float32 -> the bits of an IEEE binary16, the per-channel conversion of MRT_PRESENT_RGBA16F_LINEAR (the device computes the
 * same bits for every float): round to nearest, ties to even; subnormal halves are produced; a magnitude at or above 65520
 * gives +-inf, one at or below 2^-25 gives +-0 (the tie at 2^-25 included); zero and infinity keep their sign; every NaN gives
 * 0x7E00, whatever its sign or payload.  mrt_half_from_floats converts n floats (MRT_ERR_INVALID_ARG: a null pointer with n > 0). */
uint16_t mrt_half_bits(float v);
int mrt_half_from_floats(const float* in, size_t n, uint16_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MYRAYTRACER_AMD_H */
