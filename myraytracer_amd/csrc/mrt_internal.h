// Internal types shared by the HIP kernels (kernels.hip and the files beside it) and the host side of the C ABI
// (api.cpp and the files beside it).  Not installed; the public contract is include/myraytracer_amd.h.
#pragma once
#include <stdint.h>
#include "../../include/myraytracer_amd.h"
#include "../../include/myraytracer_amd_debug.h"

namespace mrt {

constexpr uint32_t kBandRows = 8;        // shard granule: 8 image rows (one row of 8x8 wave tiles)
constexpr uint32_t kTileW = 8;           // one 64-lane wave (= one workgroup) covers an 8x8 pixel tile
constexpr uint32_t kChunk = 16;          // spheres per chunk of the discriminant sweep (one u16 sign mask)
constexpr uint32_t kGroup = 8;           // records per scalar-load group; the sweep list is padded to this
constexpr uint32_t kClusterK = 4;        // spheres per sweep record (cluster)
constexpr uint32_t kMaxSpheres = 1u << 20;
constexpr uint32_t kMaxLevels = 4;       // levels of bounding spheres above the member spheres
// Conservativeness of a bounding-sphere test: the ray direction is stretched by kBoundStretch
// in the test and the stored radius is kBoundInflate x the enclosing radius (bounds.h, bound_record).
constexpr float kBoundStretch = 1.0001f;
constexpr double kBoundInflate = 1.015;
constexpr uint32_t kMaxFrameBatch = 32;   // frames one render launch may cover (stream mode, mrt_render)
constexpr uint32_t kQueueCap = 320;      // a work queue of the walk: < 64 left over + 4 x 64 pushed by one round
// small scenes' KParams::gen_cap: u16 entries behind the root queue, directly below the wave's candidate masks.  They held the
// stored cluster items once; the walk's table of first items lives in them and its word selection may read up to 3 x 256 bytes
// below the masks (kernels.hip, static_assert at kItemWindow).  Kept at this size for the LDS footprint (5 workgroups per CU)
constexpr uint32_t kSmallGenCap = 576;
constexpr uint32_t kStackReserve = 16;   // large scenes' work stack: entries beyond its capacity a one-item round may use (3 per level)
constexpr uint32_t kMaxDirect = 4;       // very large spheres tested by every ray directly, outside the hierarchy
constexpr uint32_t kCamMaskRecords = 128; // camera-ray cluster masks (cam_mask.hip): one 128-bit entry covers at most this many top records
constexpr uint32_t kCamListCap = 8;       // camera-ray sphere lists (cam_mask.hip): member slots one entry holds; more: kCamListOverflow
constexpr uint32_t kCamListOverflow = 0xFFFFFFFFu;      // (an unbuilt table is all ones: every entry overflowed)
// SMALL scenes (render_kernel's SC == 0): every node id of the hierarchy's n_members member slots fits 10 bits, so the hierarchy
// has one level, the member records live in LDS and the walk's work items are u16; larger scenes walk the boxes
inline bool scene_is_small(uint32_t n_members) { return n_members <= 1024u; }

// (cx, cy, cz, -(r*r)): the only per-sphere data the discriminant loop reads.  Derived on
// the host from the reference's SoA arrays (centres: vec4_f32_data, radii: f32_data;
// lib.rs:722-799) and padded to a multiple of kGroup with never-hit entries (w = +inf).
struct alignas(16) SphereRec { float cx, cy, cz, neg_r2; };

// Axis-aligned box of the member spheres under a node of the hierarchy (large scenes: the walk's second, much tighter bound
// -- a kd-built group of spheres on a plane fills its box, not its bounding sphere).
// BoxFull: what the host derives per node (hierarchy.cpp, build_boxes, by the formulas of bounds.h) and the diagnostics report: centre, half extents (measured
// from the f32 centre, rounded up) and the two coefficients of the test's slack K = kc X + kpad (X = |p|^2 or |p|_1 of the ray
// origin relative to the centre, per scene: KParams::box_quad); kc is ONE value per scene (KParams::box_kc).
// BoxRec: what the kernel reads, 24 bytes: the centre and the half extents WITH kpad folded in (e + kpad, rounded up) -- on the
// axis d x e_i the slack kpad (|d_j| + |d_k|) that gives covers what the "+ kpad" of the test covered (bounds.h, fold_kpad) --
// so an inner item's four children are 96 bytes instead of 128: a large scene's rounds wait for the vector-memory path's
// 64 bytes per clock and CU.  A never-hit box has extents -3e38.
struct BoxFull { float cx, cy, cz, ex, ey, ez, kc, kpad; };
struct alignas(8) BoxRec { float cx, cy, cz, ex, ey, ez; };

// Everything one raytrace pass needs, passed by value as kernel arguments (-> SGPRs).
// Mirrors the three bind groups of State::redraw (lib.rs:262-265): Locals + seeds,
// World + data arrays, previous framebuffer.
struct KParams {
    mrt_locals locals;          // shader.wgsl:8-17
    mrt_world world;            // shader.wgsl:178-182 (+ dielectric range)
    mrt_camera_raw cam;
    uint32_t n_spheres;         // world.spheres.length
    uint32_t n_padded;          // cluster records, multiple of kGroup
    uint32_t mask_chunks;       // chunks of kChunk records per sweep block: min(16, ceil(n_padded / kChunk))
    uint32_t shard_rank, shard_world;
    uint32_t cus;               // compute units of the device (host-side launch sizing only)
    const SphereRec* spheres;   // n_spheres records in the reference's order (exact tests)
    // Bounding-sphere hierarchy (hierarchy.cpp build_hierarchy): level 0 = the member spheres in cluster order
    // (4 per cluster, short clusters padded with never-hit records), level 1 = the clusters' bounds
    // (cx,cy,cz,-R^2), level k+1 = bounds of 4 consecutive level-k nodes; node j of level k has the
    // children 4j..4j+3 of level k-1.  The sweep runs over the TOP level (`levels`): `clusters`, n_padded
    // records (multiple of kGroup, padded with never-hit entries).  `nodes` holds levels 0..levels-1,
    // level k at level_base[k]; member_index[] is each member's index in the reference's sphere order.
    const SphereRec* clusters;
    // the same top-level records as the A operand of the matrix-core sweep (sweep.h, mfma_sweep_tile):
    // per tile of 32 records 64 lanes x 8 bf16, record order within a tile permuted to the result layout;
    // use_mfma selects that variant of the sweep (world.cpp decides per scene and camera)
    const uint16_t* top_mfma;
    uint32_t use_mfma;
    float mfma_origin[3];       // the records of top_mfma are relative to this point (centre of their bounding box)
    // The ray-side factors of the matrix-core sweep (world.cpp, fill_scene_params): with K a power of two such that
    // |K oc.ds| <= 1/2 for every ray the sweep admits, {kBoundStretch K, 2 K^2, -(1 - 2^-13) K^2, the largest admitted
    // |o - mfma_origin|^2}, and -K^2 as a pair of bf16 (sweep.h, mfma_ray_operands)
    float mfma_scale[4];
    uint32_t mfma_neg_k2_pair;
    // The sweep's space: the GEMMs see x' = mfma_axis (x - mfma_origin) per component, entries 1, 2 or 4 chosen per scene so
    // that flat clusters get small bounds (hierarchy.cpp, build_sweep_operand); top_mfma, mfma_scale and mfma_neg_k2_pair are
    // made for that space.  mfma_scaled = some entry is not 1: only then the kernel scales its rays.
    float mfma_axis[3];
    uint32_t mfma_scaled;
    const SphereRec* nodes;
    const uint32_t* member_index;
    uint32_t levels, n_nodes, n_members, gen_cap;
    uint32_t level_base[kMaxLevels];
    // Large scenes (more than 1,024 member slots): the axis-aligned boxes of the hierarchy's nodes, numbered TOP-DOWN over the
    // complete 4-ary tree below the n_padded swept records: depth t occupies [o_t, o_t + n_padded 4^t), o_t = n_padded
    // (4^t - 1) / 3, so the children of node g -- whatever its depth -- are 4 g + n_padded .. + 3 (never-hit boxes where the
    // tree has no node).  box_cluster_first = o_(levels - 1): the nodes from there on are the clusters (node g = cluster
    // g - box_cluster_first, members 4 m .. 4 m + 3 of level 0); box_cluster_parent_first = o_(levels - 2): the nodes from
    // there on have clusters as children.  box_quad: the form of the slack (selects the kernel instantiation).  gen_cap is
    // the capacity of the wave's work stack.  Null / 0 for small scenes.
    const BoxRec* boxes;
    uint32_t box_cluster_first, box_cluster_parent_first, box_quad;
    float box_kc;               // the slack's coefficient of X, one per scene (bounds.h, box_kpad)
    // the first box_lds_count boxes of that numbering (the swept top, and the level below it where it fits) are copied into
    // the workgroup's LDS: what the owners' filter and the first inner rounds read (kernels.hip)
    uint32_t box_lds_count;
    // Spheres far larger than the rest (a ground sphere) are candidates for nearly every ray: up to kMaxDirect
    // of them stay out of the hierarchy and every ray evaluates their discriminant itself, from SGPRs.
    // They are the members direct_first .. direct_first + n_direct - 1 of level 0.
    uint32_t n_direct, direct_first;
    SphereRec direct[kMaxDirect];
    uint32_t direct_index[kMaxDirect];      // their indices in the reference's sphere order
    const float* vec4_data;     // r_vec4_f32_data (shader.wgsl:189-190), 4 floats per texel
    const float* f32_data;      // r_f32_data
    const int32_t* i32_data;    // r_i32_data
    // per sphere, in the reference's order: (cx, cy, cz, radius) (albedo r, g, b, fuzz | ior) -- copies of the
    // entries of the three arrays above that shading the sphere reads (world.cpp)
    const float* shade;
    const uint32_t* seeds;      // r_rands: local_rows x W x [u32;4]
    const float* prev;          // r_framebuffer: local_rows x W x rgba
    float* out;                 // render target
    unsigned long long* counters;  // 4 x u64 (mrt_counters) or null
    uint32_t count_draws;       // launch the instantiation that also counts the RNG draws (mrt_set_draw_counting)
    // the frame's tile queue: persistent waves pull tiles tile_order[atomicAdd(tile_queue, 1)]
    const uint32_t* tile_order; // n_tiles tile ids, heaviest first (tile_order.hip), or null = index order
    uint32_t* tile_queue;       // one u32, zeroed before every launch
    uint32_t tiles_x, n_tiles;  // tiles per band row; tiles in this shard
    uint32_t pilot_spp;         // samples per pixel of the cost-estimating pilot launch
    uint32_t* tile_cost;        // n_tiles: sum of its pixels' loop trips in this frame, or null
    void* pix_acc;              // per local pixel (and per block of samples): colour sum + cost (16 B), render -> finalize
    // counter-RNG mode: a pixel's samples are independent, so the frame is n_blocks layers (block b = samples
    // [64 b, 64 b + 64)), each summed into pix_acc[b * pix_stride + texel]; finalize adds the layers in order.  1 otherwise.
    // Stream mode: layer b = frame b of a batch of consecutive frames rendered by one launch (mrt_render), with
    // rng_shuffle layer_shuffle[b]; layer_shuffle[0] is always the (first) frame's shuffle.
    // queue_layers = layers the tile QUEUE holds (n_tiles x queue_layers items): n_blocks, except for a batch of short frames
    // of the stream mode, where the queue holds every tile once and the lane that takes a pixel renders it for all
    // lane_frames frames of the batch, frame b into layer b (lane_frames = n_blocks then, 1 otherwise).
    uint32_t n_blocks, pix_stride, queue_layers, lane_frames;
    uint32_t layer_shuffle[kMaxFrameBatch][4];
    unsigned long long* wave_log;  // diagnostic (-DMRT_STAMPS builds): 4 x u64 per wave, or null
    // mrt_debug_world_hit (the DBG instantiation of render_kernel): rays in (origin xyz, direction xyz), out: winner
    // {sphere index | -1, bits of t} per ray and the bitmap of spheres that reached the root tests
    const float* dbg_rays;
    int32_t* dbg_hit;
    uint32_t* dbg_cand;
    uint32_t dbg_words;         // bitmap words per ray
    // Camera-ray cluster masks (cam_mask.hip; small scenes of at most kCamMaskRecords top records): 4 words per 8 consecutive texels
    // of the shard, entry texel >> 3, in the sweep's bit layout; the sweep ANDs them onto the candidate words of camera rays.
    // Null = off (today's instructions).  LAST, so that no other argument's offset moves.
    const uint32_t* cam_masks;
    // Camera-ray sphere lists (cam_mask.hip, the same launch; the masks' indexing): 4 words per entry, the level-0 member slots a
    // camera ray of the entry's texels can touch; the render kernel resolves such a ray in the lane, at the tail of the iteration
    // that starts its sample (kernels.hip, primary hit).  Non-null selects the instantiations that read it (SC = 3, launch_render):
    // a launch without it runs the kernels of before.  While they are in force cam_masks is null.  Appended behind cam_masks for
    // the same reason.
    const uint32_t* cam_lists;
};

// api.cpp: message behind mrt_last_error(NULL), for failures of entry points that have no context
void set_global_error(const char* msg);

// host-callable launchers (kernels.hip)
// queue reset + n_waves persistent render waves (a pilot launch also runs its cost-only finalize)
int launch_render(const KParams& p, bool pilot, uint32_t n_waves, void* stream, uint32_t* which = nullptr);
// the per-tile finalize pass of a rendered frame: colour sums -> framebuffer, tile costs; with noise_s (noise tracking: local
// texels like the framebuffer) the blend also updates the per-texel luminance variance there (finalize_tracked_kernel)
int launch_finalize(const KParams& p, void* stream, float* noise_s = nullptr);
int launch_debug_world_hit(const KParams& p, uint32_t n_waves, void* stream);
int render_waves_per_cu(int* out);
// host only: {LDS bytes of one render workgroup, workgroups per CU} for p's scene layout; the work-stack capacity (entries)
// of a large scene's wave with `mask_chunks` chunks of candidate masks
void render_lds_layout(const KParams& p, uint32_t out[2]);
uint32_t render_resident_waves(const KParams& p);
uint32_t large_scene_stack_cap(uint32_t mask_chunks, uint32_t box_lds_count);
// how many leading boxes of the top-down numbering a large scene's workgroup keeps in LDS: the top level (n_top padded records)
// and the 4 n_top slots of the level below, or the top alone, or none -- the most that leaves the waves their work stacks
uint32_t large_scene_box_lds_count(uint32_t n_top_padded, uint32_t levels, uint32_t mask_chunks, uint32_t cap);
constexpr uint32_t kBoxLdsCap = 1024;    // never more boxes (32 B each) than this in a workgroup's LDS
// tile_order.hip: order[] = tile ids sorted by cost[] descending (bucket sort; ties in any order).
// scratch: 1024 u32.
int launch_sort_tiles(const uint32_t* cost, uint32_t* order, uint32_t* scratch, uint32_t n_tiles, void* stream);
// the same for a subset frame (adaptive sampling): order[] = the n ids of list[] sorted by cost[id] descending
int launch_sort_tile_list(const uint32_t* cost, const uint32_t* list, uint32_t* order, uint32_t* scratch, uint32_t n, void* stream);
// one single-wave kernel that stays resident for `ticks` of the 100 MHz clock (at most max_polls polls); out (optional, device-
// visible) gets its {start, end} ticks
int launch_hold(unsigned long long ticks, uint32_t max_polls, unsigned long long* out, void* stream);
int launch_fill_seeds(uint32_t* seeds, uint64_t seed, uint32_t width, uint32_t height,
                      uint32_t shard_rank, uint32_t shard_world, uint32_t local_bands, void* stream);

// mrt_debug_arith / mrt_debug_arith_pairs: div_unscaled / sqrt_unscaled against `/` and sqrtf() on the device
int launch_arith_check(int mode, const uint32_t r[4], unsigned long long count, unsigned long long seed, unsigned long long* d_out,
                       void* stream);
int launch_arith_pairs(const float* d_x, const float* d_y, uint32_t n, uint32_t* d_out, void* stream);

// present.hip: `rows` rows of `width` RGBA32F texels -> 4 B per pixel (8-bit sRGB colour, linear alpha; bgra: B, G, R, A order),
// top-down with `flip`; d_tables: the 2 x 256 floats of present_thresholds() in device memory
int launch_present(const float* src, uint8_t* dst, uint32_t width, uint32_t rows, uint32_t flip, uint32_t bgra,
                   const float* d_tables, void* stream);
// present.hip: the linear formats -- the same rows as 4 x binary16 per pixel (half: half_bits of every channel) or as the
// source's own 4 x float32 bits, top-down with `flip`; no table
int launch_present_float(const float* src, uint8_t* dst, uint32_t width, uint32_t rows, uint32_t flip, uint32_t half, void* stream);
// mrt_half_bits (include/myraytracer_amd.h), the one definition the host and present.hip share: float32 -> IEEE binary16,
// round to nearest even in integer arithmetic.  Subnormal halves are produced; |v| >= 65520 -> +-inf; |v| <= 2^-25 -> +-0
// (the tie included); every NaN -> 0x7E00.
__host__ __device__ inline uint16_t half_bits(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v), sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return 0x7E00u;
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);                  // 65520 and above, inf
    if (a >= 0x38800000u) {                                                    // 2^-14 and above: a normal half
        const uint32_t r = a - 0x38000000u;                                    // (exponent rebiased: 127 -> 15)
        return (uint16_t)(sign | ((r + 0xFFFu + ((r >> 13) & 1u)) >> 13));     // (a carry out of the mantissa raises the exponent)
    }
    if (a <= 0x33000000u) return (uint16_t)sign;                               // 2^-25 and below
    const uint32_t shift = 126u - (a >> 23), m = (a & 0x7FFFFFu) | 0x800000u;  // a subnormal half: m 2^-shift units of 2^-24, shift 14..24
    const uint32_t h = m >> shift, rem = m & ((1u << shift) - 1u), tie = 1u << (shift - 1u);
    return (uint16_t)(sign | (h + ((rem > tie || (rem == tie && (h & 1u))) ? 1u : 0u)));
}
// views.hip (include/myraytracer_amd.h, "diagnostic views"): view `kind` of width x height world-1 texels (y * width + x) into
// `out`, RGBA32F.  Read per kind only: NOISE_* fb and S, with K the launch's (tile_frames null) or Kf[n_t] per tile; TILE_FRAMES
// `frames` or (float)n_t; DEPTH / NORMAL / ALBEDO / SPHERE the guides (2 float4 per pixel, launch_guide_fill's).  inv: 1 / (hi - lo).
struct ViewArgs {
    const float* fb;
    const float* S;
    const float* guides;
    const uint32_t* tile_frames;    // n_t per tile, tiles_x a row: a diverged accumulation (NOISE_*, TILE_FRAMES); else null
    const float* Kf;                // K(n) as float for every n the map holds (NOISE_* per tile)
    float* out;
    uint32_t width, height, tiles_x;
    uint32_t kind, ramp;
    float K, frames;                // a uniform accumulation's K and (float)frames_done
    float lo, inv, rel_floor;
};
int launch_view(const ViewArgs& a, void* stream);
inline mrt_view view_defaults() {
    mrt_view v{};
    v.size = sizeof(mrt_view);
    v.kind = MRT_VIEW_NOISE_REL; v.ramp = MRT_VIEW_RAMP_HEAT;
    v.lo = 0.0f; v.hi = 0.1f;       // the README's "no pixel above 10 %"
    v.rel_floor = 0.01f;            // State.render_until's floor
    return v;
}
// image_io.cpp, host: {colour, alpha} x 256 thresholds -- t[k] = the smallest float whose code is >= k (t[0] = -inf)
const float* present_thresholds();

// noise.hip: the noise report's sums over a context's texels (or a caller's buffers) and a map of its 8x8 tiles, numbered as
// finalize_kernel numbers them (band x tiles_x + tile column).  Two kernels on `stream`; *out (device) gets the sums.
struct NoiseSums {                  // 48 B
    double sum_s, sum_l;
    unsigned long long pixels, non_finite, above;
    float max_se;
    uint32_t pad;
};
size_t noise_partials_bytes(uint32_t width, uint32_t local_bands);
// host: c2 after a blend of weight w (include/myraytracer_amd.h, "noise estimate"): w^2 c2 + (1 - w)^2, 1 at w == 0; and K
inline double noise_c2_next(double c2, float w) {
    const double wd = (double)w;
    return w == 0.0f ? 1.0 : wd * wd * c2 + (1.0 - wd) * (1.0 - wd);
}
inline double noise_factor_of(double c2) { return c2 >= 1.0 ? __builtin_inf() : c2 / (1.0 - c2); }
// The recursion by one frame: c2 after frame k of an accumulation whose weights are mrt_frame_weight(k, max_w).  fixed: the weight
// is saturated -- it stays so, mrt_frame_weight being non-decreasing up to there -- and c2 did not move: every later c2 is this
// one, so stopping here (mrt_noise_factor, mrt_budget_allocate) and going on (the context's K table) give the same values.
struct NoiseC2Step { double c2; bool fixed; };
inline NoiseC2Step noise_c2_step(double c2, uint32_t k, float max_w) {
    const float w = mrt_frame_weight(k, max_w);
    const double next = noise_c2_next(c2, w);
    return {next, k != 0 && w == max_w && max_w < 0.99999988f && next == c2};
}
// The arithmetic of every form, in this order.  A pixel is counted if it lies in the image and its S_p and L_p = lum(fb_p) are
// finite (any other: non_finite alone).  With K the launch's (uniform) or K_t = Kf[n_t], n_t = tile_frames[tile] (per tile), in
// float: se_p = sqrtf(S_p * K), or +inf where K is +inf; rel_p = se_p / fmaxf(L_p, floor); above counts rel_p > threshold; max_se
// from 0.  In double: sum_l adds L_p and sum_s adds S_p (uniform: the host multiplies by K) or S_p * Kd[n_t] -- sum_var itself;
// nothing where K_t is +inf, the report being "no estimate yet" then -- (per tile).  A lane adds its four pixels by ascending
// column, a wave its lanes by xor-shuffles (32 down to 1), a block its eight rows by ascending row, noise_final_kernel the blocks'
// partials: thread t takes t, t + 256, ... in order, then a fixed tree.  The map entry of a tile: MRT_TILE_MAP_MAX_REL the largest
// rel_p of its counted pixels from 0 (a NaN ignored); MRT_TILE_MAP_SUM_S (float) of their summed (double)S_p, every other pixel
// +0.0: a row's eight columns as ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), then the eight row sums one after the other
// from the band's bottom row, starting at 0.0.  The map kind changes nothing in *out, and no K enters a summed-S map.
struct NoiseReduceArgs {
    const float* S;             // local_bands x 8 rows of `width` floats
    const float* rgba;          // the framebuffer in the same texel order
    uint32_t width, local_bands;
    uint32_t height, rank, world;   // local rows whose image row (shard rank of world) is >= height are skipped
    float K;                    // the uniform K (tile_frames null)
    const uint32_t* tile_frames;    // n_t per tile after adaptive sampling has diverged (world 1), or null: uniform
    const float* Kf;            // with tile_frames: K(n) = mrt_noise_factor(n, max_w) for every n_t, as float ...
    const double* Kd;           // ... and as double
    float threshold, floor;
    uint32_t map_kind;          // MRT_TILE_MAP_MAX_REL or MRT_TILE_MAP_SUM_S
    void* partials;             // noise_partials_bytes(width, local_bands) of scratch
    float* tiles;               // the map
    NoiseSums* out;
};
int launch_noise_reduce(const NoiseReduceArgs& a, void* stream);

// budget.hip (include/myraytracer_amd.h, "budget allocation on the device"): mrt_budget_allocate's allocation as an exact selection
// over the keys (G, j, t) -- G = 0 for a mandatory frame, else the complemented bits of g'(t, j) -- by a radix select of 8-bit
// digits, most significant first: G's eight, then j, then t's four.  One launch per digit (a histogram of the digit over the
// candidates that match the digits fixed so far; every workgroup derives those itself from the earlier launches' histograms), one
// that counts every tile's keys at or below the selected one and sums each block of 64 tiles, one that adds the blocks' sums.
// Integer atomics only; the result depends on the inputs alone.
// Where it all lives: the tile-map allocation of alloc_noise_set, in 4-byte words from d_noise_tiles.  The `ring` maps stay first,
// entry i at i * n_tiles; behind them entry i's plan at plan + i * plan_stride -- the mrt_budget_result (16 words), then k_t per
// tile: one contiguous read-back --; then the selection's scratch, which the queries share in stream order: the digits'
// histograms and the blocks' partial sums P_b (var_before's, then var_after's).
constexpr uint32_t kBudgetDigits = 13, kBudgetBins = 256, kBudgetSumTiles = 64;
constexpr uint32_t kBudgetMaxN = 1u << 24;       // the largest n_t an allocation accepts (mrt_budget_allocate's limit)
struct BudgetLayout { size_t plan, plan_stride, hist, sums, words; uint32_t blocks; };
inline BudgetLayout budget_layout(size_t n_tiles, uint32_t ring) {
    const size_t nt = n_tiles ? n_tiles : 1;
    BudgetLayout l{};
    l.blocks = (uint32_t)((nt + kBudgetSumTiles - 1) / kBudgetSumTiles);
    size_t at = (size_t)ring * nt;
    at += at & 1;                                        // (the results hold 8-byte fields)
    l.plan = at;
    l.plan_stride = sizeof(mrt_budget_result) / 4 + nt + (nt & 1);
    at += (size_t)ring * l.plan_stride;
    at = (at + 3) & ~(size_t)3;                          // (a histogram is read 16 bytes a lane)
    l.hist = at; at += (size_t)kBudgetDigits * kBudgetBins;
    l.sums = at; at += 4 * (size_t)l.blocks;             // 2 x blocks doubles
    l.words = at;
    return l;
}
struct BudgetArgs {
    const float* s;             // the summed-S map
    const uint32_t* n;          // n_t per tile, or null: n_uniform everywhere
    const double* K;            // K(n) for n <= the largest n_t + max_frames + 1
    uint32_t n_uniform, n_tiles, max_frames;
    uint64_t budget;
    uint32_t* hist;             // kBudgetDigits x kBudgetBins
    double* sums;               // 2 x ceil(n_tiles / 64)
    mrt_budget_result* res;
    uint32_t* k_out;            // n_tiles
};
int launch_budget_plan(const BudgetArgs& a, void* stream);

// adaptive.hip (include/myraytracer_amd.h, "adaptive sampling"): the per-tile blend of a frame whose tiles have their own frame
// counts.  One wave per tile of `list` (null: every tile 0 .. n - 1), in place on `fb` (and S with noise_s): w =
// mrt_frame_weight(tile_frames[t], max_w) as the same float expression, the blend and S update finalize_kernel<false> /
// finalize_tracked_kernel are built from (blend.h), then tile_frames[t] += 1 (saturating) and tile_cost[t]; the first wave zeroes *tile_queue.  One
// context of world 1: local rows are image rows.
struct TileBlendArgs {
    const void* pix_acc;        // PixAcc per texel and layer (blend.h): n_blocks layers pix_stride apart, added in order
    uint32_t pix_stride, n_blocks;
    float* fb;                  // RGBA32F, width x (8 x bands) texels, blended in place
    float* noise_s;             // S per texel, or null (tracking off)
    uint32_t* tile_frames;      // n_t per tile
    const uint32_t* list;       // the listed tiles, or null = 0 .. n - 1
    uint32_t* tile_cost;        // per tile: its heaviest pixel's loop trips (the slot's next queue order)
    uint32_t* tile_queue;       // the slot's queue counter, zeroed
    uint32_t n, width, height, tiles_x, spp;
    float max_w;
};
int launch_tile_blend(const TileBlendArgs& a, void* stream);

// refit.hip (include/myraytracer_amd.h, mrt_update_spheres): the device side of a geometry update whose grouping stays.
// launch_refit_scatter: `count` <= kRefitBatch spheres (cx, cy, cz, radius), passed BY VALUE in the kernel arguments (no staging
// buffer, no copy for the runtime to order), into the four device copies of spheres [first, first + count): spheres, floats 0..3
// of shade, and the reference's SoA -- centres = vec4_data + 4 center_base_idx, radii = f32_data + radius_base_idx.
// launch_refit: everything derived from them, by the functions hierarchy.cpp derives it with (bounds.h): the member records (level 0 of nodes), every level's
// bounding spheres (nodes / clusters), with boxes != null the boxes and their opened-wide copies in the top-down numbering for
// box_quad / box_kc, and the A operand for D = I relative to origin.  n_hier: the member slots the hierarchy covers (direct_first).
constexpr uint32_t kRefitBatch = 192;    // 3 KB of the 4 KB a launch's arguments may take
struct RefitScatterArgs {
    SphereRec* spheres;
    float* shade;
    float* centres;
    float* radii;
    uint32_t first, count;
    float xyzr[4 * kRefitBatch];
};
struct RefitArgs {
    const SphereRec* spheres;
    const float* shade;
    const uint32_t* member_index;
    SphereRec* nodes;
    SphereRec* clusters;
    BoxRec* boxes;
    BoxRec* boxes_open;
    uint16_t* top_mfma;
    uint32_t n_members, n_hier, levels, n_nodes, n_padded;
    uint32_t level_base[kMaxLevels];
    uint32_t box_quad;
    float box_kc;
    float origin[3];
};
// cam_mask.hip: the camera-ray cluster masks of p's scene (level 0 of p.nodes), camera, image shape and shard into `masks`,
// `entries` entries of 4 words (entry e: texels 8 e .. 8 e + 7 of the shard's row-major order), and the camera-ray sphere lists
// of the same entries into `lists`, 4 words each
int launch_cam_masks(const KParams& p, uint32_t* masks, uint32_t* lists, uint32_t entries, void* stream);
int launch_refit_scatter(const RefitScatterArgs& a, void* stream);
int launch_refit(const RefitArgs& a, void* stream);

// refit.hip too (include/myraytracer_amd.h, mrt_update_materials): the device side of a material edit.  `count` <= kMaterialBatch
// spheres, BY VALUE in the kernel arguments as a geometry update's are: per sphere the four floats 4..7 of its shade record, as
// material_shade derives them on the host, and its type word (types = i32_data + material_ty_base_idx).  With restart_history the
// radius of the sphere's entry in prev_xyzr becomes a NaN: the next temporal step finds no history for the pixels that show it
// and its own snapshot restores the entry.  Nothing else is written.
constexpr uint32_t kMaterialBatch = 192;  // 20 bytes a sphere: 3,840 of the 4 KB a launch's arguments may take
struct MaterialScatterArgs {
    float* shade;
    int32_t* types;
    float* prev_xyzr;
    uint32_t first, count, restart_history, _pad;
    float words[4 * kMaterialBatch];
    int32_t ty[kMaterialBatch];
};
static_assert(sizeof(MaterialScatterArgs) <= 4096, "the batch rides in the kernel arguments: 4 KB a launch");
int launch_material_scatter(const MaterialScatterArgs& a, void* stream);
// What shading a hit reads of a sphere's material: floats 4..7 of its shade record.  The ONE derivation, for the build
// (mrt_set_world_raw) and for mrt_update_materials; param = fuzz (Metal) | ior (Dielectric).
void material_shade(int32_t ty, const float* albedo, float param, float out[4]);

// regroup.hip (include/myraytracer_amd.h, mrt_regroup_spheres): the pooled spheres -- those of the clusters [0, n_pool) that
// build_clusters made from its pool -- permuted over the member slots they occupy, by the ordering of tests/regroup_ref.py: a kd
// split whose cuts fall on power-of-two blocks of clusters.  Only member_index is written (and the scratch); launch_refit follows.
// The scratch is one scene buffer of u32 words, made by mrt_set_world_raw (world.cpp) and laid out by regroup_layout:
//   pool   the pooled spheres' indices, ascending: the order every regroup starts from          (host, read only)
//   clus   the cluster whose slots rank i of an order falls into                                 (host, read only)
//   pref   pref[k] = real member slots of the clusters [0, k), n_pool + 1 entries                (host, read only)
//   ord    two orders of the pool, written in turn by the depths whose segments are wider than a block
//   box    6 words per segment of such a depth: min x, y, z and max x, y, z of the centres in key form
//   keys   n_sort u64 composite keys (segment, key along the segment's axis, rank), sorted in place
//   state  the auto-regroup policy's RegroupState (regroup_policy.hip), 8-byte aligned: uploaded as "baseline pending, counters 0",
//          written by the device alone from then on, and only while the policy is on (mrt_set_auto_regroup)
constexpr uint32_t kRegroupBlock = 512;      // clusters per workgroup of the block kernel: at most 2,048 spheres in LDS
constexpr uint32_t kRegroupChunk = 4 * kRegroupBlock;
constexpr uint32_t kRegroupMaxSegments = 4096;   // 12 bits of a composite key; 32 for the key, 20 for the rank (kMaxSpheres)
// The policy's state: q_level[k - 1] = the quality figure of level k (the sum of R^2 over its nodes that begin inside the pool), q_last
// their sum as the last judgement saw it, q_ref the sum right after the last regroup (or when the policy was turned on); pending: the
// next judgement takes q_ref instead of deciding; gate: what the regroup kernels queued behind a check read (0: return at once).
struct RegroupState {
    double q_ref, q_last, q_level[kMaxLevels];
    uint32_t pending, gate;
    uint64_t checks, regroups;
};
static_assert(sizeof(RegroupState) == 72 && sizeof(RegroupState) % 8 == 0, "RegroupState is 18 words of the scratch");
struct RegroupLayout { size_t pool, clus, pref, ord[2], box, keys, state, words; uint32_t n_sort; };
inline RegroupLayout regroup_layout(uint32_t n_pool, uint32_t pooled) {
    RegroupLayout l{};
    l.n_sort = kRegroupChunk;
    while (l.n_sort < pooled) l.n_sort <<= 1;
    size_t at = 0;
    l.pool = at; at += pooled;
    l.clus = at; at += pooled;
    l.pref = at; at += (size_t)n_pool + 1;
    l.ord[0] = at; at += pooled;
    l.ord[1] = at; at += pooled;
    l.box = at; at += 6 * ((size_t)n_pool / 8 + 2);      // the narrowest such depth has segments of 8 clusters (a block of 4)
    at += at & 1;                                        // (the keys are 8 bytes each)
    l.keys = at; at += 2 * (size_t)l.n_sort;
    l.state = at; at += sizeof(RegroupState) / sizeof(uint32_t);     // (at is even here: the state is 8-byte aligned)
    l.words = at;
    return l;
}
struct RegroupArgs {
    const SphereRec* spheres;
    uint32_t* member_index;
    uint32_t* scratch;
    uint32_t n_pool, pooled;
    uint32_t block;             // clusters per workgroup of the block kernel: a power of two, 4 .. kRegroupBlock
    const uint32_t* gate;       // null: run (mrt_regroup_spheres); else every kernel returns at once where *gate == 0
};
// the block in force for n_pool clusters (raised while a depth above it would have more than kRegroupMaxSegments segments), and
// the depths above it / within it: host only
void regroup_plan(uint32_t n_pool, uint32_t block, uint32_t out[3]);
int launch_regroup(const RegroupArgs& a, void* stream);

// regroup_policy.hip (include/myraytracer_amd.h, mrt_set_auto_regroup): the hierarchy judged on the device.  Q_k = the sum of
// (double)(-neg_r2) over the records j of level k (1 .. levels; the top is `clusters`, the others nodes + level_base[k]) with
// j 4^(k-1) < n_pool, never-hit records skipped, in a FIXED order (tests/regroup_policy_ref.py): lane l of the one 256-thread
// workgroup takes j = l, l + 256, .. ascending, lane 0 adds the 256 partials in lane order; Q = ((Q_1 + Q_2) + ..).
//   kQualityDecide: Q -> q_level, q_last; checks++; pending ? (q_ref = Q, pending = gate = 0)
//                   : Q > (double)ratio * q_ref ? (gate = pending = 1, regroups++) : gate = 0.
//   kQualityBaseline: if pending (or `mark`, which sets it first: a regroup the policy did not decide): Q -> q_ref, q_last, q_level,
//                   pending = 0; else nothing.
struct QualityArgs {
    const SphereRec* nodes;
    const SphereRec* clusters;
    RegroupState* state;
    uint32_t levels, n_nodes, n_padded, n_pool;
    uint32_t level_base[kMaxLevels];
    uint32_t mode, mark;
    float ratio;
};
constexpr uint32_t kQualityDecide = 0, kQualityBaseline = 1;
int launch_regroup_quality(const QualityArgs& a, void* stream);

// denoise.hip (include/myraytracer_amd.h, "denoiser"): world-1 texels (y * width + x), rows < height only.
// launch_guide_rays: 6 floats per pixel, the centre ray of the render's camera; launch_guide_fill: {sphere | -1, bits of t} per
// pixel (launch_debug_world_hit) -> 2 float4 per pixel {normal, t} {albedo, bits of the index}; shade / mat_ty: KParams' shade and
// the spheres' material types (i32_data + material_ty_base_idx).
int launch_guide_rays(float* rays, uint32_t width, uint32_t height, const mrt_camera_raw& cam, void* stream);
int launch_guide_fill(const float* rays, const int32_t* hits, const float* shade, const int32_t* mat_ty, float* guides,
                      uint32_t width, uint32_t height, void* stream);
// launch_denoise filters one frame: prm.iterations launches of the a-trous iteration, behind one launch for the variance field
// where the source has to make one first (into pong, where iteration 0 reads it as "the previous iteration's").  `source` names
// where the variance comes from, and with it which ONE of the three payloads below is read.
enum class DenoiseSource : uint32_t { Uniform, Temporal, Tiles };
// Uniform (an accumulation of one frame count): var = S * K.  Accumulated: the luminance stop reads var; Prefiltered: it reads the
// prefiltered var (with K = +inf there is no stop, as for Accumulated); Spatial: the spatial initial variance is the field (K is
// not read) and every iteration is prefiltered.  The values are mrt_debug_denoise_variance's.
enum class UniformVariance : uint32_t { Accumulated = 0, Prefiltered = 1, Spatial = 2 };
struct UniformField { float K; UniformVariance variance; };
// Temporal (the temporal image, mrt_read_temporal): the field is the history's -- colour and length from h0, the luminance
// moments from h1, var as "temporal reprojection" defines it (temporal_variance_kernel) -- and every iteration prefiltered; fb
// gives the alpha alone.
struct TemporalField { const float* h0; const float* h1; uint32_t spatial_len; };
// Tiles (an adaptive accumulation, "Adaptive accumulations" of the header's denoiser section): pixel p of tile (y / 8) * tiles_x +
// x / 8 has n_p = tile_frames[tile], K_p = Kf[n_p] (Kf: K(n) as float for every n the map holds) and mode / spatial_frames choose
// its variance and stop: the field is tile_variance_kernel's, and the centre pixel of an iteration decides on the luminance stop.
struct TileField { const uint32_t* tile_frames; const float* Kf; uint32_t tiles_x, mode, spatial_frames; };
struct DenoiseJob {
    const float* fb;            // the frame, width x height RGBA32F
    const float* S;             // its luminance variance (Uniform and Tiles; the temporal image's is in its history)
    const float* guides;
    float* ping;                // scratch of width x height float4 each: without a field unused for 1 iteration, and ping
    float* pong;                // alone used for 2; with a field pong always
    float* out;                 // width x height RGBA32F
    uint32_t width, height;
    mrt_denoise_params prm;
    DenoiseSource source;
    UniformField uniform;
    TemporalField temporal;
    TileField tiles;
    // The blend with the accumulation ("Blend with the accumulation"): with mix.enabled, for Uniform with a finite K and for
    // Tiles, no iteration runs as the last one -- the last writes the ping / pong buffer its parity names -- and one more launch
    // blends into `out`.  Uniform with K = +inf, and Temporal always: not read, the launches are the ones without it.
    mrt_denoise_mix mix;
};
int launch_denoise(const DenoiseJob& job, void* stream);
inline mrt_denoise_mix denoise_mix_defaults() {
    mrt_denoise_mix p{};
    p.size = sizeof(mrt_denoise_mix);
    p.enabled = 0; p.gain = 1.0f;       // chosen from the table: profiles/denoise_mix_quality.txt
    return p;
}
inline mrt_denoise_params denoise_defaults() {
    mrt_denoise_params p{};
    p.size = sizeof(mrt_denoise_params);
    p.iterations = 5; p.sigma_l = 8.0f; p.normal_exp = 7; p.sigma_z = 0.05f; p.sigma_a = 0.1f;   // tuned: profiles/denoise_quality.txt
    return p;
}


// temporal.hip (include/myraytracer_amd.h, "temporal reprojection"): one step of the history.  fb: the newest frame; rays / guides:
// the first-hit guides of the current camera and scene; shade: the spheres as they are; prev_xyzr: (cx, cy, cz, r) per sphere as
// they were at the previous step; h0 / h1: the history, float4 per texel, in -> out (different buffers); M: the inverse of the
// previous camera's (su, sv, -fw) as rows, o_prev its origin.  launch_temporal_snapshot: floats 0..3 of shade -> prev_xyzr.
struct TemporalArgs {
    const float* fb;
    const float* rays;
    const float* guides;
    const float* shade;
    const float* prev_xyzr;
    const float* h0_in;
    const float* h1_in;
    float* h0_out;
    float* h1_out;
    uint32_t width, height, n_spheres;
    float M[9], o_prev[3];
    float max_history, depth_tol;
};
int launch_temporal_reproject(const TemporalArgs& a, void* stream);
int launch_temporal_snapshot(const float* shade, float* prev_xyzr, uint32_t n_spheres, void* stream);
// The response ("temporal reprojection", steps 4b and 4c): a third history texel H2 = (fr, fg, fb, valid), in -> out with the
// other two pairs.  launch_temporal_reproject_fast: the same step with the fast colour carried along (h2_in / h2_out;
// fast_history as a float); launch_temporal_clamp, queued behind it: h0 the step's output, clamped IN PLACE (every thread reads
// and writes its own texel of h0 alone), h1 / h2 the step's outputs, read only.
struct TemporalFastArgs {
    const float* h2_in;
    float* h2_out;
    float fast_history;
};
struct TemporalClampArgs {
    float* h0;
    const float* h1;
    const float* h2;
    uint32_t width, height;
    float fast_history, clamp_sigma, antilag;
};
int launch_temporal_reproject_fast(const TemporalArgs& a, const TemporalFastArgs& f, void* stream);
int launch_temporal_clamp(const TemporalClampArgs& a, void* stream);
inline mrt_temporal_params temporal_defaults() {
    mrt_temporal_params p{};
    p.size = sizeof(mrt_temporal_params);
    p.max_history = 32; p.spatial_len = 4; p.depth_tol = 0.05f;
    return p;
}
inline mrt_temporal_response temporal_response_defaults() {
    mrt_temporal_response p{};
    p.size = sizeof(mrt_temporal_response);
    p.enabled = 0; p.fast_history = 4; p.clamp_sigma = 2.0f; p.antilag = 1.0f;      // the grid: profiles/temporal_response_quality.txt
    return p;
}
inline mrt_auto_regroup auto_regroup_defaults() {
    mrt_auto_regroup p{};
    p.size = sizeof(mrt_auto_regroup);
    p.enabled = 0; p.check_every = 8; p.ratio = 1.5f;       // measured: profiles/animation_rates.txt, section "auto-regroup"
    return p;
}

}  // namespace mrt
