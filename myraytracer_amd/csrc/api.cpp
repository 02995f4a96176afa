// Host side of the C ABI (include/myraytracer_amd.h): the in-scope parts of the
// reference's `State` (raytracer/src/lib.rs:206-308) -- Subject (Locals + seed texture),
// Object (scene packing + upload), DoubleFramebuffers (ping-pong accumulators) and the
// tail of State::redraw (accumulation weights, reshuffle) -- over HIP allocations and one
// kernel launch per frame instead of wgpu bind groups and a full-screen draw.
//
// There is deliberately no CPU fallback: without a gfx950 device mrt_create fails with
// MRT_ERR_NO_DEVICE.

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>

#include "mrt_ctx.h"

static_assert(sizeof(mrt_args) == 20, "mrt_args layout");
static_assert(sizeof(mrt_locals) == 48, "Locals is 48 bytes (lib.rs:368-377)");
static_assert(sizeof(mrt_world) == 80, "raw::World 64 B + DielectricRange 16 B");
static_assert(offsetof(mrt_world, dielectrics) == MRT_WORLD_BYTES_REFERENCE, "raw::World is the first 64 bytes of mrt_world");
static_assert(sizeof(mrt_sphere) == 36, "mrt_sphere layout");
static_assert(sizeof(mrt_material) == 20 && offsetof(mrt_sphere, material_ty) == 16, "mrt_material is the last five fields of mrt_sphere");
static_assert(sizeof(mrt_camera) == 52, "mrt_camera layout");
static_assert(sizeof(mrt_camera_raw) == 80, "mrt_camera_raw layout");
static_assert(sizeof(mrt::SphereRec) == 16, "SphereRec layout");
static_assert(sizeof(mrt_noise_report) == 96 && offsetof(mrt_noise_report, pixels) == 16 && offsetof(mrt_noise_report, threshold) == 40 &&
              offsetof(mrt_noise_report, noise_factor) == 48 && offsetof(mrt_noise_report, max_se) == 88, "mrt_noise_report layout");
static_assert(sizeof(mrt::NoiseSums) == 48, "NoiseSums layout");
static_assert(sizeof(mrt_auto_regroup) == 32 && sizeof(mrt_regroup_stats) == 72 && offsetof(mrt_regroup_stats, q_ref) == 16 &&
              offsetof(mrt_regroup_stats, levels) == 64, "mrt_auto_regroup / mrt_regroup_stats layout");
static_assert(sizeof(mrt_present_info) == 40 && offsetof(mrt_present_info, frames_done) == 8 &&
              offsetof(mrt_present_info, ring_depth) == 36, "mrt_present_info layout");
static_assert(sizeof(mrt_view) == 32 && offsetof(mrt_view, rel_floor) == 20, "mrt_view layout");

using mrt::fail, mrt::free_device, mrt::free_pinned, mrt::local_texels, mrt::local_texels_min1, mrt::tiles_min1, mrt::total_bands, mrt::alloc_frame_buffers, mrt::free_world;

namespace {

thread_local std::string g_err;   // for failures before a ctx exists

void free_frame_buffers(mrt_ctx* c) {
    mrt::free_noise_buffers(c);
    mrt::free_denoise_buffers(c);
    mrt::free_tile_frames(c);
    free_device(c->d_seeds, c->d_fb[0], c->d_fb[1]);
    for (auto& S : c->slot) {
        free_device(S.d_tile_cost, S.d_tile_order, S.d_sort_scratch, S.d_pix_acc, S.d_tile_list);
        free_pinned(S.h_tile_list);
        S.pix_acc_layers = 0; S.cost_first_layer = 0; S.cost_layers = 1;
        S.cost_valid = false;
        S.order_kind = 0; S.order_n = 0; S.order_pilot = false;
    }
}

void reset_locals(mrt_ctx* c) {
    // lib.rs:419-426: initial Locals
    std::memset(&c->locals, 0, sizeof c->locals);
    c->locals.shape[0] = c->args.width;
    c->locals.shape[1] = c->args.height;
    c->locals.samples_per_frame = c->args.samples_per_frame;
    c->locals.ray_depth = c->args.ray_depth;
    c->locals.framebuffer_weight = 0.0f;
    c->frames_done = 0;
    c->noise_c2 = 1.0;
}

uint64_t splitmix64_at(uint64_t seed, uint64_t k) {
    uint64_t z = seed + (k + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// copy between a full bottom-up image on the host and this shard's packed rows on the device
int copy_rows(mrt_ctx* c, void* device_base, void* host_full, size_t texel_bytes, bool to_device) {
    const uint32_t W = c->args.width, H = c->args.height;
    const size_t band_bytes = (size_t)mrt::kBandRows * W * texel_bytes;
    for (uint32_t b = 0; b < c->local_bands; b++) {
        const uint32_t gb = b * c->shard_world + c->shard_rank;
        const uint32_t y0 = gb * mrt::kBandRows;
        if (y0 >= H) break;
        const uint32_t rows = (H - y0 < mrt::kBandRows) ? H - y0 : mrt::kBandRows;
        char* dptr = (char*)device_base + b * band_bytes;
        char* hptr = (char*)host_full + (size_t)y0 * W * texel_bytes;
        const size_t bytes = (size_t)rows * W * texel_bytes;
        if (to_device) HIP_TRY(c, hipMemcpyAsync(dptr, hptr, bytes, hipMemcpyHostToDevice, c->stream));
        else HIP_TRY(c, hipMemcpyAsync(hptr, dptr, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    MRT_TRY(mrt::wait_stream(c, c->stream, __func__));
    return MRT_OK;
}

}  // namespace

namespace mrt {

int fail(mrt_ctx* ctx, int status, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_err = buf;
    return status;
}
void set_global_error(const char* msg) { g_err = msg ? msg : ""; }

void free_world(mrt_ctx* c) {
    free_device(c->d_spheres, c->d_clusters, c->d_nodes, c->d_boxes, c->d_boxes_open, c->d_shade, c->d_top_mfma, c->d_member_index,
                c->d_regroup, c->d_prev_xyzr, c->d_vec4, c->d_f32, c->d_i32, c->d_cam_masks);
    c->cam_mask_entries = 0;
    c->cam_mask_built = 0;
    c->cam_masks_in_force = false;
    c->cam_lists_in_force = false;
    c->cam_mask_gen++;
    c->have_world = false;
    c->guides_stale = true;
    drop_temporal_history(c);           // (the sphere indices it holds belong to the scene that goes)
}

int alloc_first_colour_sums(mrt_ctx* c, mrt_ctx::FrameSlot& S) {
    HIP_TRY(c, hipMalloc(&S.d_pix_acc, local_texels_min1(c) * 16));
    HIP_TRY(c, hipMemsetAsync(S.d_pix_acc, 0, local_texels_min1(c) * 16, c->stream));
    S.pix_acc_layers = 1;
    return MRT_OK;
}

// a shard's buffers while alloc_frame_buffers builds them: the context takes them over only when all of them exist
struct ShardBuffers {
    uint32_t* seeds = nullptr;
    float* fb[2] = {nullptr, nullptr};
    struct Slot { uint32_t *cost = nullptr, *order = nullptr, *scratch = nullptr; void* pix_acc = nullptr; } slot[mrt_ctx::kMaxFrameSlots];
    float *noise_s = nullptr, *noise_tiles = nullptr;
    void* noise_partials = nullptr;
    uint32_t n_waves = 0, cus = 0;
    void release() {
        free_device(seeds, fb[0], fb[1], noise_s, noise_tiles, noise_partials);
        for (auto& S : slot) free_device(S.cost, S.order, S.scratch, S.pix_acc);
    }
};

static int build_shard_buffers(mrt_ctx* c, uint32_t rank, uint32_t world, uint32_t local_bands, ShardBuffers& B) {
    const size_t n = (size_t)local_bands * kBandRows * c->args.width, n1 = n ? n : 1;
    const uint32_t tiles_x = (c->args.width + mrt::kTileW - 1) / mrt::kTileW;
    const size_t tiles1 = (size_t)tiles_x * local_bands ? (size_t)tiles_x * local_bands : 1;
    HIP_TRY(c, hipMalloc(&B.seeds, n * 4 * sizeof(uint32_t)));
    HIP_TRY(c, hipMalloc(&B.fb[0], n * 4 * sizeof(float)));
    HIP_TRY(c, hipMalloc(&B.fb[1], n * 4 * sizeof(float)));
    HIP_TRY(c, hipMemsetAsync(B.fb[0], 0, n * 4 * sizeof(float), c->stream));
    HIP_TRY(c, hipMemsetAsync(B.fb[1], 0, n * 4 * sizeof(float), c->stream));
    for (auto& S : B.slot) {
        HIP_TRY(c, hipMalloc(&S.cost, tiles1 * sizeof(uint32_t)));
        HIP_TRY(c, hipMalloc(&S.order, tiles1 * sizeof(uint32_t)));
        HIP_TRY(c, hipMalloc(&S.scratch, (1024 + 16) * sizeof(uint32_t)));
        HIP_TRY(c, hipMemsetAsync(S.scratch, 0, (1024 + 16) * sizeof(uint32_t), c->stream));   // [1024] = the tile queue's counter
        if (&S - B.slot >= 2) continue;        // further slots (pixel-starved shards only) get their colour sums on first use
        HIP_TRY(c, hipMalloc(&S.pix_acc, n1 * 16));
        HIP_TRY(c, hipMemsetAsync(S.pix_acc, 0, n1 * 16, c->stream));
    }
    // as many persistent single-wave workgroups as the chip holds
    {
        hipDeviceProp_t prop;
        HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
        int wpc = 0;
        if (mrt::render_waves_per_cu(&wpc) != 0 || wpc <= 0) wpc = 16;
        if (c->waves_per_cu_override > 0) wpc = c->waves_per_cu_override;
        B.n_waves = (uint32_t)prop.multiProcessorCount * (uint32_t)wpc;
        B.cus = (uint32_t)prop.multiProcessorCount;
    }
    int e = mrt::launch_fill_seeds(B.seeds, c->seed, c->args.width, c->args.height, rank, world, local_bands, c->stream);
    if (e) return fail(c, MRT_ERR_HIP, "fill_seeds launch failed: %s", hipGetErrorString((hipError_t)e));
    if (c->noise_on) MRT_TRY(alloc_noise_set(c, local_bands, &B.noise_s, &B.noise_tiles, &B.noise_partials));
    return MRT_OK;
}

// Subject::new + DoubleFramebuffers::new for shard `rank` of `world` (lib.rs:389-415, 514-538).  The new buffers are all
// allocated before the old ones are released, so a refused allocation leaves the context -- its shard, its buffers, its frame
// slots -- exactly as it was and the call can simply be repeated; the price is both sets side by side for the moment of a call
// that happens once per shard assignment.
int alloc_frame_buffers(mrt_ctx* c, uint32_t rank, uint32_t world) {
    const uint32_t nb = total_bands(c->args.height);
    const uint32_t local_bands = (nb + world - 1) / world;   // same on every rank (gather-friendly)
    ShardBuffers B;
    const int st = build_shard_buffers(c, rank, world, local_bands, B);
    if (st != MRT_OK) {
        B.release();                             // (hipFree waits for the memsets queued on them)
        return st;
    }
    free_frame_buffers(c);
    c->gather_has_s = false;            // (a gathered S was another shard layout's; the gathered colour stays readable, as before)
    c->shard_rank = rank; c->shard_world = world;
    c->local_bands = local_bands;
    c->cam_mask_gen++;                  // (the camera masks are per texel of the shard)
    c->d_seeds = B.seeds; c->d_fb[0] = B.fb[0]; c->d_fb[1] = B.fb[1];
    c->tiles_x = (c->args.width + mrt::kTileW - 1) / mrt::kTileW;
    c->n_tiles = c->tiles_x * c->local_bands;
    for (uint32_t i = 0; i < mrt_ctx::kMaxFrameSlots; i++) {
        mrt_ctx::FrameSlot& S = c->slot[i];
        S.d_tile_cost = B.slot[i].cost; S.d_tile_order = B.slot[i].order; S.d_sort_scratch = B.slot[i].scratch;
        S.d_pix_acc = B.slot[i].pix_acc;
        S.pix_acc_layers = S.d_pix_acc ? 1 : 0;
    }
    c->frame_slots = 2;
    c->last_slot = 0;               // (what mrt_debug_read_pixel_costs reads: a slot that has colour sums)
    c->width.invalidate();
    c->inputs_dirty = true;
    c->n_waves = B.n_waves; c->cus = B.cus;
    c->target = 0;
    if (c->noise_on) {
        c->d_noise_s = B.noise_s; c->d_noise_tiles = B.noise_tiles; c->d_noise_partials = B.noise_partials;
        c->noise_first = c->noise_seq + 1;          // (reports of the old geometry are discarded)
    }
    return MRT_OK;
}

// Bounded host waits.  Every wait for the GPU in this library goes through these: poll (spin briefly, then sleep in growing
// steps up to 200 us -- a frame is 0.2 ms at its shortest) until the event / stream is complete or the context's deadline has
// passed; then fail with MRT_ERR_STALLED and a message that names the wait, so that a stall is a loud status and never a silent
// hang (round 4's parity campaign lost a 420-s run to one: DESIGN_HISTORY.md, round 5).
template <typename Query>
static int bounded_wait(mrt_ctx* c, Query query, const char* what) {
    if (c->stalled) return fail(c, MRT_ERR_STALLED, "%s: the context has stalled before (destroy it)", what);
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = query();
        if (q == hipSuccess) return MRT_OK;
        if (q != hipErrorNotReady) return fail(c, MRT_ERR_HIP, "%s: %s", what, hipGetErrorString(q));
        (void)hipGetLastError();                                        // (hipErrorNotReady is not an error)
        const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (c->wait_timeout_s > 0.0 && waited > c->wait_timeout_s) {
            c->stalled = true;
            return fail(c, MRT_ERR_STALLED, "stalled in %s: not complete after %.1f s (mrt_set_wait_timeout)", what, waited);
        }
        if (waited < 50e-6) continue;                                   // spin
        std::this_thread::sleep_for(std::chrono::microseconds(waited < 2e-3 ? 20 : waited < 50e-3 ? 100 : 200));
    }
}
int wait_event(mrt_ctx* c, hipEvent_t ev, const char* what) { return bounded_wait(c, [&]() { return hipEventQuery(ev); }, what); }
int wait_stream(mrt_ctx* c, hipStream_t s, const char* what) { return bounded_wait(c, [&]() { return hipStreamQuery(s); }, what); }
// everything this context has in flight (the side streams, then the caller's stream)
int wait_all(mrt_ctx* c, const char* what) {
    char buf[160];
    for (uint32_t i = 0; i < mrt_ctx::kMaxFrameSlots; i++) {
        mrt_ctx::FrameSlot& S = c->slot[i];
        if (!S.stream) continue;
        std::snprintf(buf, sizeof buf, "%s (side stream of slot %u, last frame %llu, %u frames in flight)", what, i,
                      (unsigned long long)S.render_seq, c->frame_slots);
        MRT_TRY(wait_stream(c, S.stream, buf));
        S.render_pending = false;
    }
    if (c->stream) {
        std::snprintf(buf, sizeof buf, "%s (the context's stream, frame %llu)", what, (unsigned long long)c->frame_seq);
        MRT_TRY(wait_stream(c, c->stream, buf));
    }
    if (c->present_stream) {
        std::snprintf(buf, sizeof buf, "%s (the present copies' stream, present %llu)", what, (unsigned long long)c->present_seq);
        MRT_TRY(wait_stream(c, c->present_stream, buf));
    }
    return MRT_OK;
}

int read_rows(mrt_ctx* c, const char* who, const void* src, void* out, size_t cap, size_t texel_bytes) {
    const size_t n = (c->shard_world == 1 ? (size_t)c->args.width * c->args.height : local_texels(c)) * (texel_bytes / sizeof(float));
    if (cap < n) return fail(c, MRT_ERR_TOO_SMALL, "%s: need %zu floats", who, n);
    if (c->shard_world == 1) return copy_rows(c, const_cast<void*>(src), out, texel_bytes, false);
    HIP_TRY(c, hipMemcpyAsync(out, src, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    MRT_TRY(mrt::wait_stream(c, c->stream, who));
    return MRT_OK;
}

}  // namespace mrt

// mrt_debug_check_context's finding: 1, with the reason in `why`
static int check_finding(char* why, size_t cap, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
static int check_finding(char* why, size_t cap, const char* fmt, ...) {
    if (why && cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(why, cap, fmt, ap);
        va_end(ap);
    }
    return 1;
}

extern "C" {

int mrt_abi_version(void) { return MRT_ABI_VERSION; }

const char* mrt_status_string(int s) {
    switch (s) {
        case MRT_OK: return "ok";
        case MRT_ERR_INVALID_ARG: return "invalid argument";
        case MRT_ERR_NO_DEVICE: return "no usable HIP device";
        case MRT_ERR_HIP: return "HIP runtime error";
        case MRT_ERR_NO_SCENE: return "no scene set";
        case MRT_ERR_BAD_SCENE: return "invalid scene data";
        case MRT_ERR_TOO_SMALL: return "buffer too small";
        case MRT_ERR_STATE: return "call not allowed in this state";
        case MRT_ERR_IO: return "i/o error";
        case MRT_ERR_STALLED: return "a wait for the GPU passed its deadline";
        default: return "unknown status";
    }
}

const char* mrt_last_error(mrt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

void mrt_args_default(mrt_args* out) {
    if (!out) return;
    out->width = 0; out->height = 0;
    out->samples_per_frame = 1; out->ray_depth = 50; out->max_framebuffer_weight = 1.0f;
}

void mrt_args_resolve_size(mrt_args* a) {
    if (!a) return;
    if (a->width == 0 && a->height == 0) { a->width = MRT_DEFAULT_WIDTH; a->height = MRT_DEFAULT_HEIGHT; }
    else if (a->width == 0) a->width = a->height;
    else if (a->height == 0) a->height = a->width;
}

float mrt_frame_weight(uint32_t frames_done, float max_w) {
    if (frames_done == 0) return 0.0f;                                 // lib.rs:424
    const float w = (float)frames_done / (float)(frames_done + 1u);    // lib.rs:304
    return max_w < w ? max_w : w;                                      // f32::min, lib.rs:301-304
}

void mrt_pixel_seed(uint64_t seed, uint64_t pixel_index, uint32_t out[4]) {
    const uint64_t a = splitmix64_at(seed, 2u * pixel_index), b = splitmix64_at(seed, 2u * pixel_index + 1u);
    out[0] = (uint32_t)a; out[1] = (uint32_t)(a >> 32); out[2] = (uint32_t)b; out[3] = (uint32_t)(b >> 32);
    if ((out[0] | out[1] | out[2] | out[3]) == 0u) {
        out[0] = 0x9E3779B9u; out[1] = 0x7F4A7C15u; out[2] = 0xBF58476Du; out[3] = 0x1CE4E5B9u;
    }
}

void mrt_frame_shuffle(uint64_t seed, uint32_t frame, uint32_t out[4]) {
    if (frame == 0) { out[0] = out[1] = out[2] = out[3] = 0; return; }  // lib.rs:422
    const uint64_t s2 = seed ^ 0xD1B54A32D192ED03ull;
    const uint64_t a = splitmix64_at(s2, 2ull * frame), b = splitmix64_at(s2, 2ull * frame + 1u);
    out[0] = (uint32_t)a; out[1] = (uint32_t)(a >> 32); out[2] = (uint32_t)b; out[3] = (uint32_t)(b >> 32);
}

int mrt_camera_derive(const mrt_camera* cam, mrt_camera_raw* out) {
    if (!cam || !out) return MRT_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    out->mode = cam->mode;
    if (cam->mode == 0) return MRT_OK;
    if (cam->mode != 1) return MRT_ERR_INVALID_ARG;
    double lf[3], la[3], up[3], w[3], u[3], v[3];
    for (int i = 0; i < 3; i++) { lf[i] = cam->lookfrom[i]; la[i] = cam->lookat[i]; up[i] = cam->vup[i]; }
    for (int i = 0; i < 3; i++) w[i] = lf[i] - la[i];
    const double wl = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    for (int i = 0; i < 3; i++) w[i] /= wl;
    u[0] = up[1] * w[2] - up[2] * w[1];
    u[1] = up[2] * w[0] - up[0] * w[2];
    u[2] = up[0] * w[1] - up[1] * w[0];
    const double ul = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    for (int i = 0; i < 3; i++) u[i] /= ul;
    v[0] = w[1] * u[2] - w[2] * u[1];
    v[1] = w[2] * u[0] - w[0] * u[2];
    v[2] = w[0] * u[1] - w[1] * u[0];
    const double deg = 3.14159265358979323846 / 180.0;
    const double focus = cam->focus_dist;
    const double s = std::tan(0.5 * (double)cam->vfov_deg * deg) * focus;
    const double r = std::tan(0.5 * (double)cam->defocus_angle_deg * deg) * focus;
    out->defocus = cam->defocus_angle_deg > 0.0f;
    for (int i = 0; i < 3; i++) {
        out->origin[i] = cam->lookfrom[i];
        out->su[i] = (float)(s * u[i]);
        out->sv[i] = (float)(s * v[i]);
        out->fw[i] = (float)(focus * w[i]);
        out->ru[i] = (float)(r * u[i]);
        out->rv[i] = (float)(r * v[i]);
    }
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(out->su[i]) || !std::isfinite(out->sv[i]) || !std::isfinite(out->fw[i]) ||
            !std::isfinite(out->ru[i]) || !std::isfinite(out->rv[i]) || !std::isfinite(out->origin[i]))
            return MRT_ERR_INVALID_ARG;
    return MRT_OK;
}

// lib.rs:722-799
int mrt_pack_world(const mrt_sphere* sp, size_t n, mrt_world* world,
                   float* vec4, size_t cap_vec4, size_t* n_vec4,
                   float* f32, size_t cap_f32, size_t* n_f32,
                   int32_t* i32, size_t cap_i32, size_t* n_i32) {
    if ((!sp && n) || !world || !vec4 || !f32 || !i32 || !n_vec4 || !n_f32 || !n_i32) return MRT_ERR_INVALID_ARG;
    if (n > (size_t)INT32_MAX / 4) return MRT_ERR_INVALID_ARG;
    size_t nl = 0, nm = 0, nd = 0;
    for (size_t i = 0; i < n; i++) {
        switch (sp[i].material_ty) {
            case MRT_LAMBERTIAN: nl++; break;
            case MRT_METAL: nm++; break;
            case MRT_DIELECTRIC: nd++; break;
            default: return MRT_ERR_BAD_SCENE;
        }
    }
    if (cap_vec4 < n + nl + nm || cap_f32 < n + nm + nd || cap_i32 < 2 * n) return MRT_ERR_TOO_SMALL;
    std::memset(world, 0, sizeof *world);
    size_t v = 0, f = 0, k = 0;
    auto push4 = [&](const float* p) { vec4[4 * v] = p[0]; vec4[4 * v + 1] = p[1]; vec4[4 * v + 2] = p[2]; vec4[4 * v + 3] = 1.0f; v++; };
    world->spheres.center_base_idx = (int32_t)v;
    for (size_t i = 0; i < n; i++) push4(sp[i].center);
    world->spheres.radius_base_idx = (int32_t)f;
    for (size_t i = 0; i < n; i++) f32[f++] = sp[i].radius;
    world->spheres.material_ty_base_idx = (int32_t)k;
    for (size_t i = 0; i < n; i++) i32[k++] = sp[i].material_ty;
    world->spheres.material_idx_base_idx = (int32_t)k;
    {
        int32_t cl = 0, cm = 0, cd = 0;
        for (size_t i = 0; i < n; i++)
            i32[k++] = sp[i].material_ty == MRT_LAMBERTIAN ? cl++ : sp[i].material_ty == MRT_METAL ? cm++ : cd++;
    }
    world->spheres.length = (int32_t)n;
    world->lambertians.albedo_base_idx = (int32_t)v;
    for (size_t i = 0; i < n; i++) if (sp[i].material_ty == MRT_LAMBERTIAN) push4(sp[i].albedo);
    world->lambertians.length = (int32_t)nl;
    world->metals.albedo_base_idx = (int32_t)v;
    for (size_t i = 0; i < n; i++) if (sp[i].material_ty == MRT_METAL) push4(sp[i].albedo);
    world->metals.fuzz_base_idx = (int32_t)f;
    for (size_t i = 0; i < n; i++) if (sp[i].material_ty == MRT_METAL) f32[f++] = sp[i].param;
    world->metals.length = (int32_t)nm;
    world->dielectrics.ior_base_idx = (int32_t)f;
    for (size_t i = 0; i < n; i++) if (sp[i].material_ty == MRT_DIELECTRIC) f32[f++] = sp[i].param;
    world->dielectrics.length = (int32_t)nd;
    *n_vec4 = v; *n_f32 = f; *n_i32 = k;
    return MRT_OK;
}

int mrt_create(const mrt_args* args, uint64_t seed, int device, mrt_ctx** out) {
    if (!args || !out) return fail(nullptr, MRT_ERR_INVALID_ARG, "mrt_create: null argument");
    *out = nullptr;
    mrt_args a = *args;
    mrt_args_resolve_size(&a);
    if (a.width > (1u << 20) || a.height > (1u << 20))
        return fail(nullptr, MRT_ERR_INVALID_ARG, "mrt_create: image %ux%u too large", a.width, a.height);
    // (The frames in flight of a pixel-starved shard -- up to 8, each on a side stream of its own -- only run side by side on
    // hardware queues of their own, and HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES of them, 4 by default.  That
    // variable is the HOST's to set, before its first HIP call: INTEGRATION.md 2a; the Python package and bench.py do.  This
    // library does not touch the environment: it measures how many of its streams really run at a time when it first wants
    // more than two frames in flight -- probe_stream_concurrency -- and holds the schedule to that.)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, MRT_ERR_NO_DEVICE, "mrt_create: no HIP device (this backend has no CPU fallback)");
    if (device < 0 || device >= ndev)
        return fail(nullptr, MRT_ERR_NO_DEVICE, "mrt_create: device %d out of range (%d present)", device, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return fail(nullptr, MRT_ERR_NO_DEVICE, "mrt_create: cannot query device %d", device);
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, MRT_ERR_NO_DEVICE, "mrt_create: device %d is %s; kernels are built for gfx950 only",
                    device, prop.gcnArchName);
    mrt_ctx* c = new (std::nothrow) mrt_ctx();
    if (!c) return fail(nullptr, MRT_ERR_INVALID_ARG, "mrt_create: out of host memory");
    c->device = device; c->args = a; c->seed = seed;
    if (const char* t = std::getenv("MRT_WAIT_TIMEOUT_S")) {
        char* end = nullptr;
        const double v = std::strtod(t, &end);
        if (end != t && v >= 0.0 && std::isfinite(v)) c->wait_timeout_s = v;
    }
    c->cam_raw.mode = 0;
    reset_locals(c);
    // everything the context owns from the start; a failure names the refused call (mrt_last_error(NULL)) and mrt_destroy
    // releases whatever the half-built context holds
    auto init = [&]() -> int {
        HIP_TRY(c, hipSetDevice(device));
        HIP_TRY(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
        c->stream = c->own_stream;
        // (slots 0 and 1 now; the further ones -- pixel-starved shards only -- when redraw_frames first needs them)
        for (uint32_t i = 0; i < 2; i++) MRT_TRY(mrt::create_slot_streams(c, c->slot[i]));
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_inputs, hipEventDisableTiming));
        for (uint32_t i = 0; i < mrt_ctx::kEventRing; i++) {
            HIP_TRY(c, hipEventCreate(&c->ev_start[i]));
            HIP_TRY(c, hipEventCreate(&c->ev_stop[i]));
        }
        HIP_TRY(c, hipMalloc(&c->d_counters, 16 * sizeof(unsigned long long)));
        HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, 16 * sizeof(unsigned long long), c->stream));
        HIP_TRY(c, hipHostMalloc((void**)&c->h_stats, 5 * mrt_ctx::kMaxFrameSlots * sizeof(unsigned long long), hipHostMallocDefault));
        return alloc_frame_buffers(c, 0, 1);
    };
    const int st = init();
    if (st != MRT_OK) {
        g_err = "mrt_create: " + c->err;
        mrt_destroy(c);
        return st;
    }
    *out = c;
    return MRT_OK;
}

void mrt_destroy(mrt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    // A context that has stalled (MRT_ERR_STALLED) may hold work that never finishes: hipFree, hipStreamDestroy and
    // hipEventDestroy all wait for it.  Its device resources are then left to the process' exit rather than waited for.
    if (mrt::wait_all(c, "mrt_destroy") != MRT_OK || c->stalled) {
        delete c;
        return;
    }
    free_frame_buffers(c);
    for (auto& S : c->slot) {
        if (S.render_done) (void)hipEventDestroy(S.render_done);
        if (S.finalize_done) (void)hipEventDestroy(S.finalize_done);
        if (S.stats_ready) (void)hipEventDestroy(S.stats_ready);
        if (S.stream) (void)hipStreamDestroy(S.stream);
    }
    if (c->ev_inputs) (void)hipEventDestroy(c->ev_inputs);
    free_world(c);
    free_device(c->d_counters, c->d_wave_log, c->d_gather, c->d_gather_stage);
    free_pinned(c->h_stats);
    if (c->ev_gather) (void)hipEventDestroy(c->ev_gather);
    if (c->ev_gather_root) (void)hipEventDestroy(c->ev_gather_root);
    for (uint32_t i = 0; i < mrt_ctx::kEventRing; i++) {
        if (c->ev_start[i]) (void)hipEventDestroy(c->ev_start[i]);
        if (c->ev_stop[i]) (void)hipEventDestroy(c->ev_stop[i]);
    }
    for (auto& E : c->present_ring) {
        free_device(E.d_img);
        free_pinned(E.h_img);
        if (E.copied) (void)hipEventDestroy(E.copied);
    }
    free_device(c->d_present_tables, c->d_noise_sums);
    if (c->ev_presented) (void)hipEventDestroy(c->ev_presented);
    if (c->present_stream) (void)hipStreamDestroy(c->present_stream);
    for (auto& E : c->noise_ring)
        if (E.copied) (void)hipEventDestroy(E.copied);
    free_pinned(c->h_noise_sums);
    if (c->noise_stream) (void)hipStreamDestroy(c->noise_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int mrt_set_shard(mrt_ctx* c, uint32_t rank, uint32_t world) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (world == 0 || rank >= world) return fail(c, MRT_ERR_INVALID_ARG, "mrt_set_shard: rank %u of %u", rank, world);
    if (c->frames_done != 0) return fail(c, MRT_ERR_STATE, "mrt_set_shard: frames already rendered; call mrt_reset first");
    if (c->temporal_on && world > 1) return fail(c, MRT_ERR_STATE, "mrt_set_shard: temporal reprojection is on (a shard has no history; mrt_set_temporal)");
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, __func__));
    for (auto& E : c->present_ring) E.state = mrt_ctx::PresentEntry::kFree;      // (the presented images are discarded)
    c->present_dropped = 0;
    return alloc_frame_buffers(c, rank, world);
}

int mrt_set_stream(mrt_ctx* c, void* s) {
    if (!c) return MRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, __func__));
    c->stream = s ? (hipStream_t)s : c->own_stream;
    c->inputs_dirty = true;
    return MRT_OK;
}

int mrt_set_camera(mrt_ctx* c, const mrt_camera* cam) {
    if (!c || !cam) return MRT_ERR_INVALID_ARG;
    mrt_camera_raw raw;
    int st = mrt_camera_derive(cam, &raw);
    if (st != MRT_OK) return fail(c, st, "mrt_set_camera: degenerate or invalid camera");
    // like the geometry (mrt_set_world_raw): moderate, so that no discriminant of a camera ray can overflow
    for (int k = 0; k < 3; k++)
        if (raw.mode != 0 && !(std::fabs(raw.origin[k]) <= 1.0e7f && std::fabs(raw.ru[k]) <= 1.0e7f && std::fabs(raw.rv[k]) <= 1.0e7f))
            return fail(c, MRT_ERR_INVALID_ARG, "mrt_set_camera: |lookfrom| or the lens radius exceeds 1e7");
    c->cam_raw = raw;
    c->cam_mask_gen++;
    c->guides_stale = true;
    for (auto& S : c->slot) S.cost_valid = false;
    c->width.invalidate();              // (the launch-width controller starts over with the new workload)
    return MRT_OK;
}

int mrt_shard_info(mrt_ctx* c, uint32_t* rank, uint32_t* world, uint32_t* local_rows, uint32_t* width) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (rank) *rank = c->shard_rank;
    if (world) *world = c->shard_world;
    if (local_rows) *local_rows = c->local_bands * mrt::kBandRows;
    if (width) *width = c->args.width;
    return MRT_OK;
}

int mrt_set_seeds(mrt_ctx* c, const uint32_t* seeds, size_t n_u32) {
    if (!c || !seeds) return MRT_ERR_INVALID_ARG;
    if (n_u32 != (size_t)c->args.width * c->args.height * 4) return fail(c, MRT_ERR_INVALID_ARG, "mrt_set_seeds: expected W*H*4 u32");
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, __func__));
    c->inputs_dirty = true;
    return copy_rows(c, c->d_seeds, const_cast<uint32_t*>(seeds), 16, true);
}

int mrt_read_seeds(mrt_ctx* c, uint32_t* out, size_t cap) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    const size_t n = local_texels(c) * 4;
    if (cap < n) return fail(c, MRT_ERR_TOO_SMALL, "mrt_read_seeds: need %zu u32", n);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, c->d_seeds, n * 4, hipMemcpyDeviceToHost, c->stream));
    MRT_TRY(mrt::wait_stream(c, c->stream, __func__));
    return MRT_OK;
}

int mrt_set_wait_timeout(mrt_ctx* c, double seconds) {
    if (!c || !(seconds >= 0.0) || !std::isfinite(seconds)) return MRT_ERR_INVALID_ARG;
    c->wait_timeout_s = seconds;
    return MRT_OK;
}

// div_unscaled / sqrt_unscaled (kernels.hip) against hipcc's `/` and sqrtf(), on the device, over whole operand ranges
int mrt_debug_arith(mrt_ctx* c, int mode, const uint32_t bits_range[4], uint64_t count, uint64_t seed, uint64_t out[3]) {
    if (!c || !bits_range || !out || mode < 0 || mode > 2) return MRT_ERR_INVALID_ARG;
    if (bits_range[0] > bits_range[1] || (mode != 0 && bits_range[2] > bits_range[3]))
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_debug_arith: empty range");
    HIP_TRY(c, hipSetDevice(c->device));
    unsigned long long* d_out = nullptr;
    HIP_TRY(c, hipMalloc((void**)&d_out, 3 * sizeof(unsigned long long)));
    const unsigned long long init[3] = {0ull, 0ull, ~0ull};
    hipError_t e = hipMemcpyAsync(d_out, init, sizeof init, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = (hipError_t)mrt::launch_arith_check(mode, bits_range, count, seed, d_out, c->stream);
    unsigned long long host[3] = {0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(host, d_out, sizeof host, hipMemcpyDeviceToHost, c->stream);
    int ws = MRT_OK;
    if (e == hipSuccess) ws = mrt::wait_stream(c, c->stream, "mrt_debug_arith");
    if (ws != MRT_OK) return ws;            // (stalled: d_out is left to the process)
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(c, MRT_ERR_HIP, "mrt_debug_arith failed: %s", hipGetErrorString(e));
    for (int k = 0; k < 3; k++) out[k] = host[k];
    return MRT_OK;
}

int mrt_debug_arith_pairs(mrt_ctx* c, const float* x, const float* y, size_t n, uint32_t* out) {
    if (!c || !x || !y || !out || n > (1u << 28)) return MRT_ERR_INVALID_ARG;
    if (n == 0) return MRT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    float* d_xy = nullptr;
    uint32_t* d_o = nullptr;
    HIP_TRY(c, hipMalloc((void**)&d_xy, 2 * n * sizeof(float)));
    hipError_t e = hipSuccess;
    const char* what = "mrt_debug_arith_pairs";
    HIP_CHAIN(e, what, hipMalloc((void**)&d_o, 6 * n * sizeof(uint32_t)));
    if (e == hipSuccess) e = hipMemcpyAsync(d_xy, x, n * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_xy + n, y, n * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = (hipError_t)mrt::launch_arith_pairs(d_xy, d_xy + n, (uint32_t)n, d_o, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_o, 6 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    int ws = MRT_OK;
    if (e == hipSuccess) ws = mrt::wait_stream(c, c->stream, "mrt_debug_arith_pairs");
    if (ws != MRT_OK) return ws;
    (void)hipFree(d_xy);
    if (d_o) (void)hipFree(d_o);
    if (e != hipSuccess) return fail(c, MRT_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    return MRT_OK;
}

int mrt_sync(mrt_ctx* c) {
    if (!c) return MRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, __func__));
    return MRT_OK;
}

int mrt_reset(mrt_ctx* c) {
    if (!c) return MRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::wait_all(c, __func__));
    for (auto& E : c->present_ring) E.state = mrt_ctx::PresentEntry::kFree;      // (the presented images are discarded)
    c->present_dropped = 0;
    const size_t bytes = local_texels(c) * 4 * sizeof(float);
    HIP_TRY(c, hipMemsetAsync(c->d_fb[0], 0, bytes, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_fb[1], 0, bytes, c->stream));
    if (c->d_noise_s) HIP_TRY(c, hipMemsetAsync(c->d_noise_s, 0, local_texels(c) * sizeof(float), c->stream));
    c->noise_first = c->noise_seq + 1;          // (the reports not yet read are discarded)
    HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, 16 * sizeof(unsigned long long), c->stream));
    for (auto& S : c->slot)          // the tile queues' counters (normally left at zero by every finalize pass)
        if (S.d_sort_scratch) HIP_TRY(c, hipMemsetAsync(S.d_sort_scratch + 1024, 0, sizeof(uint32_t), c->stream));
    c->inputs_dirty = true;      // the next redraw's side stream waits for these memsets (ev_inputs)
    const uint32_t spp = c->locals.samples_per_frame, mode = c->locals.rng_mode;
    reset_locals(c);
    c->locals.samples_per_frame = spp;
    c->locals.rng_mode = mode;
    c->target = 0;
    c->tiles_diverged = false;                  // (every tile at 0 frames again: the per-tile counts are re-initialised on use)
    c->tile_frames.clear();
    return MRT_OK;
}

int mrt_get_locals(mrt_ctx* c, mrt_locals* out) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    *out = c->locals;
    return MRT_OK;
}

int mrt_set_rng_shuffle(mrt_ctx* c, const uint32_t s[4]) {
    if (!c || !s) return MRT_ERR_INVALID_ARG;
    std::memcpy(c->locals.rng_shuffle, s, 16);
    c->shuffle_overridden = true;          // the next frame is rendered on its own (mrt_render does not batch it)
    return MRT_OK;
}

int mrt_set_rng_mode(mrt_ctx* c, uint32_t mode) {
    if (!c || mode > MRT_RNG_COUNTER) return MRT_ERR_INVALID_ARG;
    c->locals.rng_mode = mode;
    c->width.invalidate();
    return MRT_OK;
}

int mrt_set_draw_counting(mrt_ctx* c, int enabled) {
    if (!c) return MRT_ERR_INVALID_ARG;
    c->count_draws = enabled != 0;
    return MRT_OK;
}

int mrt_set_samples_per_frame(mrt_ctx* c, uint32_t spp) {
    if (!c) return MRT_ERR_INVALID_ARG;
    c->locals.samples_per_frame = spp;
    c->width.invalidate();
    return MRT_OK;
}

uint32_t mrt_frames_done(mrt_ctx* c) { return c ? c->frames_done : 0; }

void* mrt_framebuffer_device_ptr(mrt_ctx* c) {
    if (!c) return nullptr;
    return c->d_fb[c->target ^ 1];   // after the swap, the last render target is "secondary"
}

int mrt_read_framebuffer(mrt_ctx* c, float* out, size_t cap) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    return mrt::read_rows(c, __func__, c->d_fb[c->target ^ 1], out, cap, 16);
}

int mrt_read_counters(mrt_ctx* c, mrt_counters* out) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    unsigned long long h[5];
    HIP_TRY(c, hipMemcpyAsync(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost, c->stream));
    MRT_TRY(mrt::wait_stream(c, c->stream, __func__));
    out->samples = h[0]; out->world_hit_calls = h[1]; out->rng_draws = h[2]; out->lane_slots = h[3];
    out->member_tests = h[4];
    out->sweep_records = c->n_padded;
    return MRT_OK;
}

// diagnostic: all 16 raw counter slots (slots 4.. are only written by -DMRT_STAMPS builds)
int mrt_debug_read_counters(mrt_ctx* c, uint64_t out[16]) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, c->d_counters, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    MRT_TRY(mrt::wait_stream(c, c->stream, __func__));
    return MRT_OK;
}

// diagnostic: enable / read the per-wave log {t_start, t_end (100 MHz ticks), trips, bounces}
// that -DMRT_STAMPS builds write; out == NULL just (re)allocates it for the current shard.  The log is a ring over the last
// kWaveLogFrames frames (frames in flight overlap): `back` = 0 reads the most recent frame's, 1 the one before, ...
int mrt_debug_wave_log_frame(mrt_ctx* c, uint32_t back, uint64_t* out, size_t cap_waves, size_t* n_waves) {
    if (!c || back >= mrt_ctx::kWaveLogFrames) return MRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = c->n_waves;
    if (n_waves) *n_waves = n;
    if (!c->d_wave_log || c->wave_log_waves != n) {
        MRT_TRY(mrt::wait_all(c, __func__));
        free_device(c->d_wave_log);
        HIP_TRY(c, hipMalloc(&c->d_wave_log, mrt_ctx::kWaveLogFrames * n * 4 * sizeof(uint64_t)));
        // (on the ctx's stream and waited for: the side streams do not order themselves behind the null stream)
        HIP_TRY(c, hipMemsetAsync(c->d_wave_log, 0, mrt_ctx::kWaveLogFrames * n * 4 * sizeof(uint64_t), c->stream));
        MRT_TRY(mrt::wait_stream(c, c->stream, __func__));
        c->wave_log_waves = n;
    }
    if (out) {
        if (cap_waves < n) return fail(c, MRT_ERR_TOO_SMALL, "mrt_debug_wave_log: need %zu waves", n);
        if (c->frame_seq <= back) return fail(c, MRT_ERR_STATE, "mrt_debug_wave_log: frame %u back has not been rendered", back);
        MRT_TRY(mrt::wait_all(c, __func__));
        const unsigned long long* src = c->d_wave_log + (size_t)((c->frame_seq - 1 - back) % mrt_ctx::kWaveLogFrames) * n * 4;
        HIP_TRY(c, hipMemcpyAsync(out, src, n * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        MRT_TRY(mrt::wait_stream(c, c->stream, __func__));
    }
    return MRT_OK;
}
int mrt_debug_wave_log(mrt_ctx* c, uint64_t* out, size_t cap_waves, size_t* n_waves) {
    return mrt_debug_wave_log_frame(c, 0, out, cap_waves, n_waves);
}

int mrt_kernel_ms_history(mrt_ctx* c, float* ms, size_t cap, size_t* n_out) {
    if (!c || !ms || !n_out) return MRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    size_t n = c->frame_seq < mrt_ctx::kEventRing ? (size_t)c->frame_seq : mrt_ctx::kEventRing;
    if (n > cap) n = cap;
    for (size_t i = 0; i < n; i++) {          // ms[0] = oldest of the n most recent redraws
        const uint32_t slot = (uint32_t)((c->frame_seq - n + i) % mrt_ctx::kEventRing);
        MRT_TRY(mrt::wait_event(c, c->ev_stop[slot], "mrt_kernel_ms_history: the render kernel's stop event"));
        HIP_TRY(c, hipEventElapsedTime(&ms[i], c->ev_start[slot], c->ev_stop[slot]));
    }
    *n_out = n;
    return MRT_OK;
}

// Host only: would a call this context ACCEPTS touch something that is not there?  Walks what the next frame, query, present,
// denoise or gather reads and writes; a part the context knows it lacks and refuses the calls for (no scene: MRT_ERR_NO_SCENE)
// is sound.  0 = sound; else 1 and the first finding in `why`.
int mrt_debug_check_context(mrt_ctx* c, char* why, size_t cap) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (why && cap) why[0] = 0;
    if (!c->stream || !c->own_stream) return check_finding(why, cap, "the context has no stream");
    if (!c->ev_inputs) return check_finding(why, cap, "ev_inputs is missing");
    for (uint32_t i = 0; i < mrt_ctx::kEventRing; i++)
        if (!c->ev_start[i] || !c->ev_stop[i]) return check_finding(why, cap, "timing event pair %u is missing", i);
    if (!c->d_counters || !c->h_stats) return check_finding(why, cap, "the counters or their pinned copy are missing");
    if (c->shard_world == 0 || c->shard_rank >= c->shard_world) return check_finding(why, cap, "shard %u of %u", c->shard_rank, c->shard_world);
    if (c->local_bands != (total_bands(c->args.height) + c->shard_world - 1) / c->shard_world || c->tiles_x != (c->args.width + mrt::kTileW - 1) / mrt::kTileW ||
        c->n_tiles != c->tiles_x * c->local_bands)
        return check_finding(why, cap, "local_bands %u / tiles %u x %u do not belong to shard %u of %u", c->local_bands, c->tiles_x, c->n_tiles, c->shard_rank, c->shard_world);
    if (local_texels(c) > 0 && (!c->d_fb[0] || !c->d_fb[1] || !c->d_seeds)) return check_finding(why, cap, "a framebuffer or the seeds are missing (%zu local texels)", local_texels(c));
    if (c->target != 0 && c->target != 1) return check_finding(why, cap, "target %d", c->target);
    if (c->n_waves == 0 || c->cus == 0) return check_finding(why, cap, "n_waves %u, cus %u", c->n_waves, c->cus);
    if (c->frame_slots < 1 || c->frame_slots > mrt_ctx::kMaxFrameSlots) return check_finding(why, cap, "frame_slots %u", c->frame_slots);
    if (c->last_slot >= mrt_ctx::kMaxFrameSlots) return check_finding(why, cap, "last_slot %u", c->last_slot);
    for (uint32_t i = 0; i < mrt_ctx::kMaxFrameSlots; i++) {
        const mrt_ctx::FrameSlot& S = c->slot[i];
        if ((S.pix_acc_layers == 0) != (S.d_pix_acc == nullptr)) return check_finding(why, cap, "slot %u: %zu layers of colour sums at %p", i, S.pix_acc_layers, S.d_pix_acc);
        if (S.d_pix_acc && (size_t)S.cost_first_layer + S.cost_layers > S.pix_acc_layers)
            return check_finding(why, cap, "slot %u: cost layers %u + %u of %zu", i, S.cost_first_layer, S.cost_layers, S.pix_acc_layers);
        if ((S.stats_pending || S.render_pending) && (!S.stream || !S.stats_ready || !S.render_done)) return check_finding(why, cap, "slot %u: a frame is pending without its stream or events", i);
        if (i >= c->frame_slots && i != c->last_slot) continue;
        if (!S.stream) return check_finding(why, cap, "slot %u of %u in use has no stream (its frames would run on the null stream)", i, c->frame_slots);
        if (!S.render_done || !S.finalize_done || !S.stats_ready) return check_finding(why, cap, "slot %u of %u in use lacks an event", i, c->frame_slots);
        if (!S.d_tile_cost || !S.d_tile_order || !S.d_sort_scratch) return check_finding(why, cap, "slot %u of %u in use lacks its tile cost / order / scratch buffers", i, c->frame_slots);
        if (S.pix_acc_layers < 1) return check_finding(why, cap, "slot %u of %u in use has no colour sums", i, c->frame_slots);
    }
    if (c->have_world) {
        if (!c->d_spheres || !c->d_clusters || !c->d_nodes || !c->d_top_mfma || !c->d_member_index || !c->d_regroup || !c->d_prev_xyzr || !c->d_shade || !c->d_vec4 || !c->d_f32 || !c->d_i32)
            return check_finding(why, cap, "have_world without one of the scene's arrays");
        if (c->regroup_words != (c->n_pool > 1 ? mrt::regroup_layout(c->n_pool, c->n_pooled).words : 0))
            return check_finding(why, cap, "a regroup scratch of %zu words for %u pool clusters of %u spheres (the policy's state is its tail)", c->regroup_words, c->n_pool, c->n_pooled);
        if (!mrt::scene_is_small(c->n_members) && (!c->d_boxes || !c->d_boxes_open)) return check_finding(why, cap, "a large scene (%u members) without its boxes", c->n_members);
        if (mrt::scene_is_small(c->n_members) && c->n_padded <= mrt::kCamMaskRecords && (!c->d_cam_masks || c->cam_mask_entries == 0))
            return check_finding(why, cap, "a small scene of %u top records without its camera masks", c->n_padded);
    }
    if ((c->d_cam_masks == nullptr) != (c->cam_mask_entries == 0)) return check_finding(why, cap, "camera masks %p of %zu entries", (void*)c->d_cam_masks, c->cam_mask_entries);
    if (c->cam_mask_built > c->cam_mask_gen || (c->cam_mask_built != 0 && !c->d_cam_masks)) return check_finding(why, cap, "camera masks built for generation %llu of %llu without a table", (unsigned long long)c->cam_mask_built, (unsigned long long)c->cam_mask_gen);
    if (c->cam_masks_in_force && (!c->d_cam_masks || !c->have_world)) return check_finding(why, cap, "camera masks in force without a table or a scene");
    if (c->noise_on) {
        if (!c->d_noise_s || !c->d_noise_tiles || !c->d_noise_partials) return check_finding(why, cap, "noise tracking is on without S, the tile maps or the scratch");
        if (!c->d_noise_sums || !c->h_noise_sums) return check_finding(why, cap, "noise tracking is on without the ring's sums");
        for (uint32_t i = 0; i < mrt_ctx::kNoiseRing; i++)
            if (!c->noise_ring[i].copied) return check_finding(why, cap, "noise ring entry %u has no event", i);
    } else if (c->d_noise_s) {
        return check_finding(why, cap, "S exists while noise tracking is off (the blends would track)");
    }
    if (c->present_depth > c->present_ring.size()) return check_finding(why, cap, "present depth %u of %zu entries", c->present_depth, c->present_ring.size());
    for (size_t i = 0; i < c->present_ring.size(); i++) {
        const mrt_ctx::PresentEntry& E = c->present_ring[i];
        if (!E.d_img || !E.h_img || !E.copied) return check_finding(why, cap, "present ring entry %zu lacks its device image, pinned image or event", i);
    }
    if (!c->present_ring.empty() && (c->present_entry_bytes == 0 || !c->d_present_tables)) return check_finding(why, cap, "a present ring without entry size or tables");
    if (!c->guides_stale && (!c->d_guides || !c->d_guide_rays || !c->d_guide_hits || !c->d_guide_queue || !c->d_guide_cand || !c->den.have_filter()))
        return check_finding(why, cap, "the guides are marked current without the denoiser's buffers");
    if (c->gather_has_s && (!c->d_gather || c->gather_bytes < mrt::gathered_colour_bytes(c) + mrt::gathered_colour_bytes(c) / 4))
        return check_finding(why, cap, "a gathered S is marked readable in a gathered frame of %zu bytes (%zu of colour)", c->gather_bytes, mrt::gathered_colour_bytes(c));
    if (c->temporal_on && c->shard_world != 1) return check_finding(why, cap, "temporal reprojection is on on shard %u of %u", c->shard_rank, c->shard_world);
    if (c->temporal_cur > 1) return check_finding(why, cap, "temporal history pair %u", c->temporal_cur);
    if (c->temporal_stepped && (!c->temporal_on || c->temporal_clear || !c->have_world || !c->d_guides || !c->den.have_filter() || !c->den.all_history(false)))
        return check_finding(why, cap, "a temporal history is marked readable without temporal reprojection, a scene, the guides or its buffers");
    if (!c->temporal_on && c->den.any_history(false)) return check_finding(why, cap, "history buffers exist while temporal reprojection is off");
    if (c->temporal_stepped && c->temporal_response.enabled && !c->den.all_history(true))
        return check_finding(why, cap, "a temporal history with the response on is marked readable without the fast history's buffers");
    if (!c->temporal_on && c->den.any_history(true)) return check_finding(why, cap, "fast history buffers exist while temporal reprojection is off");
    if (c->temporal_response.enabled > 1 || c->temporal_response.size != sizeof(mrt_temporal_response))
        return check_finding(why, cap, "temporal response enabled %u, size %u", c->temporal_response.enabled, c->temporal_response.size);
    if (c->auto_regroup.enabled > 1 || c->auto_regroup.size != sizeof(mrt_auto_regroup) || c->auto_regroup.check_every < 1 || c->auto_regroup.check_every > 1024)
        return check_finding(why, cap, "auto regroup enabled %u, size %u, check_every %u", c->auto_regroup.enabled, c->auto_regroup.size, c->auto_regroup.check_every);
    if (c->denoise_mix.enabled > 1 || c->denoise_mix.size != sizeof(mrt_denoise_mix) || !(c->denoise_mix.gain >= 0.25f && c->denoise_mix.gain <= 16.0f))
        return check_finding(why, cap, "denoise mix enabled %u, size %u, gain %g", c->denoise_mix.enabled, c->denoise_mix.size, c->denoise_mix.gain);
    if (c->d_guide_cand == nullptr ? c->guide_cand_words != 0 : c->guide_cand_words == 0) return check_finding(why, cap, "guide bitmap %p of %zu words", (void*)c->d_guide_cand, c->guide_cand_words);
    if (c->tiles_diverged) {
        if (c->n_tiles && !c->d_tile_frames) return check_finding(why, cap, "the accumulation has diverged without the tile frame counts");
        if (c->tile_frames.size() != c->n_tiles) return check_finding(why, cap, "%zu host tile frame counts for %u tiles", c->tile_frames.size(), c->n_tiles);
    }
    if (c->k_len != 0 && (!c->d_k_f32 || !c->d_k_f64 || c->k_table.size() < c->k_len)) return check_finding(why, cap, "a K table of %u entries without its buffers", c->k_len);
    if (c->d_wave_log && c->wave_log_waves == 0) return check_finding(why, cap, "a wave log of no waves");
    return 0;
}

int mrt_last_kernel_ms(mrt_ctx* c, float* ms) {
    if (!c || !ms) return MRT_ERR_INVALID_ARG;
    if (!c->frame_seq) return fail(c, MRT_ERR_STATE, "mrt_last_kernel_ms: nothing rendered yet");
    size_t n = 0;
    return mrt_kernel_ms_history(c, ms, 1, &n);
}

}  // extern "C"
