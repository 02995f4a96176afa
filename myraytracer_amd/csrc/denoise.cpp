// The denoiser and the temporal reprojection of include/myraytracer_amd.h: the first-hit guides, the filter (denoise.hip), the
// history's step and image (temporal.hip), the diagnostic views (views.hip), which write the filter's output buffer, and what
// mrt_present and the float read-backs share of them (ImageSource, mrt_ctx.h).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "mrt_ctx.h"

using mrt::fail, mrt::fill_scene_params, mrt::ImageSource;

// ---- denoiser (include/myraytracer_amd.h, "denoiser") ----------------------------------------------------------------------
// queue_denoise queues, on the ctx's stream right behind the most recent frame's blend, the guide rebuild when the guides are
// stale (denoise.hip: the centre rays; render_kernel's DBG instantiation: their closest hits; the guide records) and the filter's
// iterations into den.out(); nothing here waits on the host.  Ordering: every reader of den.out() (the present kernel, the
// read-back copy) is queued behind it on the same stream, and the next denoise is queued behind those readers.
namespace {

bool denoise_params_ok(const mrt_denoise_params* p) {
    if (p->size != sizeof(mrt_denoise_params) || p->iterations < 1 || p->iterations > 8 || p->normal_exp > 16) return false;
    for (float v : {p->sigma_l, p->sigma_z, p->sigma_a})
        if (!(std::isfinite(v) && v > 0.0f)) return false;
    for (uint32_t r : p->reserved)
        if (r != 0) return false;
    return true;
}

bool denoise_mix_ok(const mrt_denoise_mix* p) {
    if (p->size != sizeof(mrt_denoise_mix) || p->enabled > 1) return false;
    if (!(std::isfinite(p->gain) && p->gain >= 0.25f && p->gain <= 16.0f)) return false;
    for (uint32_t r : p->reserved)
        if (r != 0) return false;
    return true;
}

int ensure_denoise_buffers(mrt_ctx* c) {
    const size_t n = (size_t)c->args.width * c->args.height;
    // the filter's three buffers; with temporal reprojection on -- and only then -- the history's four behind them, and with its
    // response on as well the fast history's two behind those
    const size_t n_den = mrt::DenoiseBuffers::wanted(c->temporal_on, c->temporal_response.enabled != 0);
    if (!c->d_guides || !c->den.have_filter() || (c->temporal_on && !c->den.have_history(c->temporal_response.enabled != 0))) {  // (each of them unless it is there already, an earlier, refused attempt's included)
        if (!c->d_guide_rays) HIP_TRY(c, hipMalloc((void**)&c->d_guide_rays, n * 6 * sizeof(float)));
        if (!c->d_guide_hits) HIP_TRY(c, hipMalloc((void**)&c->d_guide_hits, n * 2 * sizeof(int32_t)));
        if (!c->d_guide_queue) HIP_TRY(c, hipMalloc((void**)&c->d_guide_queue, 64));
        for (auto& d : c->den.buf) {
            if (&d == c->den.buf + n_den) break;
            if (!d) HIP_TRY(c, hipMalloc((void**)&d, n * 16));
        }
        if (!c->d_guides) {
            HIP_TRY(c, hipMalloc((void**)&c->d_guides, n * 32));
            c->guides_stale = true;
        }
    }
    const size_t words = n + ((size_t)c->n_spheres + 31) / 32 + 1;
    if (c->guide_cand_words < words) {
        if (c->d_guide_cand) {          // (a larger scene than before: the old bitmap may still be written by a queued rebuild)
            MRT_TRY(mrt::wait_stream(c, c->stream, "denoiser: regrowing the guide pass' bitmap"));
            mrt::free_device(c->d_guide_cand);
            c->guide_cand_words = 0;
        }
        HIP_TRY(c, hipMalloc((void**)&c->d_guide_cand, words * sizeof(uint32_t)));
        c->guide_cand_words = words;
    }
    return MRT_OK;
}

// The guides of the current camera and scene, queued on the ctx's stream: always over the FULL image.  On a shard (the root of
// a gather, mrt_read_gathered_denoised) the ctx's own tile count and seed texture are its bands' alone, so the pass gets the full
// image's tile count and, for the seed texel the kernel loads for every pixel it acquires (and, in this instantiation, never
// uses), the filter's ping buffer: width x height 16-byte texels, idle here -- the filter that writes it is queued behind this
// pass on the same stream, and the previous one before it.
int rebuild_guides(mrt_ctx* c) {
    const uint32_t W = c->args.width, H = c->args.height;
    int e = mrt::launch_guide_rays(c->d_guide_rays, W, H, c->cam_raw, c->stream);
    if (e) return fail(c, MRT_ERR_HIP, "guide rays launch failed: %s", hipGetErrorString((hipError_t)e));
    // mrt_debug_world_hit's launch over the image itself: pixel (x, y) is ray y * W + x (world 1, texel order)
    mrt::KParams p;
    std::memset(&p, 0, sizeof p);
    p.locals = c->locals;
    p.locals.shape[0] = W; p.locals.shape[1] = H;
    p.locals.samples_per_frame = 1; p.locals.ray_depth = 1;
    fill_scene_params(c, p);
    p.shard_rank = 0; p.shard_world = 1;
    const bool shard = c->shard_world != 1;
    p.seeds = shard ? reinterpret_cast<const uint32_t*>(c->den.ping()) : c->d_seeds;
    p.tiles_x = c->tiles_x; p.n_tiles = shard ? c->tiles_x * mrt::total_bands(H) : c->n_tiles;
    p.tile_queue = c->d_guide_queue;
    p.n_blocks = 1; p.pix_stride = 0; p.queue_layers = 1; p.lane_frames = 1;
    p.dbg_rays = c->d_guide_rays; p.dbg_hit = c->d_guide_hits;
    p.dbg_cand = c->d_guide_cand; p.dbg_words = 1;
    e = mrt::launch_debug_world_hit(p, c->n_waves, c->stream);
    if (e) return fail(c, MRT_ERR_HIP, "guide hits launch failed: %s", hipGetErrorString((hipError_t)e));
    e = mrt::launch_guide_fill(c->d_guide_rays, c->d_guide_hits, c->d_shade, c->d_i32 + c->world.spheres.material_ty_base_idx,
                               c->d_guides, W, H, c->stream);
    if (e) return fail(c, MRT_ERR_HIP, "guide fill launch failed: %s", hipGetErrorString((hipError_t)e));
    c->guides_stale = false;
    return MRT_OK;
}

// the refusals of every denoise on a ctx; `tracking`: the filter's (the guides alone do not need noise tracking)
int denoise_check(mrt_ctx* c, const char* who, bool tracking) {
    if (tracking && !c->noise_on) return fail(c, MRT_ERR_STATE, "%s: noise tracking is off (mrt_set_noise_tracking)", who);
    if (c->shard_world != 1) return fail(c, MRT_ERR_STATE, "%s: a shard (world %u) cannot be denoised", who, c->shard_world);
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "%s: no scene", who);
    if ((size_t)c->args.width * c->args.height == 0) return fail(c, MRT_ERR_STATE, "%s: empty image", who);
    if (c->tiles_diverged && !c->denoise_adaptive)      // (K differs per tile: the per-tile filter is opt-in, mrt_set_denoise_adaptive)
        return fail(c, MRT_ERR_STATE, "%s: the accumulation is adaptive (mrt_render_tiles since the last reset)", who);
    return MRT_OK;
}

int ensure_guides(mrt_ctx* c) {
    MRT_TRY(ensure_denoise_buffers(c));
    if (c->guides_stale) MRT_TRY(rebuild_guides(c));
    return MRT_OK;
}

// launch_denoise's variance of a frame count in a mode: SPATIAL_EARLY is the spatial estimate while the history is short and
// PREFILTERED from then on
mrt::UniformVariance variance_of(uint32_t mode, uint32_t frames_done, uint32_t spatial_frames) {
    using V = mrt::UniformVariance;
    if (mode == MRT_DENOISE_VAR_SPATIAL_EARLY) return frames_done < spatial_frames ? V::Spatial : V::Prefiltered;
    return mode == MRT_DENOISE_VAR_PREFILTERED ? V::Prefiltered : V::Accumulated;
}

// what every denoise of the context shares: frame `fb` through the context's guides, scratch and parameters into den.out()
mrt::DenoiseJob denoise_job(const mrt_ctx* c, const float* fb, mrt::DenoiseSource source) {
    mrt::DenoiseJob j{};
    j.fb = fb;
    j.guides = c->d_guides;
    j.ping = c->den.ping(); j.pong = c->den.pong(); j.out = c->den.out();
    j.width = c->args.width; j.height = c->args.height;
    j.prm = c->denoise;
    j.source = source;
    j.mix = c->denoise_mix;         // (launch_denoise reads it for an accumulation alone)
    return j;
}

// The refusals of the gathered frame's guides and denoise: denoise_check's for a frame that lives on a shard's root (`tracking`:
// the filter's -- a gathered S; the guides alone need none).
int gathered_denoise_check(mrt_ctx* c, const char* who, bool tracking) {
    if (tracking) MRT_TRY(mrt::gathered_noise_check(c, who));
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "%s: no scene", who);
    if ((size_t)c->args.width * c->args.height == 0) return fail(c, MRT_ERR_STATE, "%s: empty image", who);
    return MRT_OK;
}

// The most recent frame denoised into den.out() (after denoise_check): with one K, or -- an adaptive accumulation -- K per tile.
// `gathered`: the latest gathered frame, with the gather's snapshot of K and the frame count (after gathered_denoise_check).
int queue_denoise(mrt_ctx* c, bool gathered) {
    const bool per_tile = !gathered && c->denoise_adaptive && c->tiles_diverged;
    // K per tile: the device table covers every count of the host's map, which is the device's at this point of the stream
    if (per_tile) MRT_TRY(mrt::ensure_k_table(c, mrt::most_tile_frames(c) + 1u));
    MRT_TRY(ensure_guides(c));
    mrt::DenoiseJob job = denoise_job(c, gathered ? c->d_gather : c->d_fb[c->target ^ 1], per_tile ? mrt::DenoiseSource::Tiles : mrt::DenoiseSource::Uniform);
    job.S = gathered ? mrt::gathered_noise(c) : c->d_noise_s;
    if (per_tile) job.tiles = {c->d_tile_frames, c->d_k_f32, c->tiles_x, c->denoise_var_mode, c->denoise_spatial_frames};
    else job.uniform = {(float)(gathered ? c->gather_k : mrt::noise_factor_of(c->noise_c2)),
                        variance_of(c->denoise_var_mode, gathered ? c->gather_frames : c->frames_done, c->denoise_spatial_frames)};
    const int e = mrt::launch_denoise(job, c->stream);
    if (e) return fail(c, MRT_ERR_HIP, "%sdenoise launch failed: %s", per_tile ? "per-tile " : "", hipGetErrorString((hipError_t)e));
    return MRT_OK;
}

// ---- diagnostic views (include/myraytracer_amd.h, "diagnostic views") ------------------------------------------------------
bool view_ok(const mrt_view* v) {
    if (v->size != sizeof(mrt_view) || v->kind < MRT_VIEW_NOISE_SE || v->kind > MRT_VIEW_SPHERE || v->ramp > MRT_VIEW_RAMP_HEAT) return false;
    if (!std::isfinite(v->lo) || !std::isfinite(v->hi) || v->hi == v->lo || !std::isfinite(1.0f / (v->hi - v->lo))) return false;
    if (!(std::isfinite(v->rel_floor) && v->rel_floor >= 0.0f)) return false;
    for (uint32_t r : v->reserved)
        if (r != 0) return false;
    return true;
}

bool view_reads_noise(const mrt_view& v) { return v.kind == MRT_VIEW_NOISE_SE || v.kind == MRT_VIEW_NOISE_REL; }

// the refusals of a view, in the header's order
int view_check(mrt_ctx* c, const char* who) {
    if (c->shard_world != 1) return fail(c, MRT_ERR_STATE, "%s: a shard (world %u) has no views (a view is image-sized, the guides unsharded)", who, c->shard_world);
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "%s: no scene", who);
    if ((size_t)c->args.width * c->args.height == 0) return fail(c, MRT_ERR_STATE, "%s: empty image", who);
    if (view_reads_noise(c->view) && !c->noise_on) return fail(c, MRT_ERR_STATE, "%s: a noise view with noise tracking off (mrt_set_noise_tracking)", who);
    return MRT_OK;
}

// The current view of the most recent frame into den.out() (after view_check), queued on the ctx's stream: a writer of den.out()
// like the filter, behind the earlier readers and ahead of its own.  The noise kinds and TILE_FRAMES of a diverged accumulation
// read the device's tile map, which is the host's at this point of the stream, and K per tile as queue_denoise does; a uniform
// one reads neither (the map may not exist).  The guide kinds rebuild stale guides first.
int queue_view(mrt_ctx* c) {
    const mrt_view& v = c->view;
    const bool noise = view_reads_noise(v), guides = v.kind >= MRT_VIEW_DEPTH;
    const bool per_tile = (noise || v.kind == MRT_VIEW_TILE_FRAMES) && c->tiles_diverged;
    if (per_tile && noise) MRT_TRY(mrt::ensure_k_table(c, mrt::most_tile_frames(c) + 1u));
    if (guides) MRT_TRY(ensure_guides(c));
    else MRT_TRY(ensure_denoise_buffers(c));
    mrt::ViewArgs a{};
    a.fb = c->d_fb[c->target ^ 1]; a.S = c->d_noise_s; a.guides = c->d_guides;
    if (per_tile) { a.tile_frames = c->d_tile_frames; a.Kf = c->d_k_f32; }
    a.out = c->den.out();
    a.width = c->args.width; a.height = c->args.height; a.tiles_x = c->tiles_x;
    a.kind = v.kind; a.ramp = v.ramp;
    a.K = (float)mrt::noise_factor_of(c->noise_c2); a.frames = (float)c->frames_done;
    a.lo = v.lo; a.inv = 1.0f / (v.hi - v.lo); a.rel_floor = v.rel_floor;
    const int e = mrt::launch_view(a, c->stream);
    if (e) return fail(c, MRT_ERR_HIP, "view launch failed: %s", hipGetErrorString((hipError_t)e));
    return MRT_OK;
}

// the guides (rebuilt first if stale) read back and split into their fields, after the caller's checks
int read_guides(mrt_ctx* c, const char* who, float* rays, int32_t* index, float* t, float* normal, float* albedo, size_t cap) {
    const size_t n = (size_t)c->args.width * c->args.height;
    if (cap < n) return fail(c, MRT_ERR_TOO_SMALL, "%s: need %zu pixels", who, n);
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(ensure_guides(c));
    std::vector<float> g(n * 8);
    if (rays) HIP_TRY(c, hipMemcpyAsync(rays, c->d_guide_rays, n * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(g.data(), c->d_guides, n * 32, hipMemcpyDeviceToHost, c->stream));
    MRT_TRY(mrt::wait_stream(c, c->stream, who));
    for (size_t i = 0; i < n; i++) {
        const float* r = g.data() + 8 * i;
        if (index) std::memcpy(index + i, r + 7, 4);
        if (t) t[i] = r[3];
        if (normal) std::memcpy(normal + 3 * i, r, 12);
        if (albedo) std::memcpy(albedo + 3 * i, r + 4, 12);
    }
    return MRT_OK;
}

// ---- temporal reprojection (include/myraytracer_amd.h, "temporal reprojection") ----------------------------------------------
bool temporal_params_ok(const mrt_temporal_params* p) {
    if (p->size != sizeof(mrt_temporal_params) || p->max_history < 1 || p->max_history > 256 || p->spatial_len < 1 || p->spatial_len > 16)
        return false;
    if (!(std::isfinite(p->depth_tol) && p->depth_tol > 0.0f)) return false;
    for (uint32_t r : p->reserved)
        if (r != 0) return false;
    return true;
}

// the refusals of a step, a read and a present of the temporal image; `stepped`: the reads' (they need a history)
int temporal_check(mrt_ctx* c, const char* who, bool stepped) {
    if (!c->temporal_on) return fail(c, MRT_ERR_STATE, "%s: temporal reprojection is off (mrt_set_temporal)", who);
    if (c->shard_world != 1) return fail(c, MRT_ERR_STATE, "%s: a shard (world %u) has no temporal history", who, c->shard_world);
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "%s: no scene", who);
    if ((size_t)c->args.width * c->args.height == 0) return fail(c, MRT_ERR_STATE, "%s: empty image", who);
    if (stepped && !c->temporal_stepped) return fail(c, MRT_ERR_STATE, "%s: no mrt_temporal_step since the history was last empty", who);
    return MRT_OK;
}

// The inverse of the matrix with the columns su, sv, -fw of a derived camera (mode 0: x, y, -z) by cofactors, in double, rounded
// to float, row-major; and the camera's origin.
void temporal_camera(const mrt_camera_raw& cam, float M[9], float o[3]) {
    double A[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, -1.0}};
    for (int k = 0; k < 3; k++) {
        o[k] = cam.mode != 0 ? cam.origin[k] : 0.0f;
        if (cam.mode != 0) { A[k][0] = (double)cam.su[k]; A[k][1] = (double)cam.sv[k]; A[k][2] = -(double)cam.fw[k]; }
    }
    double C[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            C[i][j] = A[i1][j1] * A[i2][j2] - A[i1][j2] * A[i2][j1];
        }
    const double det = (A[0][0] * C[0][0] + A[0][1] * C[0][1]) + A[0][2] * C[0][2];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[3 * i + j] = (float)(C[j][i] / det);
}

bool temporal_response_ok(const mrt_temporal_response* p) {
    if (p->size != sizeof(mrt_temporal_response) || p->enabled > 1 || p->fast_history < 1 || p->fast_history > 16) return false;
    if (!(std::isfinite(p->clamp_sigma) && p->clamp_sigma > 0.0f) || !(p->antilag >= 0.0f && p->antilag <= 1.0f)) return false;
    for (uint32_t r : p->reserved)
        if (r != 0) return false;
    return true;
}

// A dropped history, made what the next step reads: every length 0 (no tap counts), the fast history zeroed with it, "previous"
// camera the current one.  Queued on the ctx's stream.  (h0, cam false: mrt_debug_load_temporal brings that part itself.)
int clear_history(mrt_ctx* c, bool h0 = true, bool cam = true) {
    const size_t n = (size_t)c->args.width * c->args.height;
    const uint32_t cur = c->temporal_cur;
    if (h0) HIP_TRY(c, hipMemsetAsync(c->den.h0(cur), 0, n * 16, c->stream));
    if (c->temporal_response.enabled && c->den.h2(cur)) HIP_TRY(c, hipMemsetAsync(c->den.h2(cur), 0, n * 16, c->stream));
    if (cam) c->temporal_prev_cam = c->cam_raw;
    c->temporal_clear = false;
    return MRT_OK;
}

// What the four debug reads and loads of the history (`who`) open with: a step's refusals, the response's, the buffers'.  The rest
// stays with each: the capacity refusals (before hipSetDevice) differ -- one counts spheres too, the loads have none -- as does the clearing
int history_io_opening(mrt_ctx* c, const char* who, bool needs_response) {
    MRT_TRY(temporal_check(c, who, false));
    if (needs_response && !c->temporal_response.enabled) return fail(c, MRT_ERR_STATE, "%s: the response is off (mrt_set_temporal_response)", who);
    if (!c->den.have_history(c->temporal_response.enabled != 0)) return fail(c, MRT_ERR_STATE, "%s: no history buffers yet (mrt_temporal_step)", who);
    return MRT_OK;
}

// the temporal image into den.out(): the history's field (its variance made first), then the filter's iterations
int queue_temporal_image(mrt_ctx* c) {
    const uint32_t cur = c->temporal_cur;
    mrt::DenoiseJob job = denoise_job(c, c->d_fb[c->target ^ 1], mrt::DenoiseSource::Temporal);
    job.temporal = {c->den.h0(cur), c->den.h1(cur), c->temporal.spatial_len};
    const int e = mrt::launch_denoise(job, c->stream);
    if (e) return fail(c, MRT_ERR_HIP, "temporal image launch failed: %s", hipGetErrorString((hipError_t)e));
    return MRT_OK;
}

// mrt_debug_denoise_variance and mrt_debug_denoise_mix: a uniform accumulation given by the caller, filtered in buffers of its
// own; `mix` NULL: no blend.  With a blend on, K is read in every variance (v = S * K), the spatial one included.
int debug_denoise(mrt_ctx* c, const float* rgba, const float* S, double K, const float* guides, uint32_t width, uint32_t rows,
                  const mrt_denoise_params* params, uint32_t variance, const mrt_denoise_mix* mix, float* out) {
    if (!c || !rgba || !S || !guides || !out || !width || !rows || (uint64_t)width * rows > (1ull << 26) || variance > 2)
        return MRT_ERR_INVALID_ARG;
    if (variance == 2 && !(mix && mix->enabled)) K = 0.0;       // (the spatial initial variance: K is not read)
    if (std::isnan(K) || K < 0.0) return MRT_ERR_INVALID_ARG;
    const mrt_denoise_params prm = params ? *params : c->denoise;
    if (!denoise_params_ok(&prm)) return fail(c, MRT_ERR_INVALID_ARG, "mrt_debug_denoise: bad parameters");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)width * rows;
    float *d_fb = nullptr, *d_s = nullptr, *d_g = nullptr, *d_b[3] = {nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    const char* what = "mrt_debug_denoise";
    HIP_CHAIN(e, what, hipMalloc((void**)&d_fb, n * 16));
    HIP_CHAIN(e, what, hipMalloc((void**)&d_s, n * sizeof(float)));
    HIP_CHAIN(e, what, hipMalloc((void**)&d_g, n * 32));
    for (auto& b : d_b) HIP_CHAIN(e, what, hipMalloc((void**)&b, n * 16));
    if (e == hipSuccess) e = hipMemcpyAsync(d_fb, rgba, n * 16, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_s, S, n * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_g, guides, n * 32, hipMemcpyHostToDevice, c->stream);
    mrt::DenoiseJob job{};
    job.fb = d_fb; job.S = d_s; job.guides = d_g;
    job.ping = d_b[0]; job.pong = d_b[1]; job.out = d_b[2];
    job.width = width; job.height = rows;
    job.prm = prm;
    job.source = mrt::DenoiseSource::Uniform;
    job.uniform = {(float)K, (mrt::UniformVariance)variance};
    if (mix) job.mix = *mix;
    if (e == hipSuccess) e = (hipError_t)mrt::launch_denoise(job, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_b[2], n * 16, hipMemcpyDeviceToHost, c->stream);
    int ws = MRT_OK;
    if (e == hipSuccess) ws = mrt::wait_stream(c, c->stream, "mrt_debug_denoise");
    if (ws != MRT_OK) return ws;            // (stalled: the buffers are left to the process)
    mrt::free_device(d_fb, d_s, d_g, d_b[0], d_b[1], d_b[2]);
    if (e != hipSuccess) return fail(c, MRT_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    return MRT_OK;
}

// mrt_read_denoised, mrt_read_temporal and mrt_read_gathered_denoised (`who`): a source's image, queued and read back
int read_source(mrt_ctx* c, ImageSource source, const char* who, float* out, size_t cap) {
    MRT_TRY(mrt::source_check(c, source, who));
    const size_t n = (size_t)c->args.width * c->args.height * 4;
    if (cap < n) return fail(c, MRT_ERR_TOO_SMALL, "%s: need %zu floats", who, n);
    HIP_TRY(c, hipSetDevice(c->device));
    mrt::SourceImage S;
    MRT_TRY(mrt::source_queue(c, source, &S));
    HIP_TRY(c, hipMemcpyAsync(out, S.img, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return mrt::wait_stream(c, c->stream, who);
}

}  // namespace

namespace mrt {

// the denoiser's guides and buffers (sized for the image; allocated at the first denoise, ensure_denoise_buffers)
void free_denoise_buffers(mrt_ctx* c) {
    free_device(c->d_guide_rays, c->d_guide_hits, c->d_guide_cand, c->d_guide_queue, c->d_guides);
    c->den.free_all();
    c->guide_cand_words = 0;
    c->guides_stale = true;
    drop_temporal_history(c);
}

void drop_temporal_history(mrt_ctx* c) {
    c->temporal_clear = true;
    c->temporal_stepped = false;
}

int source_check(mrt_ctx* c, ImageSource source, const char* who) {
    switch (source) {
        case ImageSource::Denoised: return denoise_check(c, who, true);
        case ImageSource::Temporal: return temporal_check(c, who, true);
        case ImageSource::GatheredDenoised: return gathered_denoise_check(c, who, true);
        case ImageSource::View: return view_check(c, who);
        case ImageSource::Gathered:
            if (!c->d_gather) return fail(c, MRT_ERR_STATE, "%s: nothing gathered yet (mrt_gather / mrt_gather_rccl on the root)", who);
            if (c->gather_bytes < (size_t)c->args.height * c->args.width * 16) return fail(c, MRT_ERR_STATE, "%s: the gathered frame is smaller than the image", who);
            return MRT_OK;
        case ImageSource::Accumulated: break;        // (always there)
    }
    return MRT_OK;
}

int source_queue(mrt_ctx* c, ImageSource source, SourceImage* out) {
    if (source == ImageSource::Denoised || source == ImageSource::GatheredDenoised) MRT_TRY(queue_denoise(c, source == ImageSource::GatheredDenoised));
    if (source == ImageSource::Temporal) MRT_TRY(queue_temporal_image(c));
    if (source == ImageSource::View) MRT_TRY(queue_view(c));
    // (den.out() is read behind the queue, which may allocate it; the frame count is what the image shows: the gather's snapshot)
    const float* img = source == ImageSource::Accumulated ? c->d_fb[c->target ^ 1] : source == ImageSource::Gathered ? c->d_gather : c->den.out();
    *out = {img, source_rows(c, source), source == ImageSource::GatheredDenoised ? c->gather_frames : c->frames_done};
    return MRT_OK;
}

}  // namespace mrt

extern "C" {

void mrt_denoise_params_default(mrt_denoise_params* out) {
    if (out) *out = mrt::denoise_defaults();
}

int mrt_set_denoise_params(mrt_ctx* c, const mrt_denoise_params* params) {
    if (!params) return MRT_ERR_INVALID_ARG;
    if (!denoise_params_ok(params))
        return !c ? (int)MRT_ERR_INVALID_ARG : fail(c, MRT_ERR_INVALID_ARG, "mrt_set_denoise_params: size %u (%zu), iterations %u (1..8), normal_exp %u (0..16), "
                    "sigma_l %g, sigma_z %g, sigma_a %g (finite, > 0), reserved 0", params->size, sizeof(mrt_denoise_params),
                    params->iterations, params->normal_exp, params->sigma_l, params->sigma_z, params->sigma_a);
    if (c) c->denoise = *params;          // (ctx NULL: a check of the parameters alone)
    return MRT_OK;
}

int mrt_get_denoise_params(mrt_ctx* c, mrt_denoise_params* out) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    *out = c->denoise;
    return MRT_OK;
}

int mrt_set_denoise_variance(mrt_ctx* c, uint32_t mode, uint32_t spatial_frames) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (mode > MRT_DENOISE_VAR_SPATIAL_EARLY || spatial_frames < 1 || spatial_frames > 64)
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_set_denoise_variance: mode %u (0..2), spatial_frames %u (1..64)", mode, spatial_frames);
    c->denoise_var_mode = mode;
    c->denoise_spatial_frames = spatial_frames;
    return MRT_OK;
}

int mrt_get_denoise_variance(mrt_ctx* c, uint32_t* mode, uint32_t* spatial_frames) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (mode) *mode = c->denoise_var_mode;
    if (spatial_frames) *spatial_frames = c->denoise_spatial_frames;
    return MRT_OK;
}

void mrt_denoise_mix_default(mrt_denoise_mix* out) {
    if (out) *out = mrt::denoise_mix_defaults();
}

int mrt_set_denoise_mix(mrt_ctx* c, const mrt_denoise_mix* p) {
    if (!p) return MRT_ERR_INVALID_ARG;
    if (!denoise_mix_ok(p))
        return !c ? (int)MRT_ERR_INVALID_ARG : fail(c, MRT_ERR_INVALID_ARG, "mrt_set_denoise_mix: size %u (%zu), enabled %u (0, 1), gain %g (finite, 0.25..16), "
                    "reserved 0", p->size, sizeof(mrt_denoise_mix), p->enabled, p->gain);
    if (c) c->denoise_mix = *p;           // (ctx NULL: a check of the setting alone)
    return MRT_OK;
}

int mrt_get_denoise_mix(mrt_ctx* c, mrt_denoise_mix* out) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    *out = c->denoise_mix;
    return MRT_OK;
}

int mrt_set_denoise_adaptive(mrt_ctx* c, int enabled) {
    if (!c) return MRT_ERR_INVALID_ARG;
    c->denoise_adaptive = enabled != 0;
    return MRT_OK;
}

int mrt_get_denoise_adaptive(mrt_ctx* c, int* enabled) {
    if (!c || !enabled) return MRT_ERR_INVALID_ARG;
    *enabled = c->denoise_adaptive ? 1 : 0;
    return MRT_OK;
}

int mrt_read_denoised(mrt_ctx* c, float* out, size_t cap) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    return read_source(c, ImageSource::Denoised, __func__, out, cap);
}

int mrt_read_gathered_denoised(mrt_ctx* c, float* out, size_t cap) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    return read_source(c, ImageSource::GatheredDenoised, __func__, out, cap);
}

void mrt_temporal_params_default(mrt_temporal_params* out) {
    if (out) *out = mrt::temporal_defaults();
}

int mrt_set_temporal(mrt_ctx* c, int enabled, const mrt_temporal_params* params) {
    if (!c && !params) return MRT_ERR_INVALID_ARG;
    if (params && !temporal_params_ok(params))
        return !c ? (int)MRT_ERR_INVALID_ARG : fail(c, MRT_ERR_INVALID_ARG, "mrt_set_temporal: size %u (%zu), max_history %u (1..256), spatial_len %u (1..16), "
                    "depth_tol %g (finite, > 0), reserved 0", params->size, sizeof(mrt_temporal_params), params->max_history,
                    params->spatial_len, params->depth_tol);
    if (!c) return MRT_OK;              // (ctx NULL: a check of the parameters alone)
    if (enabled && c->shard_world != 1) return fail(c, MRT_ERR_STATE, "mrt_set_temporal: a shard (world %u) has no temporal history", c->shard_world);
    if (!enabled && c->temporal_on) {   // the history goes; queued steps and reads may still use it
        HIP_TRY(c, hipSetDevice(c->device));
        MRT_TRY(mrt::wait_stream(c, c->stream, "mrt_set_temporal: releasing the history"));
        c->den.free_history();
        mrt::drop_temporal_history(c);
    }
    if (params) c->temporal = *params;
    c->temporal_on = enabled != 0;
    return MRT_OK;
}

int mrt_get_temporal(mrt_ctx* c, int* enabled, mrt_temporal_params* out) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (enabled) *enabled = c->temporal_on ? 1 : 0;
    if (out) *out = c->temporal;
    return MRT_OK;
}

void mrt_temporal_response_default(mrt_temporal_response* out) {
    if (out) *out = mrt::temporal_response_defaults();
}

int mrt_set_temporal_response(mrt_ctx* c, const mrt_temporal_response* r) {
    if (!r) return MRT_ERR_INVALID_ARG;
    if (!temporal_response_ok(r))
        return !c ? (int)MRT_ERR_INVALID_ARG : fail(c, MRT_ERR_INVALID_ARG, "mrt_set_temporal_response: size %u (%zu), enabled %u (0, 1), fast_history %u (1..16), "
                    "clamp_sigma %g (finite, > 0), antilag %g (0..1), reserved 0", r->size, sizeof(mrt_temporal_response), r->enabled,
                    r->fast_history, r->clamp_sigma, r->antilag);
    if (!c) return MRT_OK;              // (ctx NULL: a check of the setting alone)
    // another kind of history from the next step on: what is there goes (nothing queued, nothing freed; the H2 pair comes with
    // the first step that needs it)
    if (r->enabled != c->temporal_response.enabled) mrt::drop_temporal_history(c);
    c->temporal_response = *r;
    return MRT_OK;
}

int mrt_get_temporal_response(mrt_ctx* c, mrt_temporal_response* out) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    *out = c->temporal_response;
    return MRT_OK;
}

int mrt_temporal_step(mrt_ctx* c) {
    if (!c) return MRT_ERR_INVALID_ARG;
    MRT_TRY(temporal_check(c, "mrt_temporal_step", false));
    if (c->frames_done == 0) return fail(c, MRT_ERR_STATE, "mrt_temporal_step: no frame since mrt_create / mrt_reset");
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(ensure_guides(c));
    const uint32_t cur = c->temporal_cur;
    const mrt_temporal_response& resp = c->temporal_response;
    if (c->temporal_clear) MRT_TRY(clear_history(c));       // every length 0: no tap of this step counts
    mrt::TemporalArgs a;
    std::memset(&a, 0, sizeof a);
    a.fb = c->d_fb[c->target ^ 1];
    a.rays = c->d_guide_rays; a.guides = c->d_guides; a.shade = c->d_shade; a.prev_xyzr = c->d_prev_xyzr;
    a.h0_in = c->den.h0(cur); a.h1_in = c->den.h1(cur);
    a.h0_out = c->den.h0(cur ^ 1); a.h1_out = c->den.h1(cur ^ 1);
    a.width = c->args.width; a.height = c->args.height; a.n_spheres = c->n_spheres;
    temporal_camera(c->temporal_prev_cam, a.M, a.o_prev);
    a.max_history = (float)c->temporal.max_history; a.depth_tol = c->temporal.depth_tol;
    // with the response on: the same step with the fast history, then the clamp in place on its output
    const mrt::TemporalFastArgs f{c->den.h2(cur), c->den.h2(cur ^ 1), (float)resp.fast_history};
    int e = resp.enabled ? mrt::launch_temporal_reproject_fast(a, f, c->stream) : mrt::launch_temporal_reproject(a, c->stream);
    if (e) return fail(c, MRT_ERR_HIP, "temporal reprojection launch failed: %s", hipGetErrorString((hipError_t)e));
    if (resp.enabled) {
        const mrt::TemporalClampArgs k{a.h0_out, a.h1_out, f.h2_out, a.width, a.height, f.fast_history, resp.clamp_sigma, resp.antilag};
        e = mrt::launch_temporal_clamp(k, c->stream);
        if (e) return fail(c, MRT_ERR_HIP, "temporal clamp launch failed: %s", hipGetErrorString((hipError_t)e));
    }
    // "previous" from here on: the state at this step
    e = mrt::launch_temporal_snapshot(c->d_shade, c->d_prev_xyzr, c->n_spheres, c->stream);
    if (e) return fail(c, MRT_ERR_HIP, "temporal snapshot launch failed: %s", hipGetErrorString((hipError_t)e));
    c->temporal_prev_cam = c->cam_raw;
    c->temporal_cur = cur ^ 1;
    c->temporal_stepped = true;
    return MRT_OK;
}

int mrt_temporal_reset(mrt_ctx* c) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (!c->temporal_on) return fail(c, MRT_ERR_STATE, "mrt_temporal_reset: temporal reprojection is off (mrt_set_temporal)");
    mrt::drop_temporal_history(c);      // (the next step zeroes the lengths it reads, on the stream, before it reads them)
    return MRT_OK;
}

int mrt_read_temporal(mrt_ctx* c, float* out, size_t cap) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    return read_source(c, ImageSource::Temporal, __func__, out, cap);
}

void mrt_view_default(mrt_view* out) {
    if (out) *out = mrt::view_defaults();
}

int mrt_set_view(mrt_ctx* c, const mrt_view* v) {
    if (!v) return MRT_ERR_INVALID_ARG;
    if (!view_ok(v))
        return !c ? (int)MRT_ERR_INVALID_ARG : fail(c, MRT_ERR_INVALID_ARG, "mrt_set_view: size %u (%zu), kind %u (1..7), ramp %u (0, 1), lo %g, hi %g (finite, "
                    "hi != lo, 1 / (hi - lo) finite), rel_floor %g (finite, >= 0), reserved 0", v->size, sizeof(mrt_view), v->kind, v->ramp,
                    v->lo, v->hi, v->rel_floor);
    if (c) c->view = *v;                  // (ctx NULL: a check of the setting alone)
    return MRT_OK;
}

int mrt_get_view(mrt_ctx* c, mrt_view* out) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    *out = c->view;
    return MRT_OK;
}

int mrt_read_view(mrt_ctx* c, float* out, size_t cap) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    return read_source(c, ImageSource::View, __func__, out, cap);
}

int mrt_debug_read_temporal(mrt_ctx* c, float* h0, float* h1, float* prev_xyzr, size_t cap) {
    if (!c) return MRT_ERR_INVALID_ARG;
    MRT_TRY(history_io_opening(c, __func__, false));
    const size_t n = (size_t)c->args.width * c->args.height;
    if (cap < n || (prev_xyzr && cap < c->n_spheres)) return fail(c, MRT_ERR_TOO_SMALL, "mrt_debug_read_temporal: need %zu pixels, %u spheres", n, c->n_spheres);
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t cur = c->temporal_cur;
    if (c->temporal_clear) MRT_TRY(clear_history(c));       // (a dropped history reads as what the next step will see)
    if (h0) HIP_TRY(c, hipMemcpyAsync(h0, c->den.h0(cur), n * 16, hipMemcpyDeviceToHost, c->stream));
    if (h1) HIP_TRY(c, hipMemcpyAsync(h1, c->den.h1(cur), n * 16, hipMemcpyDeviceToHost, c->stream));
    if (prev_xyzr && c->n_spheres) HIP_TRY(c, hipMemcpyAsync(prev_xyzr, c->d_prev_xyzr, (size_t)c->n_spheres * 16, hipMemcpyDeviceToHost, c->stream));
    return mrt::wait_stream(c, c->stream, __func__);
}

int mrt_debug_load_temporal(mrt_ctx* c, const float* h0, const float* h1, const float* prev_xyzr, size_t n_spheres,
                            const mrt_camera_raw* prev_cam) {
    if (!c) return MRT_ERR_INVALID_ARG;
    MRT_TRY(history_io_opening(c, __func__, false));
    if (prev_xyzr && n_spheres != c->n_spheres) return fail(c, MRT_ERR_INVALID_ARG, "mrt_debug_load_temporal: %zu spheres for a scene of %u", n_spheres, c->n_spheres);
    const size_t n = (size_t)c->args.width * c->args.height;
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t cur = c->temporal_cur;
    if (c->temporal_clear) MRT_TRY(clear_history(c, !h0, !prev_cam));       // (only where the caller brings nothing in its place)
    if (h0) HIP_TRY(c, hipMemcpyAsync(c->den.h0(cur), h0, n * 16, hipMemcpyHostToDevice, c->stream));
    if (h1) HIP_TRY(c, hipMemcpyAsync(c->den.h1(cur), h1, n * 16, hipMemcpyHostToDevice, c->stream));
    if (prev_xyzr && c->n_spheres) HIP_TRY(c, hipMemcpyAsync(c->d_prev_xyzr, prev_xyzr, (size_t)c->n_spheres * 16, hipMemcpyHostToDevice, c->stream));
    MRT_TRY(mrt::wait_stream(c, c->stream, __func__));      // (the caller's arrays are pageable: theirs again on return)
    if (prev_cam) c->temporal_prev_cam = *prev_cam;
    c->temporal_stepped = true;
    return MRT_OK;
}

int mrt_debug_read_temporal_fast(mrt_ctx* c, float* h2, size_t cap) {
    if (!c || !h2) return MRT_ERR_INVALID_ARG;
    MRT_TRY(history_io_opening(c, __func__, true));
    const size_t n = (size_t)c->args.width * c->args.height;
    if (cap < n) return fail(c, MRT_ERR_TOO_SMALL, "mrt_debug_read_temporal_fast: need %zu pixels", n);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->temporal_clear) MRT_TRY(clear_history(c));
    HIP_TRY(c, hipMemcpyAsync(h2, c->den.h2(c->temporal_cur), n * 16, hipMemcpyDeviceToHost, c->stream));
    return mrt::wait_stream(c, c->stream, __func__);
}

int mrt_debug_load_temporal_fast(mrt_ctx* c, const float* h2) {
    if (!c || !h2) return MRT_ERR_INVALID_ARG;
    MRT_TRY(history_io_opening(c, __func__, true));
    const size_t n = (size_t)c->args.width * c->args.height;
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->temporal_clear) MRT_TRY(clear_history(c));
    HIP_TRY(c, hipMemcpyAsync(c->den.h2(c->temporal_cur), h2, n * 16, hipMemcpyHostToDevice, c->stream));
    MRT_TRY(mrt::wait_stream(c, c->stream, __func__));      // (the caller's array is pageable: theirs again on return)
    c->temporal_stepped = true;
    return MRT_OK;
}

int mrt_debug_read_guides(mrt_ctx* c, float* rays, int32_t* index, float* t, float* normal, float* albedo, size_t cap) {
    if (!c) return MRT_ERR_INVALID_ARG;
    MRT_TRY(denoise_check(c, "mrt_debug_read_guides", false));
    return read_guides(c, "mrt_debug_read_guides", rays, index, t, normal, albedo, cap);
}

int mrt_debug_read_gathered_guides(mrt_ctx* c, float* rays, int32_t* index, float* t, float* normal, float* albedo, size_t cap) {
    if (!c) return MRT_ERR_INVALID_ARG;
    MRT_TRY(gathered_denoise_check(c, "mrt_debug_read_gathered_guides", false));
    return read_guides(c, "mrt_debug_read_gathered_guides", rays, index, t, normal, albedo, cap);
}

int mrt_debug_denoise(mrt_ctx* c, const float* rgba, const float* S, double K, const float* guides, uint32_t width, uint32_t rows,
                      const mrt_denoise_params* params, float* out) {
    return mrt_debug_denoise_variance(c, rgba, S, K, guides, width, rows, params, 0, out);
}

int mrt_debug_denoise_variance(mrt_ctx* c, const float* rgba, const float* S, double K, const float* guides, uint32_t width,
                               uint32_t rows, const mrt_denoise_params* params, uint32_t variance, float* out) {
    return debug_denoise(c, rgba, S, K, guides, width, rows, params, variance, nullptr, out);
}

int mrt_debug_denoise_mix(mrt_ctx* c, const float* rgba, const float* S, double K, const float* guides, uint32_t width,
                          uint32_t rows, const mrt_denoise_params* params, uint32_t variance, const mrt_denoise_mix* mix, float* out) {
    if (!c || !mix) return MRT_ERR_INVALID_ARG;
    if (!denoise_mix_ok(mix)) return fail(c, MRT_ERR_INVALID_ARG, "mrt_debug_denoise_mix: bad setting");
    return debug_denoise(c, rgba, S, K, guides, width, rows, params, variance, mix, out);
}

}  // extern "C"
