// Headless counterpart of native-runner/src/main.rs: the same five flags
// (main.rs:20-31: --width --height --samples-per-frame --ray-depth --max-framebuffer-weight)
// driving the MI355X backend through the C ABI, plus what a windowless run needs
// (--frames, --seed, --scene, --out, --device; --warmup N renders N untimed frames first and restarts the accumulation;
// --rng stream|counter selects the RNG mode, MRT_RNG_*).  The reference renders forever into a
// window (lib.rs:187-192); this renders --frames frames and writes the image.
// --gpus N (devices 0..N-1) or --devices a,b,c tile-shards the frame over several GPUs from this one
// process: one context per GPU, interleaved 8-row bands, one mrt_gather per frame onto the first device
// (SURVEY.md 8e).  A device may be listed more than once (--devices 0,0 rehearses the path on one GPU).

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/myraytracer_amd.h"

static void usage() {
    std::fprintf(stderr,
        "usage: native_runner [--width N] [--height N] [--samples-per-frame N] [--ray-depth N]\n"
        "                     [--max-framebuffer-weight F] [--frames N] [--warmup N] [--seed N] [--rng stream|counter]\n"
        "                     [--scene default|cover|cover-glass|stress | --scene-file FILE] [--save-scene FILE]\n"
        "                     [--out FILE.pfm|FILE.ppm|FILE.png] [--device N | --gpus N | --devices a,b,...]\n"
                         "                     [--schedule div,mult] [--target-noise REL [--check-every N] [--adaptive | --budget N [--plan-on-device]]]\n"
        "                     [--denoise-out FILE [--denoise-variance accumulated|prefiltered|spatial-early[:N]] [--denoise-mix [GAIN]]]\n"
        "                     [--snapshot-every N --snapshot-out PREFIX] [--view KIND[:LO:HI[:RAMP]] --view-out FILE]\n"
        "  --target-noise REL: render until the noise estimate's relative RMSE is <= REL (--frames is then the cap), checking\n"
        "                      every --check-every frames (default 16); prints the final report\n"
        "  --adaptive:         with --target-noise (one GPU): every chunk after the first renders only the tiles the report one\n"
        "                      check earlier finds noisy, and the loop also stops when no pixel is above rel 0.02; prints frames,\n"
        "                      samples and tiles selected per check\n"
        "  --budget N:         with --target-noise (one GPU): every chunk after the first spends N tile-frames (one frame of one 8x8\n"
        "                      tile each) where the summed-S map of the report one check earlier says they lower the image's\n"
        "                      variance most, at most min(--check-every, 32) per tile (mrt_render_budget); prints each chunk's allocation\n"
        "  --plan-on-device:   with --budget: the queries allocate on the device behind their reduction (mrt_noise_query_budget) and the\n"
        "                      chunks render those plans (mrt_render_planned: a plan is a target, frames queued since its query count)\n"
        "  --denoise-out FILE: noise tracking on; also writes the denoised final frame (.pfm / .ppm / .png); with several GPUs the\n"
        "                      noise estimate is gathered with the frame and the first GPU denoises the gathered frame; with\n"
        "                      --adaptive the per-tile filter of an adaptive accumulation is turned on (mrt_set_denoise_adaptive)\n"
        "  --denoise-variance: the luminance stop's variance (mrt_set_denoise_variance): the pixel's own accumulated estimate\n"
        "                      (default), its 3 x 3 prefilter, or a spatial estimate while fewer than N frames (default 3) are done\n"
        "  --denoise-mix [GAIN]: with --denoise-out: blend the filtered with the accumulated image per pixel by the estimated error\n"
        "                      (mrt_set_denoise_mix); GAIN 0.25 .. 16, default the library's\n"
        "  --snapshot-every N --snapshot-out PREFIX: (one GPU, not with --target-noise) the frames are queued N at a time and the\n"
        "                      accumulation after each N is written as PREFIX<frames done, 5 digits>.pfm: the exact floats, presented\n"
        "                      through the ring (MRT_PRESENT_RGBA32F_LINEAR) without draining the frames in flight\n"
        "  --view KIND[:LO:HI[:RAMP]] --view-out FILE: (one GPU) after the last frame, writes a diagnostic view (mrt_set_view /\n"
        "                      mrt_read_view; .pfm / .ppm / .png): KIND noise_se | noise_rel | tile_frames | depth | normal | albedo |\n"
        "                      sphere, a scalar kind mapped from LO..HI (default 0:0.1) through RAMP grey | heat (default heat); the\n"
        "                      noise kinds turn noise tracking on\n");
}

int main(int argc, char** argv) {
    // The HOST's job, before its first HIP call: up to eight frames of a pixel-starved shard run side by
    // side, each on a stream of its own, and HIP gives a process 4 hardware queues unless told otherwise.  The library itself
    // never touches the environment.  A value the user exported wins.
    (void)setenv("GPU_MAX_HW_QUEUES", "20", 0);
    mrt_args args;
    mrt_args_default(&args);
    uint32_t frames = 1, warmup = 0, rng_mode = MRT_RNG_PIXEL_STREAM; uint64_t seed = 1; int device = 0;
    uint32_t hint_div = 0, hint_mult = 0, check_every = 16, denoise_var = MRT_DENOISE_VAR_ACCUMULATED, spatial_frames = 3;
    double target_noise = -1.0;
    bool adaptive = false, plan_on_device = false;
    uint64_t budget = 0;
    uint32_t snapshot_every = 0;
    std::string snapshot_out;
    mrt_denoise_mix mix;
    mrt_denoise_mix_default(&mix);
    std::string scene = "default", scene_file, save_scene, out, denoise_out, view_out;
    mrt_view view;
    mrt_view_default(&view);
    bool have_view = false;
    std::vector<int> devices;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i], v;
        size_t eq = a.find('=');
        if (eq != std::string::npos) { v = a.substr(eq + 1); a = a.substr(0, eq); }
        else if (a == "--help" || a == "-h") { usage(); return 0; }
        else if (a == "--adaptive") { adaptive = true; continue; }
        else if (a == "--plan-on-device") { plan_on_device = true; continue; }
        else if (a == "--denoise-mix" && (i + 1 >= argc || !std::strncmp(argv[i + 1], "--", 2))) { mix.enabled = 1; continue; }   // (no GAIN)
        else if (i + 1 < argc) v = argv[++i];
        else { usage(); return 2; }
        if (a == "--width") args.width = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (a == "--height") args.height = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (a == "--samples-per-frame") args.samples_per_frame = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (a == "--ray-depth") args.ray_depth = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (a == "--max-framebuffer-weight") args.max_framebuffer_weight = std::strtof(v.c_str(), nullptr);
        else if (a == "--frames") frames = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (a == "--warmup") warmup = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (a == "--rng") {
            if (v == "counter") rng_mode = MRT_RNG_COUNTER;
            else if (v != "stream") { std::fprintf(stderr, "unknown --rng %s\n", v.c_str()); return 2; }
        }
        else if (a == "--seed") seed = std::strtoull(v.c_str(), nullptr, 10);
        else if (a == "--scene") scene = v;
        else if (a == "--scene-file") scene_file = v;
        else if (a == "--save-scene") save_scene = v;
        else if (a == "--schedule") {       // "div,mult": pin the launch schedule on every GPU (mrt_set_schedule_hint)
            if (std::sscanf(v.c_str(), "%u,%u", &hint_div, &hint_mult) != 2) { std::fprintf(stderr, "--schedule wants div,mult\n"); return 2; }
        }
        else if (a == "--out") out = v;
        else if (a == "--denoise-out") denoise_out = v;
        else if (a == "--denoise-mix") { mix.enabled = 1; mix.gain = std::strtof(v.c_str(), nullptr); }
        else if (a == "--denoise-variance") {
            const size_t colon = v.find(':');
            const std::string m = v.substr(0, colon);
            if (m == "accumulated") denoise_var = MRT_DENOISE_VAR_ACCUMULATED;
            else if (m == "prefiltered") denoise_var = MRT_DENOISE_VAR_PREFILTERED;
            else if (m == "spatial-early") denoise_var = MRT_DENOISE_VAR_SPATIAL_EARLY;
            else { std::fprintf(stderr, "unknown --denoise-variance %s\n", v.c_str()); return 2; }
            if (colon != std::string::npos) {
                if (denoise_var != MRT_DENOISE_VAR_SPATIAL_EARLY) { std::fprintf(stderr, "--denoise-variance: only spatial-early takes :N\n"); return 2; }
                spatial_frames = (uint32_t)std::strtoul(v.c_str() + colon + 1, nullptr, 10);
            }
        }
        else if (a == "--view") {           // KIND[:LO:HI[:RAMP]]
            static const char* const kinds[] = {"noise_se", "noise_rel", "tile_frames", "depth", "normal", "albedo", "sphere"};
            std::vector<std::string> part;
            for (size_t p0 = 0; p0 <= v.size();) {
                const size_t p1 = v.find(':', p0) == std::string::npos ? v.size() : v.find(':', p0);
                part.push_back(v.substr(p0, p1 - p0));
                p0 = p1 + 1;
            }
            view.kind = 0;
            for (uint32_t k = 0; k < 7; k++)
                if (part[0] == kinds[k]) view.kind = k + 1;
            if (!view.kind || part.size() == 2 || part.size() > 4) { std::fprintf(stderr, "--view wants KIND[:LO:HI[:RAMP]], got %s\n", v.c_str()); return 2; }
            if (part.size() >= 3) { view.lo = std::strtof(part[1].c_str(), nullptr); view.hi = std::strtof(part[2].c_str(), nullptr); }
            if (part.size() == 4) {
                if (part[3] == "grey") view.ramp = MRT_VIEW_RAMP_GREY;
                else if (part[3] == "heat") view.ramp = MRT_VIEW_RAMP_HEAT;
                else { std::fprintf(stderr, "unknown --view ramp %s\n", part[3].c_str()); return 2; }
            }
            if (mrt_set_view(nullptr, &view) != MRT_OK) { std::fprintf(stderr, "--view %s: LO and HI must be finite and differ\n", v.c_str()); return 2; }
            have_view = true;
        }
        else if (a == "--view-out") view_out = v;
        else if (a == "--device") device = std::atoi(v.c_str());
        else if (a == "--target-noise") target_noise = std::strtod(v.c_str(), nullptr);
        else if (a == "--budget") budget = std::strtoull(v.c_str(), nullptr, 10);
        else if (a == "--snapshot-every") snapshot_every = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (a == "--snapshot-out") snapshot_out = v;
        else if (a == "--check-every") check_every = (uint32_t)std::strtoul(v.c_str(), nullptr, 10);
        else if (a == "--gpus") { devices.clear(); for (int d = 0; d < std::atoi(v.c_str()); d++) devices.push_back(d); }
        else if (a == "--devices") {
            devices.clear();
            for (size_t p0 = 0; p0 <= v.size();) {
                const size_t p1 = v.find(',', p0) == std::string::npos ? v.size() : v.find(',', p0);
                if (p1 > p0) devices.push_back(std::atoi(v.substr(p0, p1 - p0).c_str()));
                p0 = p1 + 1;
            }
        }
        else { std::fprintf(stderr, "unknown flag %s\n", a.c_str()); usage(); return 2; }
    }
    mrt_args_resolve_size(&args);

    std::vector<mrt_sphere> spheres(70000);
    mrt_camera cam; std::memset(&cam, 0, sizeof cam);
    int n;
    if (!scene_file.empty()) {
        // scenes as data: count first, then read
        int has_cam = 0;
        n = mrt_scene_load(scene_file.c_str(), nullptr, 0, &cam, &has_cam);
        if (n >= 0) { spheres.resize((size_t)n + 1); n = mrt_scene_load(scene_file.c_str(), spheres.data(), spheres.size(), &cam, &has_cam); }
        if (n < 0) { std::fprintf(stderr, "%s: %s (%s)\n", scene_file.c_str(), mrt_status_string(-n), mrt_last_error(nullptr)); return 1; }
    }
    else if (scene == "default") n = mrt_scene_default(spheres.data(), spheres.size());
    else if (scene == "cover") n = mrt_scene_cover(1, 0, spheres.data(), spheres.size(), &cam);
    else if (scene == "cover-glass") n = mrt_scene_cover(1, 1, spheres.data(), spheres.size(), &cam);
    else if (scene == "stress") n = mrt_scene_stress(1, 100, spheres.data(), spheres.size(), &cam);
    else { std::fprintf(stderr, "unknown scene %s\n", scene.c_str()); return 2; }
    if (n < 0) { std::fprintf(stderr, "scene generation failed\n"); return 1; }
    if (!save_scene.empty()) {
        const int ss = mrt_scene_save(save_scene.c_str(), spheres.data(), (size_t)n, &cam);
        if (ss != MRT_OK) { std::fprintf(stderr, "%s: %s (%s)\n", save_scene.c_str(), mrt_status_string(ss), mrt_last_error(nullptr)); return 1; }
    }

    // one context per GPU; with a single device this is exactly the reference's one State
    if (devices.empty()) devices.push_back(device);
    const uint32_t n_gpus = (uint32_t)devices.size();
    std::vector<mrt_ctx*> ctxs(n_gpus, nullptr);
    auto destroy_all = [&]() { for (mrt_ctx* c : ctxs) mrt_destroy(c); };
#define TRY(ctx, call) do { int s_ = (call); if (s_ != MRT_OK) { std::fprintf(stderr, "%s: %s (%s)\n", #call, mrt_status_string(s_), mrt_last_error(ctx)); destroy_all(); return 1; } } while (0)
    for (uint32_t i = 0; i < n_gpus; i++) {
        int st = mrt_create(&args, seed, devices[i], &ctxs[i]);
        if (st != MRT_OK) { std::fprintf(stderr, "mrt_create(device %d): %s (%s)\n", devices[i], mrt_status_string(st), mrt_last_error(nullptr)); destroy_all(); return 1; }
        if (n_gpus > 1) TRY(ctxs[i], mrt_set_shard(ctxs[i], i, n_gpus));
        TRY(ctxs[i], mrt_set_world(ctxs[i], spheres.data(), (size_t)n));
        TRY(ctxs[i], mrt_set_camera(ctxs[i], &cam));
        if (rng_mode != MRT_RNG_PIXEL_STREAM) TRY(ctxs[i], mrt_set_rng_mode(ctxs[i], rng_mode));
        if (hint_div) TRY(ctxs[i], mrt_set_schedule_hint(ctxs[i], hint_div, hint_mult));
        const bool noise_view = have_view && (view.kind == MRT_VIEW_NOISE_SE || view.kind == MRT_VIEW_NOISE_REL);
        if (target_noise >= 0.0 || !denoise_out.empty() || noise_view) TRY(ctxs[i], mrt_set_noise_tracking(ctxs[i], 1));
        if (have_view) TRY(ctxs[i], mrt_set_view(ctxs[i], &view));
        TRY(ctxs[i], mrt_set_denoise_variance(ctxs[i], denoise_var, spatial_frames));
        // an adaptive run's tiles end at their own frame counts: its denoise is the per-tile filter (one GPU: checked below)
        if ((adaptive || budget) && !denoise_out.empty()) TRY(ctxs[i], mrt_set_denoise_adaptive(ctxs[i], 1));
        TRY(ctxs[i], mrt_set_denoise_mix(ctxs[i], &mix));
    }
    // several GPUs: the noise estimate travels with the gather, and the first GPU denoises the gathered frame
    if (!denoise_out.empty() && n_gpus > 1) TRY(ctxs[0], mrt_set_gather_noise(ctxs[0], 1));
    if (mix.enabled && denoise_out.empty()) { std::fprintf(stderr, "--denoise-mix wants --denoise-out\n"); destroy_all(); return 2; }
    if (have_view != !view_out.empty() || (have_view && n_gpus > 1)) { std::fprintf(stderr, "--view KIND and --view-out FILE go together, on one GPU\n"); destroy_all(); return 2; }
    if (check_every == 0) { std::fprintf(stderr, "--check-every wants N >= 1\n"); destroy_all(); return 2; }
    if (adaptive && (target_noise < 0.0 || n_gpus > 1)) { std::fprintf(stderr, "--adaptive wants --target-noise and one GPU\n"); destroy_all(); return 2; }
    if (budget && (adaptive || target_noise < 0.0 || n_gpus > 1)) { std::fprintf(stderr, "--budget wants --target-noise and one GPU, and not --adaptive\n"); destroy_all(); return 2; }
    if (plan_on_device && !budget) { std::fprintf(stderr, "--plan-on-device wants --budget\n"); destroy_all(); return 2; }
    if ((snapshot_every != 0) != !snapshot_out.empty()) { std::fprintf(stderr, "--snapshot-every N (>= 1) and --snapshot-out PREFIX go together\n"); destroy_all(); return 2; }
    if (snapshot_every && (target_noise >= 0.0 || n_gpus > 1)) { std::fprintf(stderr, "--snapshot-every wants one GPU and the plain --frames mode (not --target-noise)\n"); destroy_all(); return 2; }
    if (warmup) {           // untimed: the tile-cost estimate, buffers and peer mappings exist afterwards
        for (mrt_ctx* c : ctxs) TRY(c, mrt_render(c, warmup));
        if (n_gpus > 1) TRY(ctxs[0], mrt_gather(ctxs.data(), n_gpus, 0));
        for (mrt_ctx* c : ctxs) TRY(c, mrt_sync(c));
        for (mrt_ctx* c : ctxs) TRY(c, mrt_reset(c));
        // every GPU renders an equal share of the same frame: one launch schedule for all of them -- the first context's, if its
        // controller has settled (the setting is measured on the host's clock: GPUs may otherwise decide differently)
        uint32_t sch[6] = {0, 0, 0, 0, 0, 0};
        TRY(ctxs[0], mrt_get_schedule(ctxs[0], sch));
        if (n_gpus > 1 && !hint_div && sch[0] != 0 && sch[2] != 0)
            for (mrt_ctx* c : ctxs) TRY(c, mrt_set_schedule_hint(c, sch[0], sch[1]));
    }
    for (mrt_ctx* c : ctxs) TRY(c, mrt_sync(c));
    auto t0 = std::chrono::steady_clock::now();
    // only the final accumulated image is wanted, so every GPU renders all its frames (mrt_render may share a launch
    // among several frames when its shard is too small to fill the GPU) and the shards are gathered once
    mrt_noise_report report{};
    if (snapshot_every) {
        // --snapshot-every: chunks of N frames, each followed by a present of the exact floats (bottom-up, as PFM wants them);
        // the images are taken in FIFO order as their copies land -- polled between chunks, waited for only after the last --
        // and the frames stay in flight: no mrt_read_framebuffer before the final --out.  At most depth - 1 presents are kept
        // outstanding (nothing is dropped then: a full ring waits for its oldest image); the depth is known from the first image on
        mrt_ctx* c = ctxs[0];
        uint32_t outstanding = 0, keep = 1, written = 0;
        auto take = [&](int wait) -> int {                   // 1: wrote one, 0: none has finished, < 0: failed
            const uint8_t* px = nullptr;
            mrt_present_info info{};
            const int s_ = mrt_present_acquire(c, MRT_ACQUIRE_OLDEST, wait, &px, &info);
            if (s_ != MRT_OK) { std::fprintf(stderr, "mrt_present_acquire: %s (%s)\n", mrt_status_string(s_), mrt_last_error(c)); return -1; }
            if (!px) return 0;
            if (info.dropped) { std::fprintf(stderr, "--snapshot-every: %u snapshot(s) before frame %u were dropped\n", info.dropped, info.frames_done); return -1; }
            char name[16];
            std::snprintf(name, sizeof name, "%05u.pfm", info.frames_done);
            const std::string path = snapshot_out + name;
            if (mrt_write_pfm(path.c_str(), reinterpret_cast<const float*>(px), info.width, info.rows) != MRT_OK) {
                std::fprintf(stderr, "cannot write %s\n", path.c_str());
                return -1;
            }
            keep = std::max(1u, info.ring_depth - 1u);
            outstanding--; written++;
            return 1;
        };
        for (uint32_t done = 0; done < frames;) {
            const uint32_t k = std::min(snapshot_every, frames - done);
            TRY(c, mrt_render(c, k));
            done += k;
            while (outstanding >= keep) if (take(1) <= 0) { destroy_all(); return 1; }
            TRY(c, mrt_present(c, MRT_PRESENT_RGBA32F_LINEAR, 0));
            outstanding++;
            for (int r = 1; r == 1 && outstanding;) if ((r = take(0)) < 0) { destroy_all(); return 1; }
        }
        while (outstanding) if (take(1) <= 0) { destroy_all(); return 1; }
        TRY(c, mrt_present_release(c));
        std::printf("wrote %u snapshots %s<frames done>.pfm\n", written, snapshot_out.c_str());
    } else if (target_noise < 0.0) {
        for (mrt_ctx* c : ctxs) TRY(c, mrt_render(c, frames));               // asynchronous: all GPUs render at once
    } else {
        // --target-noise: chunks of check_every frames; chunk k + 1 is queued before report k is waited for (the pipeline stays
        // full), so the stop overshoots the first report that meets the target by at most one chunk
        // --adaptive: every chunk after the first renders the tiles that the report one check before the newest finds noisy
        // (State.render_until(adaptive=True)'s loop); subset frames count as frames
        // --budget: every chunk after the first is mrt_render_budget from that report's summed-S map (render_until(budget=N)'s
        // loop: the queries leave that kind of map), and the loop also stops when a chunk finds nothing worth a frame
        uint32_t done = 0;
        uint64_t earlier = 0;             // that report (0: none yet)
        uint32_t selected = 0;            // the tiles of the latest chunk
        uint64_t tile_frames = 0;         // tiles x frames queued: at most 64 x spp samples each
        mrt_budget_result spent{};        // --budget: the latest chunk's allocation
        bool idle = false;                // ... which found nothing to spend on
        // --plan-on-device: the plans hold at most plan_frames frames a tile; a last chunk with fewer frames left is the host's
        const uint32_t plan_frames = std::min(check_every, 32u);
        auto chunk = [&]() -> int {
            const uint32_t k = std::min(check_every, frames - done);
            for (mrt_ctx* c : ctxs) {
                if (!k) continue;
                int s_ = MRT_OK;
                if (adaptive && earlier != 0) {
                    uint64_t used = 0;
                    s_ = mrt_render_adaptive(c, k, earlier, &used, &selected);
                } else if (budget && plan_on_device && earlier != 0 && k >= plan_frames) {
                    mrt_budget_result planned{};
                    s_ = mrt_render_planned(c, earlier, &spent, nullptr, 0);
                    if (s_ == MRT_OK) s_ = mrt_read_budget_plan(c, earlier, nullptr, 0, &planned);
                    idle = planned.tile_frames == 0;        // (a plan that is met already is not the end: the next one may not be)
                    tile_frames += spent.tile_frames;
                    selected = 0;
                } else if (budget && earlier != 0) {
                    s_ = mrt_render_budget(c, budget, std::min(k, 32u), earlier, &spent, nullptr, 0);
                    idle = spent.tile_frames == 0;
                    tile_frames += spent.tile_frames;
                    selected = 0;                       // (counted above: the levels differ in length)
                } else {
                    s_ = mrt_render(c, k);
                    uint32_t tx = 0, tr = 0;
                    (void)mrt_read_tile_frames(c, nullptr, 0, &tx, &tr);      // (the shape only)
                    selected = tx * tr;
                }
                if (s_ != MRT_OK) return s_;
            }
            tile_frames += (uint64_t)selected * (mrt_frames_done(ctxs[0]) - done);
            done = mrt_frames_done(ctxs[0]);
            return MRT_OK;
        };
        auto query = [&]() -> int {
            for (mrt_ctx* c : ctxs) {
                const int s_ = plan_on_device ? mrt_noise_query_budget(c, 0.02f, 0.01f, budget, plan_frames)
                                              : mrt_noise_query_map(c, 0.02f, 0.01f, budget ? MRT_TILE_MAP_SUM_S : MRT_TILE_MAP_MAX_REL);
                if (s_ != MRT_OK) return s_;
            }
            return MRT_OK;
        };
        TRY(ctxs[0], chunk());
        TRY(ctxs[0], query());
        for (;;) {
            TRY(ctxs[0], chunk());
            // every context's report of the previous check, combined: counts and sums added, the largest max_se
            mrt_noise_report r{};
            for (uint32_t i = 0; i < n_gpus; i++) {
                mrt_noise_report part{};
                TRY(ctxs[i], mrt_noise_result(ctxs[i], 1, &part));
                if (i == 0) { r = part; continue; }
                r.pixels += part.pixels; r.non_finite += part.non_finite; r.above += part.above;
                r.sum_var += part.sum_var; r.sum_lum += part.sum_lum;
                r.max_se = std::max(r.max_se, part.max_se);
            }
            if (n_gpus > 1 && !std::isinf(r.noise_factor)) {
                r.rmse = r.pixels ? std::sqrt(r.sum_var / (double)r.pixels) : 0.0;
                r.rel_rmse = r.rmse > 0.0 ? r.rmse / (r.sum_lum / (double)r.pixels) : 0.0;
            }
            report = r;
            if (adaptive)       // (no host wait here: the counted samples come after the loop)
                std::printf("check: report at frame %u: %llu pixels above, rel_rmse %.5g; %u frames queued, %u tiles in the latest chunk, "
                            "%llu samples at most\n", r.frames_done, (unsigned long long)r.above, r.rel_rmse, done, selected,
                            (unsigned long long)(tile_frames * 64u * args.samples_per_frame));
            if (budget && earlier != 0)
                std::printf("check: report at frame %u: rel_rmse %.5g; %u frames queued; the latest chunk: %llu tile-frames over %u tiles in "
                            "%u frames, modelled variance %.6g -> %.6g\n", r.frames_done, r.rel_rmse, done,
                            (unsigned long long)spent.tile_frames, spent.tiles, spent.frames, spent.var_before, spent.var_after);
            if (r.rel_rmse <= target_noise || r.frames_done >= frames || (adaptive && r.above == 0) || idle) break;
            earlier = r.seq;
            TRY(ctxs[0], query());
        }
        frames = done;
    }
    if (n_gpus > 1) TRY(ctxs[0], mrt_gather(ctxs.data(), n_gpus, 0));         // every shard's bands -> the first GPU
    for (mrt_ctx* c : ctxs) TRY(c, mrt_sync(c));
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double samples = (double)args.width * args.height * args.samples_per_frame * frames;
    if (adaptive || budget) {             // subset frames: the samples the render kernels counted
        mrt_counters cnt{};
        TRY(ctxs[0], mrt_read_counters(ctxs[0], &cnt));
        samples = (double)cnt.samples;
    }
    std::printf("%ux%u, %u spp x %u frames, depth %u, %d spheres, %u GPU(s): %.3f s, %.1f Msamples/s\n", args.width, args.height,
                args.samples_per_frame, frames, args.ray_depth, n, n_gpus, sec, samples / sec * 1e-6);
    if (target_noise >= 0.0)
        std::printf("noise: %u frames used (target rel_rmse %g); report at frame %u: rel_rmse %.5g, rmse %.5g, max_se %.5g, "
                    "%llu of %llu pixels above rel %.3g (%llu not finite)\n", frames, target_noise, report.frames_done,
                    report.rel_rmse, report.rmse, (double)report.max_se, (unsigned long long)report.above,
                    (unsigned long long)report.pixels, (double)report.threshold, (unsigned long long)report.non_finite);
    auto write_image = [&](const std::string& path, const std::vector<float>& fb) -> int {
        const std::string ext = path.size() > 4 ? path.substr(path.size() - 4) : "";
        int s2 = ext == ".ppm" ? mrt_write_ppm(path.c_str(), fb.data(), args.width, args.height)
               : ext == ".png" ? mrt_write_png(path.c_str(), fb.data(), args.width, args.height)
                               : mrt_write_pfm(path.c_str(), fb.data(), args.width, args.height);
        if (s2 != MRT_OK) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
        std::printf("wrote %s\n", path.c_str());
        return 0;
    };
    if (!out.empty()) {
        std::vector<float> fb((size_t)args.width * args.height * 4);
        if (n_gpus > 1) TRY(ctxs[0], mrt_read_gathered(ctxs[0], fb.data(), fb.size()));
        else TRY(ctxs[0], mrt_read_framebuffer(ctxs[0], fb.data(), fb.size()));
        if (write_image(out, fb)) { destroy_all(); return 1; }
    }
    if (!denoise_out.empty()) {
        std::vector<float> fb((size_t)args.width * args.height * 4);
        if (n_gpus > 1) TRY(ctxs[0], mrt_read_gathered_denoised(ctxs[0], fb.data(), fb.size()));
        else TRY(ctxs[0], mrt_read_denoised(ctxs[0], fb.data(), fb.size()));
        if (write_image(denoise_out, fb)) { destroy_all(); return 1; }
    }
    if (have_view) {
        std::vector<float> fb((size_t)args.width * args.height * 4);
        TRY(ctxs[0], mrt_read_view(ctxs[0], fb.data(), fb.size()));
        if (write_image(view_out, fb)) { destroy_all(); return 1; }
    }
    destroy_all();
    return 0;
}
