// The noise estimate of include/myraytracer_amd.h: S and its reports, and adaptive sampling's selection from them.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "mrt_ctx.h"

using mrt::fail, mrt::local_texels, mrt::free_noise_buffers, mrt::alloc_noise_buffers;

namespace mrt {

// noise tracking's per-texel buffers, sized like the framebuffers (mrt_set_noise_tracking)
void free_noise_buffers(mrt_ctx* c) { free_device(c->d_noise_s, c->d_noise_tiles, c->d_noise_partials); }

int alloc_noise_set(mrt_ctx* c, uint32_t local_bands, float** s, float** tiles, void** partials) {
    const size_t texels = (size_t)local_bands * kBandRows * c->args.width, n = texels ? texels : 1;
    const size_t n_tiles = (size_t)((c->args.width + kTileW - 1) / kTileW) * local_bands;
    // a tile map per report of the ring; behind them the reports' budget plans and the selection's scratch (budget_layout)
    const size_t map_floats = mrt::budget_layout(n_tiles, mrt_ctx::kNoiseRing).words;
    const int st = [&]() -> int {
        HIP_TRY(c, hipMalloc((void**)s, n * sizeof(float)));
        HIP_TRY(c, hipMemsetAsync(*s, 0, n * sizeof(float), c->stream));
        HIP_TRY(c, hipMalloc((void**)tiles, map_floats * sizeof(float)));
        HIP_TRY(c, hipMemsetAsync(*tiles, 0, map_floats * sizeof(float), c->stream));
        HIP_TRY(c, hipMalloc(partials, std::max<size_t>(mrt::noise_partials_bytes(c->args.width, local_bands), 64)));
        return MRT_OK;
    }();
    if (st != MRT_OK) free_device(*s, *tiles, *partials);      // (all three or none: S alone would switch the blends to tracking)
    return st;
}

int alloc_noise_buffers(mrt_ctx* c) {
    free_noise_buffers(c);
    MRT_TRY(alloc_noise_set(c, c->local_bands, &c->d_noise_s, &c->d_noise_tiles, &c->d_noise_partials));
    c->noise_first = c->noise_seq + 1;          // (reports of the old geometry are discarded)
    return MRT_OK;
}

// Adaptive sampling: K(n) = mrt_noise_factor(n, max_w) for n < len on the device (as float and as double), grown by doubling.
// The host table continues the c2 recursion of mrt_noise_factor; a larger device table replaces the old one after the ctx's
// stream -- the only one whose reductions read it -- has drained (a handful of times per accumulation).
int ensure_k_table(mrt_ctx* c, uint32_t len) {
    if (len <= c->k_len) return MRT_OK;
    uint32_t cap = std::max<uint32_t>(c->k_len ? c->k_len : 4096u, 4096u);
    while (cap < len) cap = cap > 0x7FFFFFFFu ? 0xFFFFFFFFu : 2u * cap;
    const float max_w = c->args.max_framebuffer_weight;
    while (c->k_table.size() < cap) {
        c->k_table.push_back(mrt::noise_factor_of(c->k_c2));     // K after k_table.size() frames
        c->k_c2 = mrt::noise_c2_step(c->k_c2, (uint32_t)(c->k_table.size() - 1), max_w).c2;
    }
    std::vector<float> kf(c->k_table.begin(), c->k_table.end());
    MRT_TRY(mrt::wait_stream(c, c->stream, "growing the K table"));
    mrt::free_device(c->d_k_f32, c->d_k_f64);
    c->k_len = 0;
    HIP_TRY(c, hipMalloc((void**)&c->d_k_f32, (size_t)cap * sizeof(float)));
    HIP_TRY(c, hipMalloc((void**)&c->d_k_f64, (size_t)cap * sizeof(double)));
    HIP_TRY(c, hipMemcpy(c->d_k_f32, kf.data(), (size_t)cap * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_k_f64, c->k_table.data(), (size_t)cap * sizeof(double), hipMemcpyHostToDevice));
    c->k_len = cap;
    return MRT_OK;
}

}  // namespace mrt

// ---- noise estimate (include/myraytracer_amd.h, "noise estimate") ----------------------------------------------------------
// While tracking is on, every blend also updates S (finalize_tracked_kernel, kernels.hip) and the host follows c2 (noise_c2).
// mrt_noise_query queues, on the ctx's stream right behind the most recent frame's blend, the reduction (noise.hip) into the
// ring entry's device sums and the copy of those 48 bytes into pinned host memory, and records the entry's event; nothing
// here waits for the frames in flight.  Ordering: S and the framebuffer the reduction reads are next written by blends queued
// after it on the same stream; the scratch and the tile map are written only by reductions, in stream order.
namespace {

using NoiseEntry = mrt_ctx::NoiseEntry;
constexpr uint32_t kNoiseRing = mrt_ctx::kNoiseRing;

// the ring's pinned sums, device sums and events, kept from the first enable to mrt_destroy
int ensure_noise_ring(mrt_ctx* c) {
    if (!c->d_noise_sums) HIP_TRY(c, hipMalloc((void**)&c->d_noise_sums, kNoiseRing * sizeof(mrt::NoiseSums)));
    if (!c->h_noise_sums) HIP_TRY(c, hipHostMalloc((void**)&c->h_noise_sums, kNoiseRing * sizeof(mrt::NoiseSums), hipHostMallocDefault));
    for (auto& E : c->noise_ring)
        if (!E.copied) HIP_TRY(c, hipEventCreateWithFlags(&E.copied, hipEventDisableTiming));
    return MRT_OK;
}

// the report of the sums and what the host knew at query time; K = +inf is "no estimate yet" (every derived figure +inf,
// without forming 0 * inf).  per_tile: reduced with K per tile (adaptive sampling), whose sum_s is sum_var already.
void noise_fill(mrt_noise_report* r, const mrt::NoiseSums& s, bool per_tile = false) {
    r->pixels = s.pixels; r->non_finite = s.non_finite; r->above = s.above;
    r->sum_lum = s.sum_l;
    if (std::isinf(r->noise_factor)) {
        r->sum_var = r->rmse = r->rel_rmse = INFINITY;
        r->max_se = INFINITY;
        return;
    }
    r->sum_var = per_tile ? s.sum_s : s.sum_s * r->noise_factor;
    r->max_se = s.max_se;
    r->rmse = s.pixels ? std::sqrt(r->sum_var / (double)s.pixels) : 0.0;
    r->rel_rmse = r->rmse > 0.0 ? r->rmse / (s.sum_l / (double)s.pixels) : 0.0;
}

bool noise_args_ok(float threshold, float floor_) { return std::isfinite(threshold) && std::isfinite(floor_) && floor_ >= 0.0f; }

// what an allocation on the device (mrt_noise_query_budget, mrt_debug_budget_plan) refuses before anything is allocated or grown;
// most: the largest n_t
int plan_ask_refusal(mrt_ctx* c, const char* who, uint32_t max_frames, uint32_t most) {
    if (max_frames < 1 || max_frames > mrt::kMaxFrameBatch)
        return fail(c, MRT_ERR_INVALID_ARG, "%s: max_frames %u (1 .. %u)", who, max_frames, mrt::kMaxFrameBatch);
    if (most > mrt::kBudgetMaxN) return fail(c, MRT_ERR_INVALID_ARG, "%s: a tile has more than %u frames", who, mrt::kBudgetMaxN);
    return MRT_OK;
}

}  // namespace

extern "C" {

double mrt_noise_factor(uint32_t frames_done, float max_w) {
    double c2 = 1.0;
    for (uint32_t k = 0; k < frames_done; k++) {
        const mrt::NoiseC2Step step = mrt::noise_c2_step(c2, k, max_w);
        if (step.fixed) break;
        c2 = step.c2;
    }
    return mrt::noise_factor_of(c2);
}

int mrt_set_noise_tracking(mrt_ctx* c, int enabled) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (c->frames_done != 0) return fail(c, MRT_ERR_STATE, "mrt_set_noise_tracking: frames already rendered; call mrt_reset first");
    HIP_TRY(c, hipSetDevice(c->device));
    if ((enabled != 0) == c->noise_on) return MRT_OK;
    MRT_TRY(mrt::wait_all(c, __func__));
    if (enabled) {
        MRT_TRY(ensure_noise_ring(c));
        MRT_TRY(alloc_noise_buffers(c));
        c->noise_on = true;
    } else {
        free_noise_buffers(c);
        c->noise_on = false;
        c->noise_first = c->noise_seq + 1;
    }
    return MRT_OK;
}

// mrt_noise_query and mrt_noise_query_map: map_kind 0 queues exactly what mrt_noise_query always has.  With `plan`
// (mrt_noise_query_budget: a summed-S query) the allocation of budget.hip is queued behind the reduction, ahead of the entry's
// copy and event, from n_t as the host knows it here: the device's at this point of the stream.
struct PlanAsk { uint64_t budget; uint32_t max_frames; };
static int noise_query(mrt_ctx* c, float threshold, float floor_, uint32_t map_kind, const PlanAsk* plan = nullptr) {
    if (!c || map_kind > MRT_TILE_MAP_SUM_S) return MRT_ERR_INVALID_ARG;
    if (!c->noise_on) return fail(c, MRT_ERR_STATE, "mrt_noise_query: noise tracking is off (mrt_set_noise_tracking)");
    if (!noise_args_ok(threshold, floor_))
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_noise_query: threshold %g, floor %g (finite, floor >= 0)", threshold, floor_);
    const uint32_t most = c->tiles_diverged ? mrt::most_tile_frames(c) : c->frames_done;       // the largest n_t
    if (plan) {
        MRT_TRY(plan_ask_refusal(c, "mrt_noise_query_budget", plan->max_frames, most));
        if (c->shard_world != 1) return fail(c, MRT_ERR_STATE, "mrt_noise_query_budget: a shard (world %u) has no budgets", c->shard_world);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const uint64_t seq = c->noise_seq + 1;
    const uint32_t i = (uint32_t)(seq % kNoiseRing);
    NoiseEntry& E = c->noise_ring[i];
    if (seq > kNoiseRing) {           // the ring is full when the entry's previous report is still in flight
        char what[96];
        std::snprintf(what, sizeof what, "mrt_noise_query: the ring is full (report %llu)", (unsigned long long)(seq - kNoiseRing));
        MRT_TRY(mrt::wait_event(c, E.copied, what));
    }
    float* map = c->d_noise_tiles + (size_t)i * mrt::tiles_min1(c);
    // the plan reads K up to the largest n_t + max_frames + 1 (the first such call may grow the table: the bounded wait of ensure_k_table)
    if (plan) MRT_TRY(mrt::ensure_k_table(c, most + plan->max_frames + 2u));
    double K = mrt::noise_factor_of(c->noise_c2);
    mrt::NoiseReduceArgs r{};
    r.S = c->d_noise_s; r.rgba = c->d_fb[c->target ^ 1];
    r.width = c->args.width; r.local_bands = c->local_bands; r.height = c->args.height;
    r.rank = c->shard_rank; r.world = c->shard_world;
    if (c->tiles_diverged) {        // adaptive sampling: K per tile; the report's K is the largest (the least-sampled tile's)
        MRT_TRY(mrt::ensure_k_table(c, most + 1u));
        K = 0.0;
        for (uint32_t t : c->tile_frames) K = std::max(K, c->k_table[t]);
        r.tile_frames = c->d_tile_frames; r.Kf = c->d_k_f32; r.Kd = c->d_k_f64;
    }
    r.K = (float)K;
    r.threshold = threshold; r.floor = floor_;
    r.map_kind = map_kind;
    r.partials = c->d_noise_partials; r.tiles = map; r.out = c->d_noise_sums + i;
    int e = mrt::launch_noise_reduce(r, c->stream);
    if (e) return fail(c, MRT_ERR_HIP, "noise reduction launch failed: %s", hipGetErrorString((hipError_t)e));
    E.has_plan = false;
    if (plan) {
        const mrt::BudgetLayout L = mrt::budget_layout(c->n_tiles, kNoiseRing);
        uint32_t* words = reinterpret_cast<uint32_t*>(c->d_noise_tiles);
        uint32_t* at = words + L.plan + (size_t)i * L.plan_stride;
        mrt::BudgetArgs a{};
        a.s = map;
        a.n = c->tiles_diverged ? c->d_tile_frames : nullptr;
        a.K = c->d_k_f64;
        a.n_uniform = c->frames_done; a.n_tiles = c->n_tiles; a.max_frames = plan->max_frames;
        a.budget = plan->budget;
        a.hist = words + L.hist;
        a.sums = reinterpret_cast<double*>(words + L.sums);
        a.res = reinterpret_cast<mrt_budget_result*>(at);
        a.k_out = at + sizeof(mrt_budget_result) / sizeof(uint32_t);
        e = mrt::launch_budget_plan(a, c->stream);
        if (e) return fail(c, MRT_ERR_HIP, "budget allocation launch failed: %s", hipGetErrorString((hipError_t)e));
    }
    HIP_TRY(c, hipMemcpyAsync(c->h_noise_sums + i, c->d_noise_sums + i, sizeof(mrt::NoiseSums), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(E.copied, c->stream));
    if (plan) {
        E.has_plan = true;
        E.nq_uniform = c->frames_done;
        if (c->tiles_diverged) E.nq = c->tile_frames;
        else E.nq.clear();
    }
    E.report = mrt_noise_report{};
    E.report.seq = seq;
    E.report.frames_done = c->frames_done;
    E.report.reserved = map_kind;
    E.report.threshold = threshold; E.report.floor = floor_;
    E.report.noise_factor = K;
    E.per_tile = c->tiles_diverged;
    c->noise_seq = seq;
    return MRT_OK;
}

int mrt_noise_query(mrt_ctx* c, float threshold, float floor_) { return noise_query(c, threshold, floor_, MRT_TILE_MAP_MAX_REL); }

int mrt_noise_query_map(mrt_ctx* c, float threshold, float floor_, uint32_t map_kind) { return noise_query(c, threshold, floor_, map_kind); }

int mrt_noise_query_budget(mrt_ctx* c, float threshold, float floor_, uint64_t budget, uint32_t max_frames) {
    const PlanAsk plan{budget, max_frames};
    return noise_query(c, threshold, floor_, MRT_TILE_MAP_SUM_S, &plan);
}

int mrt_noise_result(mrt_ctx* c, int wait, mrt_noise_report* out) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    *out = mrt_noise_report{};
    if (c->noise_seq < c->noise_first) return MRT_OK;                 // nothing queued (since the last reset)
    HIP_TRY(c, hipSetDevice(c->device));
    if (wait) {
        char what[96];
        std::snprintf(what, sizeof what, "mrt_noise_result: report %llu", (unsigned long long)c->noise_seq);
        MRT_TRY(mrt::wait_event(c, c->noise_ring[c->noise_seq % kNoiseRing].copied, what));
    }
    const uint64_t oldest = mrt::oldest_noise_report(c);
    for (uint64_t seq = c->noise_seq; seq >= oldest; seq--) {        // the newest whose copy has landed (stream order)
        const uint32_t i = (uint32_t)(seq % kNoiseRing);
        const hipError_t q = hipEventQuery(c->noise_ring[i].copied);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); continue; }
        if (q != hipSuccess) return fail(c, MRT_ERR_HIP, "mrt_noise_result: %s", hipGetErrorString(q));
        *out = c->noise_ring[i].report;
        noise_fill(out, c->h_noise_sums[i], c->noise_ring[i].per_tile);
        return MRT_OK;
    }
    return MRT_OK;
}

int mrt_read_noise(mrt_ctx* c, float* out, size_t cap) {
    if (!c || !out) return MRT_ERR_INVALID_ARG;
    if (!c->noise_on) return fail(c, MRT_ERR_STATE, "mrt_read_noise: noise tracking is off (mrt_set_noise_tracking)");
    HIP_TRY(c, hipSetDevice(c->device));
    return mrt::read_rows(c, __func__, c->d_noise_s, out, cap, sizeof(float));
}

int mrt_read_noise_tiles(mrt_ctx* c, float* out, size_t cap, uint32_t* tiles_x, uint32_t* tiles_rows) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (tiles_x) *tiles_x = c->tiles_x;
    if (tiles_rows) *tiles_rows = c->local_bands;
    if (!c->noise_on || c->noise_seq < c->noise_first)
        return fail(c, MRT_ERR_STATE, "mrt_read_noise_tiles: no noise query since tracking was enabled or the last reset");
    if (!out) return MRT_ERR_INVALID_ARG;
    const size_t n = c->n_tiles;
    if (cap < n) return fail(c, MRT_ERR_TOO_SMALL, "mrt_read_noise_tiles: need %zu floats", n);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->noise_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->noise_stream, hipStreamNonBlocking));
    // behind the latest query only: its copy's event, then the tile map on a stream of its own
    HIP_TRY(c, hipStreamWaitEvent(c->noise_stream, c->noise_ring[c->noise_seq % kNoiseRing].copied, 0));
    const float* map = c->d_noise_tiles + (size_t)(c->noise_seq % kNoiseRing) * n;
    if (n) HIP_TRY(c, hipMemcpyAsync(out, map, n * sizeof(float), hipMemcpyDeviceToHost, c->noise_stream));
    return mrt::wait_stream(c, c->noise_stream, __func__);
}

}  // extern "C"

namespace {

// The report a selection is made from (mrt_render_adaptive: kind MRT_TILE_MAP_MAX_REL, mrt_render_budget: MRT_TILE_MAP_SUM_S).
// report_seq == 0: the newest finished report of that kind, without waiting (*seq = 0: none); any other: that report, which must
// be held and of that kind, after a bounded wait on the host for its copy -- so *seq != 0 names a report whose `copied` the
// host has seen complete.
// plan: only a report that carries a budget plan (mrt_noise_query_budget) will do.
int choose_report(mrt_ctx* c, const char* who, uint64_t report_seq, uint32_t kind, uint64_t* seq, bool plan = false) {
    const uint64_t oldest = mrt::oldest_noise_report(c);
    *seq = 0;
    if (report_seq == 0) {
        for (uint64_t k = c->noise_seq; k >= oldest && k != 0; k--) {
            if (c->noise_ring[k % kNoiseRing].report.reserved != kind) continue;
            if (plan && !c->noise_ring[k % kNoiseRing].has_plan) continue;
            const hipError_t q = hipEventQuery(c->noise_ring[k % kNoiseRing].copied);
            if (q == hipErrorNotReady) { (void)hipGetLastError(); continue; }
            if (q != hipSuccess) return fail(c, MRT_ERR_HIP, "%s: %s", who, hipGetErrorString(q));
            *seq = k;
            break;
        }
        return MRT_OK;
    }
    if (report_seq > c->noise_seq || report_seq < oldest)
        return fail(c, MRT_ERR_STATE, "%s: report %llu is not among the reports held (%llu .. %llu)", who,
                    (unsigned long long)report_seq, (unsigned long long)oldest, (unsigned long long)c->noise_seq);
    if (c->noise_ring[report_seq % kNoiseRing].report.reserved != kind)
        return fail(c, MRT_ERR_STATE, "%s: report %llu holds a tile map of kind %u, not %u (mrt_noise_query_map)", who,
                    (unsigned long long)report_seq, c->noise_ring[report_seq % kNoiseRing].report.reserved, kind);
    if (plan && !c->noise_ring[report_seq % kNoiseRing].has_plan)
        return fail(c, MRT_ERR_STATE, "%s: report %llu carries no plan (mrt_noise_query_budget)", who, (unsigned long long)report_seq);
    char what[96];
    std::snprintf(what, sizeof what, "%s: report %llu", who, (unsigned long long)report_seq);
    MRT_TRY(mrt::wait_event(c, c->noise_ring[report_seq % kNoiseRing].copied, what));
    *seq = report_seq;
    return MRT_OK;
}

// `bytes` of what report `seq` (choose_report's: its copy has landed) left at `src` on the device -- its tile map, or its plan --
// into `dst`
int read_report_data(mrt_ctx* c, const char* who, uint64_t seq, const void* src, size_t bytes, void* dst) {
    // it was written before the report's copy: behind its event, on a stream of its own (the ctx's may hold frames)
    if (!c->noise_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->noise_stream, hipStreamNonBlocking));
    HIP_TRY(c, hipStreamWaitEvent(c->noise_stream, c->noise_ring[seq % kNoiseRing].copied, 0));
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->noise_stream));
    return mrt::wait_stream(c, c->noise_stream, who);
}

// report `seq`'s tile map into c->h_select_map
int read_report_map(mrt_ctx* c, const char* who, uint64_t seq, uint32_t nt) {
    c->h_select_map.resize(nt);
    return read_report_data(c, who, seq, c->d_noise_tiles + (size_t)(seq % kNoiseRing) * nt, (size_t)nt * sizeof(float), c->h_select_map.data());
}

// report `seq`'s plan as allocated (choose_report's, with a plan) into c->h_plan: the mrt_budget_result, then k_t per tile
// (k == null: the result alone, 64 bytes)
int read_report_plan(mrt_ctx* c, const char* who, uint64_t seq, uint32_t nt, mrt_budget_result* r, const uint32_t** k) {
    constexpr size_t head = sizeof(mrt_budget_result) / sizeof(uint32_t);
    const mrt::BudgetLayout L = mrt::budget_layout(nt, kNoiseRing);
    c->h_plan.resize(head + nt);
    const uint32_t* at = reinterpret_cast<const uint32_t*>(c->d_noise_tiles) + L.plan + (size_t)(seq % kNoiseRing) * L.plan_stride;
    MRT_TRY(read_report_data(c, who, seq, at, (head + (k ? nt : 0)) * sizeof(uint32_t), c->h_plan.data()));
    std::memcpy(r, c->h_plan.data(), sizeof *r);
    r->used_seq = seq;
    if (k) *k = c->h_plan.data() + head;
    return MRT_OK;
}

// L_j = {t : k_t >= j}, j = 1 .. frames (the largest k_t), in ascending tile id; consecutive j with the same list (the lists
// only shrink: the same size) are one mrt_render_tiles call
int render_levels(mrt_ctx* c, const uint32_t* k, uint32_t nt, uint32_t frames) {
    std::vector<uint32_t> listed(frames + 2u, 0u);          // listed[j] = |L_j|: a histogram of k, summed from the top
    for (uint32_t t = 0; t < nt; t++) listed[std::min(k[t], frames)]++;
    for (uint32_t j = frames; j-- > 0;) listed[j] += listed[j + 1];
    for (uint32_t j = 1; j <= frames;) {
        c->selection.clear();
        for (uint32_t t = 0; t < nt; t++)
            if (k[t] >= j) c->selection.push_back(t);
        uint32_t run = 1;
        while (j + run <= frames && listed[j + run] == listed[j]) run++;
        MRT_TRY(mrt_render_tiles(c, c->selection.data(), c->selection.size(), run));
        j += run;
    }
    return MRT_OK;
}

// mrt_render_tiles' refusals, for the callers that must refuse before anything is queued
int render_tiles_refusals(mrt_ctx* c, const char* who) {
    if (c->shard_world != 1) return fail(c, MRT_ERR_STATE, "%s: a shard (world %u) renders whole frames only", who, c->shard_world);
    if (!c->have_world) return fail(c, MRT_ERR_NO_SCENE, "%s: no scene (call mrt_set_world first)", who);
    if (c->locals.rng_mode == MRT_RNG_COUNTER && c->locals.samples_per_frame > MRT_COUNTER_BLOCK)
        return fail(c, MRT_ERR_INVALID_ARG, "%s: counter mode renders at most %u samples per frame by tiles (%u)", who,
                    (unsigned)MRT_COUNTER_BLOCK, c->locals.samples_per_frame);
    return MRT_OK;
}

// What mrt_render_budget, mrt_read_budget_plan and mrt_render_planned do first, in this order: *r zeroed with its size set and
// copied to *res, max_frames (where the call has one) in range, k_out's capacity, tracking on, for a call that renders
// mrt_render_tiles' refusals, k_out zeroed
int plan_call_opening(mrt_ctx* c, const char* who, const uint32_t* max_frames, bool renders, mrt_budget_result* r,
                      mrt_budget_result* res, uint32_t* k_out, size_t cap) {
    *r = mrt_budget_result{};
    r->size = sizeof *r;
    if (res) *res = *r;
    if (max_frames && (*max_frames < 1 || *max_frames > mrt::kMaxFrameBatch))
        return fail(c, MRT_ERR_INVALID_ARG, "%s: max_frames %u (1 .. %u)", who, *max_frames, mrt::kMaxFrameBatch);
    if (k_out && cap < c->n_tiles) return fail(c, MRT_ERR_TOO_SMALL, "%s: need %u values", who, c->n_tiles);
    if (!c->noise_on) return fail(c, MRT_ERR_STATE, "%s: noise tracking is off (mrt_set_noise_tracking)", who);
    if (renders) MRT_TRY(render_tiles_refusals(c, who));
    if (k_out) std::fill(k_out, k_out + c->n_tiles, 0u);
    return MRT_OK;
}

}  // namespace

extern "C" {

// Adaptive sampling's selection: the tiles whose entry in report `report_seq`'s tile map is > its threshold (the tiles holding a
// pixel counted in its `above`), from that report's own map (one per ring entry), then mrt_render_tiles.  Waits for that query only.
int mrt_render_adaptive(mrt_ctx* c, uint32_t frames, uint64_t report_seq, uint64_t* used_seq, uint32_t* tiles_selected) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (used_seq) *used_seq = 0;
    if (tiles_selected) *tiles_selected = 0;
    if (!c->noise_on) return fail(c, MRT_ERR_STATE, "mrt_render_adaptive: noise tracking is off (mrt_set_noise_tracking)");
    HIP_TRY(c, hipSetDevice(c->device));
    uint64_t seq = 0;                           // report_seq 0 and none finished: every tile
    MRT_TRY(choose_report(c, __func__, report_seq, MRT_TILE_MAP_MAX_REL, &seq));
    const uint32_t nt = c->n_tiles;
    c->selection.clear();
    if (seq == 0) {
        for (uint32_t t = 0; t < nt; t++) c->selection.push_back(t);
    } else {
        MRT_TRY(read_report_map(c, __func__, seq, nt));
        const float threshold = c->noise_ring[seq % kNoiseRing].report.threshold;
        for (uint32_t t = 0; t < nt; t++)
            if (c->h_select_map[t] > threshold) c->selection.push_back(t);
    }
    if (used_seq) *used_seq = seq;
    if (tiles_selected) *tiles_selected = (uint32_t)c->selection.size();
    if (c->selection.empty()) return MRT_OK;              // converged at that threshold: nothing to render
    return mrt_render_tiles(c, c->selection.data(), c->selection.size(), frames);
}

// Adaptive sampling by budget (include/myraytracer_amd.h): the definition there, as a selection over the candidates.  K(n) comes
// from one table made by mrt_noise_factor's own recursion (the values are its, bit for bit); the table ends where c2 has
// reached its fixed point at a saturated weight, as mrt_noise_factor's loop does, and K is constant from there.
int mrt_budget_allocate(const float* s, const uint32_t* n, size_t tiles, float max_w, uint64_t budget, uint32_t max_frames,
                        uint32_t* k_out, mrt_budget_result* res) {
    if (!s || !n || !k_out || !res || tiles == 0 || max_frames < 1 || max_frames > mrt::kMaxFrameBatch) return MRT_ERR_INVALID_ARG;
    if (!(max_w > 0.0f) || std::isinf(max_w)) return MRT_ERR_INVALID_ARG;
    uint32_t most = 0;
    for (size_t t = 0; t < tiles; t++) {
        if (n[t] > mrt::kBudgetMaxN) return MRT_ERR_INVALID_ARG;
        most = std::max(most, n[t]);
    }
    std::vector<double> table;
    mrt::NoiseC2Step at{1.0, false};
    for (uint32_t k = 0; k < most + max_frames + 1u && !at.fixed; k++) {
        table.push_back(mrt::noise_factor_of(at.c2));           // K(k)
        at = mrt::noise_c2_step(at.c2, k, max_w);
    }
    const auto K = [&](uint32_t frames) { return table[std::min<size_t>(frames, table.size() - 1)]; };
    const auto clean = [&](size_t t) { return s[t] >= 0.0f ? (double)s[t] : 0.0; };      // (a NaN compares false)
    std::fill(k_out, k_out + tiles, 0u);
    uint64_t left = budget;
    // mandatory frames: j ascending, then t ascending
    for (uint32_t j = 0; j < std::min(2u, max_frames) && left != 0; j++)
        for (size_t t = 0; t < tiles && left != 0; t++)
            if (n[t] + j < 2u) { k_out[t]++; left--; }
    if (left != 0) {
        struct Cand { double g; uint32_t j, t; };
        const auto before = [](const Cand& a, const Cand& b) { return a.g != b.g ? a.g > b.g : a.j != b.j ? a.j < b.j : a.t < b.t; };
        std::vector<Cand> cand;
        cand.reserve(std::min<size_t>(tiles * max_frames, 1u << 22));
        std::vector<double> step(table.size());                 // K(n) - K(n + 1); 0 from the table's end on, where K stays
        for (size_t i = 0; i + 1 < table.size(); i++) step[i] = table[i] - table[i + 1];
        const auto gain = [&](uint32_t frames) { return frames < step.size() ? step[frames] : 0.0; };
        for (size_t t = 0; t < tiles; t++) {
            const double st = clean(t);
            const uint32_t m = n[t] < 2u ? std::min(2u - n[t], max_frames) : 0u;
            if (!(st > 0.0) || std::isinf(st) || n[t] + m < 2u) continue;
            double g = INFINITY;
            for (uint32_t j = m; j < max_frames; j++) {
                g = std::min(g, st * gain(n[t] + j));
                if (!(g > 0.0)) break;                          // g' never increases: no later candidate counts
                cand.push_back(Cand{g, j, (uint32_t)t});
            }
        }
        if (left < cand.size()) {
            std::nth_element(cand.begin(), cand.begin() + (ptrdiff_t)left, cand.end(), before);
            cand.resize((size_t)left);
        }
        for (const Cand& q : cand) k_out[q.t]++;
    }
    mrt_budget_result r{};
    r.size = sizeof r;
    for (size_t t = 0; t < tiles; t++) {
        r.tile_frames += k_out[t];
        r.tiles += k_out[t] ? 1u : 0u;
        r.frames = std::max(r.frames, k_out[t]);
        if (n[t] >= 2u) {
            r.var_before += clean(t) * K(n[t]);
            r.var_after += clean(t) * K(n[t] + k_out[t]);
        }
    }
    *res = r;
    return MRT_OK;
}

int mrt_render_budget(mrt_ctx* c, uint64_t budget, uint32_t max_frames, uint64_t report_seq, mrt_budget_result* res, uint32_t* k_out,
                      size_t cap) {
    if (!c) return MRT_ERR_INVALID_ARG;
    mrt_budget_result r;
    MRT_TRY(plan_call_opening(c, __func__, &max_frames, true, &r, res, k_out, cap));
    const uint32_t nt = c->n_tiles;
    HIP_TRY(c, hipSetDevice(c->device));
    uint64_t seq = 0;
    MRT_TRY(choose_report(c, __func__, report_seq, MRT_TILE_MAP_SUM_S, &seq));
    if (seq == 0 || nt == 0) return MRT_OK;               // no report of that kind has finished: nothing to allocate from
    r.used_seq = seq;
    if (res) *res = r;
    if (budget == 0) return MRT_OK;
    MRT_TRY(read_report_map(c, __func__, seq, nt));
    std::vector<uint32_t> uniform;
    if (!c->tiles_diverged) uniform.assign(nt, c->frames_done);
    const uint32_t* n = c->tiles_diverged ? c->tile_frames.data() : uniform.data();
    std::vector<uint32_t> k(nt);
    if (mrt_budget_allocate(c->h_select_map.data(), n, nt, c->args.max_framebuffer_weight, budget, max_frames, k.data(), &r) != MRT_OK)
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_render_budget: a tile has more than %u frames", mrt::kBudgetMaxN);
    r.used_seq = seq;
    if (res) *res = r;
    if (k_out) std::copy(k.begin(), k.end(), k_out);
    return render_levels(c, k.data(), nt, r.frames);
}

int mrt_read_budget_plan(mrt_ctx* c, uint64_t report_seq, uint32_t* k_out, size_t cap, mrt_budget_result* res) {
    if (!c) return MRT_ERR_INVALID_ARG;
    mrt_budget_result r;
    MRT_TRY(plan_call_opening(c, __func__, nullptr, false, &r, res, k_out, cap));
    const uint32_t nt = c->n_tiles;
    HIP_TRY(c, hipSetDevice(c->device));
    uint64_t seq = 0;
    MRT_TRY(choose_report(c, __func__, report_seq, MRT_TILE_MAP_SUM_S, &seq, true));
    if (seq == 0 || nt == 0) return MRT_OK;               // no report with a plan has finished
    const uint32_t* k = nullptr;
    MRT_TRY(read_report_plan(c, __func__, seq, nt, &r, k_out ? &k : nullptr));
    if (res) *res = r;
    if (k_out) std::copy(k, k + nt, k_out);
    return MRT_OK;
}

int mrt_render_planned(mrt_ctx* c, uint64_t report_seq, mrt_budget_result* res, uint32_t* k_out, size_t cap) {
    if (!c) return MRT_ERR_INVALID_ARG;
    mrt_budget_result r;
    MRT_TRY(plan_call_opening(c, __func__, nullptr, true, &r, res, k_out, cap));
    const uint32_t nt = c->n_tiles;
    HIP_TRY(c, hipSetDevice(c->device));
    uint64_t seq = 0;
    MRT_TRY(choose_report(c, __func__, report_seq, MRT_TILE_MAP_SUM_S, &seq, true));
    if (seq == 0 || nt == 0) return MRT_OK;               // no report with a plan has finished: nothing to render
    const uint32_t* k = nullptr;
    MRT_TRY(read_report_plan(c, __func__, seq, nt, &r, &k));
    // the plan is a target: tile t should reach n_q[t] + k_t frames, and the frames queued since the query count towards it
    const NoiseEntry& E = c->noise_ring[seq % kNoiseRing];
    std::vector<uint32_t> left(nt);
    r.tile_frames = 0; r.tiles = 0; r.frames = 0;
    for (uint32_t t = 0; t < nt; t++) {
        const uint64_t target = (uint64_t)(E.nq.empty() ? E.nq_uniform : E.nq[t]) + k[t];
        const uint64_t now = c->tiles_diverged ? c->tile_frames[t] : c->frames_done;
        left[t] = target > now ? (uint32_t)(target - now) : 0u;
        r.tile_frames += left[t];
        r.tiles += left[t] ? 1u : 0u;
        r.frames = std::max(r.frames, left[t]);
    }
    if (res) *res = r;
    if (k_out) std::copy(left.begin(), left.end(), k_out);
    return render_levels(c, left.data(), nt, r.frames);
}

int mrt_debug_noise_reduce(mrt_ctx* c, const float* S, const float* rgba, uint32_t width, uint32_t rows, double K,
                           float threshold, float floor_, mrt_noise_report* out, float* tiles_out) {
    if (!c || !S || !rgba || !out || !width || !rows || (uint64_t)width * rows > (1ull << 28) || !noise_args_ok(threshold, floor_) ||
        std::isnan(K) || K < 0.0)
        return MRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)width * rows;
    const uint32_t bands = (rows + mrt::kBandRows - 1) / mrt::kBandRows, tx = (width + mrt::kTileW - 1) / mrt::kTileW;
    const size_t tiles = (size_t)bands * tx;
    float *d_s = nullptr, *d_rgba = nullptr, *d_tiles = nullptr;
    void* d_part = nullptr;
    mrt::NoiseSums* d_sums = nullptr;
    mrt::NoiseSums h{};
    hipError_t e = hipSuccess;
    const char* what = "mrt_debug_noise_reduce";
    HIP_CHAIN(e, what, hipMalloc((void**)&d_s, n * sizeof(float)));
    HIP_CHAIN(e, what, hipMalloc((void**)&d_rgba, n * 16));
    HIP_CHAIN(e, what, hipMalloc((void**)&d_tiles, tiles * sizeof(float)));
    HIP_CHAIN(e, what, hipMalloc(&d_part, mrt::noise_partials_bytes(width, bands)));
    HIP_CHAIN(e, what, hipMalloc((void**)&d_sums, sizeof h));
    if (e == hipSuccess) e = hipMemcpyAsync(d_s, S, n * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rgba, rgba, n * 16, hipMemcpyHostToDevice, c->stream);
    mrt::NoiseReduceArgs r{};
    r.S = d_s; r.rgba = d_rgba;
    r.width = width; r.local_bands = bands; r.height = rows;
    r.rank = 0; r.world = 1;
    r.K = (float)K;
    r.threshold = threshold; r.floor = floor_;
    r.map_kind = MRT_TILE_MAP_MAX_REL;
    r.partials = d_part; r.tiles = d_tiles; r.out = d_sums;
    if (e == hipSuccess) e = (hipError_t)mrt::launch_noise_reduce(r, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d_sums, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && tiles_out) e = hipMemcpyAsync(tiles_out, d_tiles, tiles * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    int ws = MRT_OK;
    if (e == hipSuccess) ws = mrt::wait_stream(c, c->stream, "mrt_debug_noise_reduce");
    if (ws != MRT_OK) return ws;            // (stalled: the buffers are left to the process)
    mrt::free_device(d_s, d_rgba, d_tiles, d_part, d_sums);
    if (e != hipSuccess) return fail(c, MRT_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    *out = mrt_noise_report{};
    out->threshold = threshold; out->floor = floor_;
    out->noise_factor = K;
    noise_fill(out, h);
    return MRT_OK;
}

int mrt_debug_budget_plan(mrt_ctx* c, const float* s, const uint32_t* n, uint32_t n_uniform, size_t tiles, uint64_t budget,
                          uint32_t max_frames, uint32_t* k_out, mrt_budget_result* res) {
    if (!c || !s || !k_out || !res || tiles == 0 || tiles > (1ull << 28)) return MRT_ERR_INVALID_ARG;
    uint32_t most = n ? 0u : n_uniform;
    for (size_t t = 0; n && t < tiles; t++) most = std::max(most, n[t]);
    MRT_TRY(plan_ask_refusal(c, __func__, max_frames, most));
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(mrt::ensure_k_table(c, most + max_frames + 2u));
    // one entry's layout: the map (s), its plan, the selection's scratch
    constexpr size_t head = sizeof(mrt_budget_result) / sizeof(uint32_t);
    const mrt::BudgetLayout L = mrt::budget_layout(tiles, 1);
    uint32_t *d_plan_words = nullptr, *d_plan_n = nullptr;
    std::vector<uint32_t> h(head + tiles);
    hipError_t e = hipSuccess;
    const char* what = "mrt_debug_budget_plan";
    HIP_CHAIN(e, what, hipMalloc((void**)&d_plan_words, L.words * sizeof(uint32_t)));
    if (n) HIP_CHAIN(e, what, hipMalloc((void**)&d_plan_n, tiles * sizeof(uint32_t)));
    if (e == hipSuccess) e = hipMemcpyAsync(d_plan_words, s, tiles * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(d_plan_n, n, tiles * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    mrt::BudgetArgs a{};
    if (e == hipSuccess) {
        a.s = reinterpret_cast<const float*>(d_plan_words);
        a.n = d_plan_n;
        a.K = c->d_k_f64;
        a.n_uniform = n_uniform; a.n_tiles = (uint32_t)tiles; a.max_frames = max_frames;
        a.budget = budget;
        a.hist = d_plan_words + L.hist;
        a.sums = reinterpret_cast<double*>(d_plan_words + L.sums);
        a.res = reinterpret_cast<mrt_budget_result*>(d_plan_words + L.plan);
        a.k_out = d_plan_words + L.plan + head;
        e = (hipError_t)mrt::launch_budget_plan(a, c->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d_plan_words + L.plan, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    int ws = MRT_OK;
    if (e == hipSuccess) ws = mrt::wait_stream(c, c->stream, "mrt_debug_budget_plan");
    if (ws != MRT_OK) return ws;            // (stalled: the buffers are left to the process)
    mrt::free_device(d_plan_words, d_plan_n);
    if (e != hipSuccess) return fail(c, MRT_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    std::memcpy(res, h.data(), sizeof *res);
    std::copy(h.begin() + head, h.end(), k_out);
    return MRT_OK;
}

}  // extern "C"
