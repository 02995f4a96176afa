// The present pass of include/myraytracer_amd.h: mrt_present and its ring of images.
#include <algorithm>
#include <cstdio>

#include "mrt_ctx.h"

using mrt::fail, mrt::ImageSource, mrt::local_texels;

// ---- present pass (include/myraytracer_amd.h, "present pass") -------------------------------------------------------------
// mrt_present queues, on the ctx's stream right behind the most recent frame's blend, the present kernel (present.hip) into a
// ring entry's device buffer and then the copy of that buffer into the entry's pinned host buffer (on a stream of its own, or
// on the ctx's stream: mrt_debug_set_present_copy), and records the entry's event.  Nothing here waits for the ctx's stream or
// the side streams, so the frames in flight stay in flight.  Ordering: the framebuffer the kernel reads is next overwritten two
// blends later on the same stream; a gathered frame (d_gather) is next overwritten by copies that wait for everything queued on
// the root's stream before that gather (ev_gather_root, multi_gpu.cpp); an entry is reused only once its copy has landed.
namespace {

using PresentEntry = mrt_ctx::PresentEntry;
constexpr size_t kPresentPinnedBudget = 256000000;             // pinned bytes of all of a ring's entries together
constexpr uint32_t kPresentMaxDepth = mrt_ctx::kMaxFrameSlots + 2;

int ensure_present_tables(mrt_ctx* c) {
    if (c->d_present_tables) return MRT_OK;
    float* d = nullptr;
    HIP_TRY(c, hipMalloc((void**)&d, 512 * sizeof(float)));
    const hipError_t e = hipMemcpyAsync(d, mrt::present_thresholds(), 512 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { (void)hipFree(d); return fail(c, MRT_ERR_HIP, "present tables upload failed: %s", hipGetErrorString(e)); }
    c->d_present_tables = d;
    return MRT_OK;
}

bool present_copy_landed(const PresentEntry& E) { return hipEventQuery(E.copied) == hipSuccess; }

int present_wait(mrt_ctx* c, const PresentEntry& E, const char* who) {
    char what[160];
    std::snprintf(what, sizeof what, "%s: the copy of present %llu", who, (unsigned long long)E.info.seq);
    return mrt::wait_event(c, E.copied, what);
}

// the images not yet acquired are dropped once their copies have landed (bounded wait)
int present_discard_queued(mrt_ctx* c, const char* who) {
    for (auto& E : c->present_ring) {
        if (E.state != PresentEntry::kQueued) continue;
        MRT_TRY(present_wait(c, E, who));
        E.state = PresentEntry::kFree;
    }
    c->present_dropped = 0;
    return MRT_OK;
}

// the depth the next present uses: pinned, or the frames in flight + 2 (never less than before); held to the pinned-memory budget
uint32_t present_depth_for(const mrt_ctx* c) {
    uint32_t fif = c->frame_slots;
    if (c->width.s.div) fif = std::max(fif, c->width.frames_in_flight());
    uint32_t want = c->present_depth_pin ? c->present_depth_pin : std::max(c->present_depth, fif + 2u);
    const size_t cap = std::max<size_t>(2, kPresentPinnedBudget / std::max<size_t>(c->present_entry_bytes, 1));
    return (uint32_t)std::min<size_t>({(size_t)want, cap, (size_t)kPresentMaxDepth});
}

// entries of `bytes` each, at least `depth` of them: added without synchronising anything (hipMalloc, hipHostMalloc); entries
// too small for `bytes` are released first, after their copies have landed (a larger source or a wider format than before:
// rare; the queued images are discarded and counted as dropped, MRT_ERR_STATE while the caller holds one).  Entries are never
// shrunk: they fit the largest image presented so far, whatever its format
int present_ring_reserve(mrt_ctx* c, size_t bytes, uint32_t depth) {
    if (bytes > c->present_entry_bytes) {
        for (const auto& E : c->present_ring)
            if (E.state == PresentEntry::kHeld)
                return fail(c, MRT_ERR_STATE, "mrt_present: the image (%zu bytes) outgrows the ring's entries; release the held one first", bytes);
        const uint32_t dropped = c->present_dropped + (uint32_t)std::count_if(c->present_ring.begin(), c->present_ring.end(),
                                                        [](const PresentEntry& E) { return E.state == PresentEntry::kQueued; });
        MRT_TRY(present_discard_queued(c, "mrt_present (regrowing the ring)"));
        c->present_dropped = dropped;
        for (auto& E : c->present_ring) {
            (void)hipFree(E.d_img); (void)hipHostFree(E.h_img); (void)hipEventDestroy(E.copied);
        }
        c->present_ring.clear();
        c->present_entry_bytes = bytes;
        c->present_depth = 0;
        depth = present_depth_for(c);
    }
    while (c->present_ring.size() < depth) {
        c->present_ring.emplace_back();
        PresentEntry& E = c->present_ring.back();
        hipError_t e = hipSuccess;
        const char* what = "";
        HIP_CHAIN(e, what, hipMalloc((void**)&E.d_img, c->present_entry_bytes));
        HIP_CHAIN(e, what, hipHostMalloc((void**)&E.h_img, c->present_entry_bytes, hipHostMallocDefault));
        HIP_CHAIN(e, what, hipEventCreateWithFlags(&E.copied, hipEventDisableTiming));
        if (e != hipSuccess) {
            if (E.d_img) (void)hipFree(E.d_img);
            if (E.h_img) (void)hipHostFree(E.h_img);
            c->present_ring.pop_back();
            return fail(c, MRT_ERR_HIP, "mrt_present: ring entry %zu (%zu bytes): %s failed: %s", c->present_ring.size(),
                        c->present_entry_bytes, what, hipGetErrorString(e));
        }
    }
    c->present_depth = depth;
    return MRT_OK;
}

// an entry for the next present: a free one, else the oldest whose image has landed unacquired (dropped), else -- every other
// entry's copy is in flight -- the oldest, after a bounded wait on the host
int present_pick(mrt_ctx* c, uint32_t* out) {
    int done = -1, busy = -1;
    for (uint32_t i = 0; i < c->present_depth; i++) {
        const PresentEntry& E = c->present_ring[i];
        if (E.state == PresentEntry::kFree) { *out = i; return MRT_OK; }
        if (E.state != PresentEntry::kQueued) continue;
        int& best = present_copy_landed(E) ? done : busy;
        if (best < 0 || E.info.seq < c->present_ring[best].info.seq) best = (int)i;
    }
    (void)hipGetLastError();        // (hipEventQuery's hipErrorNotReady is not an error)
    if (done < 0 && busy < 0) return fail(c, MRT_ERR_STATE, "mrt_present: no ring entry the caller does not hold");
    if (done < 0) {
        MRT_TRY(present_wait(c, c->present_ring[busy], "mrt_present: the ring is full"));
        done = busy;
    }
    c->present_dropped++;
    *out = (uint32_t)done;
    return MRT_OK;
}

bool present_format_8bit(int format) { return format == MRT_PRESENT_RGBA8_SRGB || format == MRT_PRESENT_BGRA8_SRGB; }

// bytes per pixel of a present format; 0: no such format
uint32_t present_pixel_bytes(int format) {
    if (present_format_8bit(format)) return 4;
    return format == MRT_PRESENT_RGBA16F_LINEAR ? 8u : format == MRT_PRESENT_RGBA32F_LINEAR ? 16u : 0u;
}

// The source a flag word names (FLIP_Y is no source).  The rule is "at most one source bit", and the table's order gives the
// refusals: of a word with several, the second in this order is refused, with that source's own reason why it is none of those
// before it.  A new source is one more row and one more reason.
int source_of_flags(mrt_ctx* c, uint32_t flags, ImageSource* out) {
    static constexpr struct { uint32_t bit; ImageSource source; } kSources[] = {
        {MRT_PRESENT_GATHERED, ImageSource::Gathered}, {MRT_PRESENT_DENOISED, ImageSource::Denoised},
        {MRT_PRESENT_TEMPORAL, ImageSource::Temporal}, {MRT_PRESENT_GATHERED_DENOISED, ImageSource::GatheredDenoised},
        {MRT_PRESENT_VIEW, ImageSource::View}};
    uint32_t known = MRT_PRESENT_FLIP_Y;
    for (const auto& s : kSources) known |= s.bit;
    if (flags & ~known) return fail(c, MRT_ERR_INVALID_ARG, "mrt_present: flags 0x%x", flags);
    *out = ImageSource::Accumulated;
    for (const auto& s : kSources) {
        if (!(flags & s.bit)) continue;
        if (*out == ImageSource::Accumulated) { *out = s.source; continue; }
        if (s.source == ImageSource::Denoised) return fail(c, MRT_ERR_INVALID_ARG, "mrt_present: the gathered frame cannot be denoised (it has no S)");
        if (s.source == ImageSource::Temporal) return fail(c, MRT_ERR_INVALID_ARG, "mrt_present: the temporal image is neither the gathered nor the denoised frame (flags 0x%x)", flags);
        if (s.source == ImageSource::View) return fail(c, MRT_ERR_INVALID_ARG, "mrt_present: a view is computed from the accumulation, not from another source (flags 0x%x: with FLIP_Y only)", flags);
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_present: the denoised gathered frame is a source of its own (flags 0x%x: with FLIP_Y only)", flags);
    }
    return MRT_OK;
}

}  // namespace

extern "C" {

int mrt_present(mrt_ctx* c, int format, uint32_t flags) {
    if (!c) return MRT_ERR_INVALID_ARG;
    const uint32_t pixel_bytes = present_pixel_bytes(format);
    if (!pixel_bytes) return fail(c, MRT_ERR_INVALID_ARG, "mrt_present: format %d", format);
    ImageSource source;
    MRT_TRY(source_of_flags(c, flags, &source));
    MRT_TRY(mrt::source_check(c, source, "mrt_present"));
    // (the one refusal of a source that stays here: it is FLIP_Y's, and source_check sees the state alone, not the flags)
    if (source == ImageSource::Accumulated && c->shard_world > 1 && (flags & MRT_PRESENT_FLIP_Y))
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_present: a shard's packed rows cannot be flipped (gather them first)");
    const uint32_t width = c->args.width, rows = mrt::source_rows(c, source);
    // (an image larger than the ring's entries -- a larger source, or a wider format than any presented so far -- regrows them)
    const size_t bytes = (size_t)rows * width * pixel_bytes;
    if (bytes == 0) return fail(c, MRT_ERR_STATE, "mrt_present: empty image");
    HIP_TRY(c, hipSetDevice(c->device));
    if (pixel_bytes == 4) MRT_TRY(ensure_present_tables(c));        // (the linear formats search no table)
    MRT_TRY(present_ring_reserve(c, bytes, present_depth_for(c)));
    uint32_t i = 0;
    MRT_TRY(present_pick(c, &i));
    PresentEntry& E = c->present_ring[i];
    E.state = PresentEntry::kFree;
    mrt::SourceImage S;
    MRT_TRY(mrt::source_queue(c, source, &S));
    const uint32_t flip = (flags & MRT_PRESENT_FLIP_Y) ? 1u : 0u;
    const int e = pixel_bytes == 4 ? mrt::launch_present(S.img, E.d_img, width, rows, flip, format == MRT_PRESENT_BGRA8_SRGB ? 1u : 0u,
                                                         c->d_present_tables, c->stream)
                                   : mrt::launch_present_float(S.img, E.d_img, width, rows, flip, pixel_bytes == 8 ? 1u : 0u, c->stream);
    if (e) return fail(c, MRT_ERR_HIP, "present launch failed: %s", hipGetErrorString((hipError_t)e));
    hipStream_t copy_stream = c->stream;
    if (c->present_copy_mode == 0) {
        // (each unless an earlier, refused attempt already left it)
        if (!c->ev_presented) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_presented, hipEventDisableTiming));
        if (!c->present_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->present_stream, hipStreamNonBlocking));
        HIP_TRY(c, hipEventRecord(c->ev_presented, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->present_stream, c->ev_presented, 0));
        copy_stream = c->present_stream;
    }
    HIP_TRY(c, hipMemcpyAsync(E.h_img, E.d_img, bytes, hipMemcpyDeviceToHost, copy_stream));
    HIP_TRY(c, hipEventRecord(E.copied, copy_stream));
    E.info = mrt_present_info{};
    E.info.seq = ++c->present_seq;
    E.info.frames_done = S.frames_done;
    E.info.width = width; E.info.rows = rows; E.info.row_bytes = width * pixel_bytes;
    E.info.format = (uint32_t)format; E.info.flags = flags;
    E.state = PresentEntry::kQueued;
    return MRT_OK;
}

int mrt_present_acquire(mrt_ctx* c, int mode, int wait, const uint8_t** pixels, mrt_present_info* info) {
    if (!c || !pixels) return MRT_ERR_INVALID_ARG;
    *pixels = nullptr;
    if (mode != MRT_ACQUIRE_NEWEST && mode != MRT_ACQUIRE_OLDEST) return fail(c, MRT_ERR_INVALID_ARG, "mrt_present_acquire: mode %d", mode);
    if (c->present_seq == 0) return fail(c, MRT_ERR_STATE, "mrt_present_acquire: nothing presented yet (mrt_present)");
    HIP_TRY(c, hipSetDevice(c->device));
    for (auto& E : c->present_ring)
        if (E.state == PresentEntry::kHeld) E.state = PresentEntry::kFree;        // (the image held before is released)
    const bool newest = mode == MRT_ACQUIRE_NEWEST;
    int pick = -1;
    for (;;) {
        int oldest = -1, latest = -1, latest_done = -1;
        bool oldest_done = false;
        for (uint32_t i = 0; i < c->present_ring.size(); i++) {
            const PresentEntry& E = c->present_ring[i];
            if (E.state != PresentEntry::kQueued) continue;
            const bool done = present_copy_landed(E);
            if (oldest < 0 || E.info.seq < c->present_ring[oldest].info.seq) { oldest = (int)i; oldest_done = done; }
            if (latest < 0 || E.info.seq > c->present_ring[latest].info.seq) latest = (int)i;
            if (done && (latest_done < 0 || E.info.seq > c->present_ring[latest_done].info.seq)) latest_done = (int)i;
        }
        (void)hipGetLastError();
        pick = newest ? latest_done : (oldest_done ? oldest : -1);
        if (pick >= 0 || !wait || oldest < 0) break;
        MRT_TRY(present_wait(c, c->present_ring[newest ? latest : oldest], "mrt_present_acquire"));
    }
    if (pick < 0) return MRT_OK;
    PresentEntry& P = c->present_ring[pick];
    if (newest)           // mailbox: the older images that have landed are skipped
        for (auto& E : c->present_ring)
            if (E.state == PresentEntry::kQueued && E.info.seq < P.info.seq && present_copy_landed(E)) {
                E.state = PresentEntry::kFree;
                c->present_dropped++;
            }
    (void)hipGetLastError();
    P.state = PresentEntry::kHeld;
    if (info) {
        *info = P.info;
        info->dropped = c->present_dropped;
        info->ring_depth = c->present_depth;
    }
    c->present_dropped = 0;
    *pixels = P.h_img;
    return MRT_OK;
}

int mrt_present_release(mrt_ctx* c) {
    if (!c) return MRT_ERR_INVALID_ARG;
    for (auto& E : c->present_ring)
        if (E.state == PresentEntry::kHeld) { E.state = PresentEntry::kFree; return MRT_OK; }
    return fail(c, MRT_ERR_STATE, "mrt_present_release: no image is held (mrt_present_acquire)");
}

int mrt_set_present_ring(mrt_ctx* c, uint32_t depth) {
    if (!c) return MRT_ERR_INVALID_ARG;
    if (depth != 0 && (depth < 2 || depth > kPresentMaxDepth))
        return fail(c, MRT_ERR_INVALID_ARG, "mrt_set_present_ring: depth %u (2..%u, or 0 = automatic)", depth, kPresentMaxDepth);
    for (const auto& E : c->present_ring)
        if (E.state == PresentEntry::kHeld) return fail(c, MRT_ERR_STATE, "mrt_set_present_ring: an image is held (mrt_present_release)");
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(present_discard_queued(c, "mrt_set_present_ring"));
    c->present_depth_pin = depth;
    c->present_depth = 0;                  // (the next present sets it; the entries already allocated are kept)
    return MRT_OK;
}

int mrt_debug_set_present_copy(mrt_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 1) return MRT_ERR_INVALID_ARG;
    c->present_copy_mode = mode;
    return MRT_OK;
}

int mrt_debug_present_encode(mrt_ctx* c, const float* rgba, uint32_t width, uint32_t rows, int format, uint32_t flags,
                             uint8_t* out) {
    if (!c || !rgba || !out || !width || !rows || !present_format_8bit(format) || (flags & ~(uint32_t)MRT_PRESENT_FLIP_Y) ||
        (uint64_t)width * rows > (1ull << 28))
        return MRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    MRT_TRY(ensure_present_tables(c));
    const size_t n = (size_t)width * rows;
    float* d_in = nullptr;
    uint8_t* d_out = nullptr;
    HIP_TRY(c, hipMalloc((void**)&d_in, n * 16));
    hipError_t e = hipSuccess;
    const char* what = "mrt_debug_present_encode";
    HIP_CHAIN(e, what, hipMalloc((void**)&d_out, n * 4));
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, rgba, n * 16, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = (hipError_t)mrt::launch_present(d_in, d_out, width, rows, (flags & MRT_PRESENT_FLIP_Y) ? 1u : 0u,
                                            format == MRT_PRESENT_BGRA8_SRGB ? 1u : 0u, c->d_present_tables, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n * 4, hipMemcpyDeviceToHost, c->stream);
    int ws = MRT_OK;
    if (e == hipSuccess) ws = mrt::wait_stream(c, c->stream, "mrt_debug_present_encode");
    if (ws != MRT_OK) return ws;            // (stalled: the buffers are left to the process)
    (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (e != hipSuccess) return fail(c, MRT_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    return MRT_OK;
}

}  // extern "C"
