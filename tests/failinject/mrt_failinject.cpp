// The failure-injection shim behind mrt_failinject.h: counts the library's creator calls and refuses the armed one without
// calling the runtime, counts its stream waits and drops the chosen one, keeps the live device / pinned allocations, streams and events, withholds releases of what is not live
// and copies / memsets that leave the live device allocations, and reports all of it to the tests.  Host code only; the one
// thing it needs from HIP are the functions it forwards to (tests/test_failinject_shim.py links it against a stand-in).
#define MRT_FAILINJECT_SHIM
#include "mrt_failinject.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

namespace {

struct Shim {
    std::mutex mu;
    uint64_t calls = 0, armed = 0;
    bool fired = false;
    std::string fired_site;
    std::set<std::string> sites;
    std::vector<std::string> violations;
    std::map<uintptr_t, size_t> device;          // base -> bytes
    std::set<uintptr_t> pinned, streams, events;
    uint64_t waits = 0, skip = 0;                // the stream waits, counted apart: the skip-th is dropped
    bool skipped = false;
    std::string skipped_site;
    std::set<std::string> wait_sites;
};
Shim& shim() { static Shim s; return s; }

std::string site_of(const char* file, int line, const char* name) {
    const char* base = std::strrchr(file, '/');
    char buf[256];
    std::snprintf(buf, sizeof buf, "%s:%d %s", base ? base + 1 : file, line, name);
    return buf;
}

void violation(Shim& s, const std::string& site, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
void violation(Shim& s, const std::string& site, const char* fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    s.violations.push_back(site + ": " + buf);
}

// a creator call: true = refuse it (the armed one)
bool creator(Shim& s, const std::string& site) {
    s.sites.insert(site);
    s.calls++;
    if (s.armed != 0 && s.calls == s.armed) {
        s.armed = 0;
        s.fired = true;
        s.fired_site = site;
        return true;
    }
    return false;
}

// [p, p + bytes) inside one live device allocation?
bool in_live_device(const Shim& s, const void* p, size_t bytes) {
    const uintptr_t a = (uintptr_t)p;
    auto it = s.device.upper_bound(a);
    if (it == s.device.begin()) return false;
    --it;
    return a >= it->first && bytes <= it->second && a - it->first <= it->second - bytes;
}

// the device sides of a copy: false (and a violation) if one leaves the live allocations
bool copy_ok(Shim& s, const std::string& site, const void* dst, const void* src, size_t dst_bytes, size_t src_bytes, hipMemcpyKind kind) {
    const bool dst_dev = kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice;
    const bool src_dev = kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice;
    bool ok = true;
    if (kind != hipMemcpyHostToDevice && kind != hipMemcpyDeviceToHost && kind != hipMemcpyDeviceToDevice && kind != hipMemcpyHostToHost) {
        violation(s, site, "copy of kind %d: the device side cannot be checked", (int)kind);
        ok = false;
    }
    if (dst_dev && dst_bytes && !in_live_device(s, dst, dst_bytes)) {
        violation(s, site, "destination %p + %zu is not inside a live device allocation", dst, dst_bytes);
        ok = false;
    }
    if (src_dev && src_bytes && !in_live_device(s, src, src_bytes)) {
        violation(s, site, "source %p + %zu is not inside a live device allocation", src, src_bytes);
        ok = false;
    }
    return ok;
}

bool fill_ok(Shim& s, const std::string& site, const void* dst, size_t bytes) {
    if (!bytes || in_live_device(s, dst, bytes)) return true;
    violation(s, site, "destination %p + %zu is not inside a live device allocation", dst, bytes);
    return false;
}

// a release: true = forward it (the handle was live and is forgotten)
bool release(Shim& s, const std::string& site, std::set<uintptr_t>& live, const void* h, const char* what) {
    if (live.erase((uintptr_t)h)) return true;
    violation(s, site, "%s %p is not live (released twice, or never created)", what, h);
    return false;
}

}  // namespace

extern "C" {

hipError_t mrt_fi_malloc(const char* file, int line, void** p, size_t bytes) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    if (creator(s, site_of(file, line, "hipMalloc"))) return hipErrorOutOfMemory;
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess && *p) s.device[(uintptr_t)*p] = bytes;
    return e;
}

hipError_t mrt_fi_host_malloc(const char* file, int line, void** p, size_t bytes, unsigned flags) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    if (creator(s, site_of(file, line, "hipHostMalloc"))) return hipErrorOutOfMemory;
    const hipError_t e = hipHostMalloc(p, bytes, flags);
    if (e == hipSuccess && *p) s.pinned.insert((uintptr_t)*p);
    return e;
}

hipError_t mrt_fi_stream_create(const char* file, int line, hipStream_t* st, int with_flags, unsigned flags) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    if (creator(s, site_of(file, line, with_flags ? "hipStreamCreateWithFlags" : "hipStreamCreate"))) return hipErrorInvalidValue;
    const hipError_t e = with_flags ? hipStreamCreateWithFlags(st, flags) : hipStreamCreate(st);
    if (e == hipSuccess) s.streams.insert((uintptr_t)*st);
    return e;
}

hipError_t mrt_fi_event_create(const char* file, int line, hipEvent_t* ev, int with_flags, unsigned flags) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    if (creator(s, site_of(file, line, with_flags ? "hipEventCreateWithFlags" : "hipEventCreate"))) return hipErrorInvalidValue;
    const hipError_t e = with_flags ? hipEventCreateWithFlags(ev, flags) : hipEventCreate(ev);
    if (e == hipSuccess) s.events.insert((uintptr_t)*ev);
    return e;
}

hipError_t mrt_fi_free(const char* file, int line, void* p) {
    if (!p) return hipSuccess;                   // (hipFree(NULL) is defined to do nothing)
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    const std::string site = site_of(file, line, "hipFree");
    if (!s.device.erase((uintptr_t)p)) {
        violation(s, site, "device pointer %p is not live (released twice, or never created)", p);
        return hipErrorInvalidValue;
    }
    return hipFree(p);
}

hipError_t mrt_fi_host_free(const char* file, int line, void* p) {
    if (!p) return hipSuccess;
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    if (!release(s, site_of(file, line, "hipHostFree"), s.pinned, p, "pinned pointer")) return hipErrorInvalidValue;
    return hipHostFree(p);
}

hipError_t mrt_fi_stream_destroy(const char* file, int line, hipStream_t st) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    if (!release(s, site_of(file, line, "hipStreamDestroy"), s.streams, st, "stream")) return hipErrorInvalidValue;
    return hipStreamDestroy(st);
}

hipError_t mrt_fi_event_destroy(const char* file, int line, hipEvent_t ev) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    if (!release(s, site_of(file, line, "hipEventDestroy"), s.events, ev, "event")) return hipErrorInvalidValue;
    return hipEventDestroy(ev);
}

hipError_t mrt_fi_memcpy(const char* file, int line, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    Shim& s = shim();
    {
        std::lock_guard<std::mutex> g(s.mu);
        if (!copy_ok(s, site_of(file, line, "hipMemcpy"), dst, src, bytes, bytes, kind)) return hipErrorInvalidValue;
    }
    return hipMemcpy(dst, src, bytes, kind);
}

hipError_t mrt_fi_memcpy_async(const char* file, int line, void* dst, const void* src, size_t bytes, hipMemcpyKind kind,
                               hipStream_t stream) {
    Shim& s = shim();
    {
        std::lock_guard<std::mutex> g(s.mu);
        if (!copy_ok(s, site_of(file, line, "hipMemcpyAsync"), dst, src, bytes, bytes, kind)) return hipErrorInvalidValue;
    }
    return hipMemcpyAsync(dst, src, bytes, kind, stream);
}

hipError_t mrt_fi_memcpy2d_async(const char* file, int line, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
                                 size_t height, hipMemcpyKind kind, hipStream_t stream) {
    Shim& s = shim();
    {
        std::lock_guard<std::mutex> g(s.mu);
        const size_t db = height && width ? (height - 1) * dpitch + width : 0, sb = height && width ? (height - 1) * spitch + width : 0;
        if (!copy_ok(s, site_of(file, line, "hipMemcpy2DAsync"), dst, src, db, sb, kind)) return hipErrorInvalidValue;
    }
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, stream);
}

hipError_t mrt_fi_memcpy_peer_async(const char* file, int line, void* dst, int dst_dev, const void* src, int src_dev, size_t bytes,
                                    hipStream_t stream) {
    Shim& s = shim();
    {
        std::lock_guard<std::mutex> g(s.mu);
        if (!copy_ok(s, site_of(file, line, "hipMemcpyPeerAsync"), dst, src, bytes, bytes, hipMemcpyDeviceToDevice)) return hipErrorInvalidValue;
    }
    return hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, stream);
}

hipError_t mrt_fi_memset(const char* file, int line, void* dst, int value, size_t bytes) {
    Shim& s = shim();
    {
        std::lock_guard<std::mutex> g(s.mu);
        if (!fill_ok(s, site_of(file, line, "hipMemset"), dst, bytes)) return hipErrorInvalidValue;
    }
    return hipMemset(dst, value, bytes);
}

hipError_t mrt_fi_memset_async(const char* file, int line, void* dst, int value, size_t bytes, hipStream_t stream) {
    Shim& s = shim();
    {
        std::lock_guard<std::mutex> g(s.mu);
        if (!fill_ok(s, site_of(file, line, "hipMemsetAsync"), dst, bytes)) return hipErrorInvalidValue;
    }
    return hipMemsetAsync(dst, value, bytes, stream);
}

hipError_t mrt_fi_memset_d32_async(const char* file, int line, hipDeviceptr_t dst, int value, size_t count, hipStream_t stream) {
    Shim& s = shim();
    {
        std::lock_guard<std::mutex> g(s.mu);
        if (!fill_ok(s, site_of(file, line, "hipMemsetD32Async"), (const void*)dst, count * 4)) return hipErrorInvalidValue;
    }
    return hipMemsetD32Async(dst, value, count, stream);
}

hipError_t mrt_fi_stream_wait_event(const char* file, int line, hipStream_t stream, hipEvent_t event, unsigned flags) {
    Shim& s = shim();
    {
        std::lock_guard<std::mutex> g(s.mu);
        const std::string site = site_of(file, line, "hipStreamWaitEvent");
        s.wait_sites.insert(site);
        s.waits++;
        if (s.skip != 0 && s.waits == s.skip) {      // dropped: the caller sees success, the runtime sees nothing
            s.skip = 0;
            s.skipped = true;
            s.skipped_site = site;
            return hipSuccess;
        }
    }
    return hipStreamWaitEvent(stream, event, flags);
}

void mrt_fi_skip_wait(uint64_t n) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    s.skip = n; s.waits = 0; s.skipped = false; s.skipped_site.clear();
}

uint64_t mrt_fi_waits(void) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    return s.waits;
}

int mrt_fi_skipped(char* site, size_t cap) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    if (site && cap) std::snprintf(site, cap, "%s", s.skipped ? s.skipped_site.c_str() : "");
    return s.skipped ? 1 : 0;
}

size_t mrt_fi_wait_sites(char* buf, size_t cap) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    std::string all;
    for (const auto& x : s.wait_sites) all += x + "\n";
    if (buf && cap) std::snprintf(buf, cap, "%s", all.c_str());
    return all.size() + 1;
}

void mrt_fi_arm(uint64_t n) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    s.armed = n; s.calls = 0; s.fired = false; s.fired_site.clear();
}

void mrt_fi_disarm(void) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    s.armed = 0;
}

uint64_t mrt_fi_calls(void) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    return s.calls;
}

int mrt_fi_fired(char* site, size_t cap) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    if (site && cap) std::snprintf(site, cap, "%s", s.fired ? s.fired_site.c_str() : "");
    return s.fired ? 1 : 0;
}

size_t mrt_fi_sites(char* buf, size_t cap) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    std::string all;
    for (const auto& x : s.sites) all += x + "\n";
    if (buf && cap) std::snprintf(buf, cap, "%s", all.c_str());
    return all.size() + 1;
}

void mrt_fi_live(uint64_t out[4]) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    out[0] = s.device.size(); out[1] = s.pinned.size(); out[2] = s.streams.size(); out[3] = s.events.size();
}

size_t mrt_fi_violations(char* buf, size_t cap) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    std::string all;
    for (const auto& x : s.violations) all += x + "\n";
    if (buf && cap) std::snprintf(buf, cap, "%s", all.c_str());
    return s.violations.size();
}

void mrt_fi_reset(void) {
    Shim& s = shim();
    std::lock_guard<std::mutex> g(s.mu);
    s.sites.clear(); s.violations.clear();
    s.calls = 0; s.armed = 0; s.fired = false; s.fired_site.clear();
    s.wait_sites.clear();
    s.waits = 0; s.skip = 0; s.skipped = false; s.skipped_site.clear();
}

}  // extern "C"
