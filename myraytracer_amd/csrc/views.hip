// The diagnostic views (mrt_set_view / mrt_read_view / MRT_PRESENT_VIEW, include/myraytracer_amd.h "diagnostic views"): what the
// renderer decides by -- the per-pixel noise estimate, the per-tile frame count, the first-hit guides -- as an RGBA32F image the
// size of the frame.  One pass, one thread per pixel, that reads only what its kind needs and writes one texel; the header states
// the arithmetic, tests/view_ref.py restates it.  The noise kinds are noise_reduce_kernel's se and rel (noise.hip), with the same
// lum() (rt_math.h) and under the same -ffp-contract=off.  A translation unit of its own: nothing of the render, noise, denoise or
// present kernels changes.  Memory-bound; per pixel, read + written: NOISE_* 20 B + 16 B (per tile: + the tile's n_t and K, from
// cache), TILE_FRAMES 0 B + 16 B (per tile: the tile's n_t), DEPTH / NORMAL / ALBEDO / SPHERE 16 B + 16 B.
#include <hip/hip_runtime.h>
#include "mrt_internal.h"
#include "rt_math.h"

namespace mrt {
namespace {

constexpr uint32_t kViewBlock = 256;

__device__ __forceinline__ float c01(float y) { return fminf(fmaxf(y, 0.0f), 1.0f); }

// a scalar through the ramp: grey is u itself, unclamped; heat runs blue, cyan, green, yellow, red over u in 0..1, a NaN magenta
__device__ __forceinline__ float4 ramp_of(float q, uint32_t ramp, float lo, float inv) {
    const float u = (q - lo) * inv;
    if (ramp == MRT_VIEW_RAMP_GREY) return make_float4(u, u, u, 1.0f);
    if (q != q) return make_float4(1.0f, 0.0f, 1.0f, 1.0f);
    const float v = fminf(fmaxf(u, 0.0f), 1.0f), x = v * 4.0f;
    return make_float4(c01(x - 2.0f), c01(fminf(x, 4.0f - x)), c01(2.0f - x), 1.0f);
}

__device__ __forceinline__ float hash_channel(uint32_t byte) { return ((float)byte + 0.5f) * (1.0f / 256.0f); }

// grid ceil(pixels / 256): thread i takes pixel i = y * width + x of the world-1 texel order the framebuffer, S and the guides
// share.  kKind: MRT_VIEW_*; kPerTile (NOISE_*, TILE_FRAMES): n_t = tile_frames[(y / 8) * tiles_x + x / 8] and K = Kf[n_t], else
// the launch's K and count.  Every load and the store are 16 bytes a lane (S: 4), consecutive lanes consecutive texels.
template <uint32_t kKind, bool kPerTile>
__global__ void __launch_bounds__(kViewBlock) view_kernel(ViewArgs a) {
    const size_t n = (size_t)a.width * a.height;
    const size_t i = (size_t)blockIdx.x * kViewBlock + threadIdx.x;
    if (i >= n) return;
    float4 out;
    if constexpr (kKind == MRT_VIEW_NOISE_SE || kKind == MRT_VIEW_NOISE_REL || kKind == MRT_VIEW_TILE_FRAMES) {
        float K = a.K, frames = a.frames;
        if constexpr (kPerTile) {
            const uint32_t y = (uint32_t)(i / a.width), x = (uint32_t)(i - (size_t)y * a.width);
            const uint32_t nt = a.tile_frames[(size_t)(y / kBandRows) * a.tiles_x + x / kTileW];
            frames = (float)nt;
            if constexpr (kKind != MRT_VIEW_TILE_FRAMES) K = a.Kf[nt];
        }
        float q = frames;
        if constexpr (kKind != MRT_VIEW_TILE_FRAMES) {
            const float s = a.S[i];
            const float4 c = reinterpret_cast<const float4*>(a.fb)[i];
            const float L = lumf(c.x, c.y, c.z);
            if (__builtin_isfinite(s) && __builtin_isfinite(L)) {
                const float se = __builtin_isinf(K) ? __builtin_inff() : sqrtf(s * K);
                q = kKind == MRT_VIEW_NOISE_SE ? se : se / fmaxf(L, a.rel_floor);
            } else {
                q = __builtin_nanf("");
            }
        }
        out = ramp_of(q, a.ramp, a.lo, a.inv);
    } else if constexpr (kKind == MRT_VIEW_DEPTH) {
        out = ramp_of(reinterpret_cast<const float4*>(a.guides)[2 * i].w, a.ramp, a.lo, a.inv);
    } else if constexpr (kKind == MRT_VIEW_NORMAL) {
        const float4 g = reinterpret_cast<const float4*>(a.guides)[2 * i];
        out = make_float4(g.x * 0.5f + 0.5f, g.y * 0.5f + 0.5f, g.z * 0.5f + 0.5f, 1.0f);
    } else {
        // (loaded as integers: the albedo keeps its bits, and the index is no float)
        const uint4 g = reinterpret_cast<const uint4*>(a.guides)[2 * i + 1];
        if constexpr (kKind == MRT_VIEW_ALBEDO) {
            out = make_float4(__uint_as_float(g.x), __uint_as_float(g.y), __uint_as_float(g.z), 1.0f);
        } else {
            uint32_t h = (g.w + 1u) * 2654435761u;
            h ^= h >> 15;
            out = g.w == 0xFFFFFFFFu ? make_float4(0.0f, 0.0f, 0.0f, 1.0f)
                              : make_float4(hash_channel(h >> 24), hash_channel((h >> 16) & 255u), hash_channel((h >> 8) & 255u), 1.0f);
        }
    }
    reinterpret_cast<float4*>(a.out)[i] = out;
}

template <uint32_t kKind, bool kPerTile>
void launch_one(const ViewArgs& a, uint32_t blocks, hipStream_t st) {
    hipLaunchKernelGGL((view_kernel<kKind, kPerTile>), dim3(blocks), dim3(kViewBlock), 0, st, a);
}

}  // namespace

int launch_view(const ViewArgs& a, void* stream) {
    const size_t n = (size_t)a.width * a.height;
    const size_t blocks = (n + kViewBlock - 1) / kViewBlock;
    if (n == 0) return 0;
    if (blocks > 0x7FFFFFFFu || !a.out) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const bool per_tile = a.tile_frames != nullptr;
    const uint32_t b = (uint32_t)blocks;
    switch (a.kind) {
        case MRT_VIEW_NOISE_SE: per_tile ? launch_one<MRT_VIEW_NOISE_SE, true>(a, b, st) : launch_one<MRT_VIEW_NOISE_SE, false>(a, b, st); break;
        case MRT_VIEW_NOISE_REL: per_tile ? launch_one<MRT_VIEW_NOISE_REL, true>(a, b, st) : launch_one<MRT_VIEW_NOISE_REL, false>(a, b, st); break;
        case MRT_VIEW_TILE_FRAMES: per_tile ? launch_one<MRT_VIEW_TILE_FRAMES, true>(a, b, st) : launch_one<MRT_VIEW_TILE_FRAMES, false>(a, b, st); break;
        case MRT_VIEW_DEPTH: launch_one<MRT_VIEW_DEPTH, false>(a, b, st); break;
        case MRT_VIEW_NORMAL: launch_one<MRT_VIEW_NORMAL, false>(a, b, st); break;
        case MRT_VIEW_ALBEDO: launch_one<MRT_VIEW_ALBEDO, false>(a, b, st); break;
        case MRT_VIEW_SPHERE: launch_one<MRT_VIEW_SPHERE, false>(a, b, st); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

}  // namespace mrt
