// Adaptive sampling (mrt_render_tiles / mrt_render_adaptive, include/myraytracer_amd.h "adaptive sampling"): the blend of a frame
// whose tiles each have their own frame count n_t.  Once a subset frame has been blended, the framebuffer is blended in place
// (frames.cpp): a subset frame then costs its listed tiles, not the image, and the unlisted tiles keep their texels and S bit for bit.
// A translation unit of its own, so that kernels.hip -- render_kernel and finalize_kernel / finalize_tracked_kernel -- is unchanged.
#include <hip/hip_runtime.h>
#include "mrt_internal.h"

namespace mrt {
namespace {

struct alignas(16) PixAcc { float r, g, b; uint32_t cost; };      // kernels.hip's colour sum + cost of one texel

__device__ __forceinline__ float mixf(float a, float b, float t) { return a * (1.0f - t) + b * t; }
__device__ __forceinline__ float lumf(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// one wave per listed tile.  The blend and S update are finalize_kernel<false>'s / finalize_tracked_kernel's, operation for
// operation (-ffp-contract=off), at the weight mrt_frame_weight(n_t, max_w) computes on the host: so a tile's texels are exactly
// what a uniform accumulation of its n_t + 1 frames gives.  In place: every texel is read and then written by its own lane.
template <bool TRACKED>
__global__ void __launch_bounds__(64) tile_blend_kernel(const TileBlendArgs A) {
    const uint32_t lane = threadIdx.x;
    const uint32_t tile = A.list ? A.list[blockIdx.x] : blockIdx.x;
    const uint32_t tile_x = tile % A.tiles_x, band = tile / A.tiles_x;
    const uint32_t px = tile_x * kTileW + (lane & 7u);
    const uint32_t py = band * kBandRows + (lane >> 3);
    const size_t texel = (size_t)py * A.width + px;
    const uint32_t nt = A.tile_frames[tile];
    float w = 0.0f;                                                   // mrt_frame_weight (lib.rs:301-304, :424)
    if (nt != 0u) {
        w = (float)nt / (float)(nt + 1u);                             // (n_t = UINT32_MAX: x / 0 = +inf, then max_w)
        w = A.max_w < w ? A.max_w : w;
    }
    uint32_t cost = 0;
    if (px < A.width && py < A.height) {
        const PixAcc* acc = reinterpret_cast<const PixAcc*>(A.pix_acc);
        PixAcc sa = acc[texel];
        for (uint32_t b = 1; b < A.n_blocks; b++) {
            const PixAcc sb = acc[(size_t)b * A.pix_stride + texel];
            sa.r += sb.r; sa.g += sb.g; sa.b += sb.b; sa.cost += sb.cost;
        }
        cost = sa.cost;
        const float n = (float)A.spp;
        const float mr = sa.r / n, mg = sa.g / n, mb = sa.b / n;
        float4* fb = reinterpret_cast<float4*>(A.fb);
        const float4 prev = fb[texel];
        float4 res;
        res.x = mixf(mr, prev.x, w);
        res.y = mixf(mg, prev.y, w);
        res.z = mixf(mb, prev.z, w);
        res.w = mixf(1.0f, prev.w, w);
        fb[texel] = res;
        if (TRACKED) {
            const float d = lumf(mr, mg, mb) - lumf(prev.x, prev.y, prev.z);
            const float s = A.noise_s[texel];
            A.noise_s[texel] = w == 0.0f ? 0.0f : w * (s + (1.0f - w) * (d * d));
        }
    } else if (px < A.width) {
        reinterpret_cast<float4*>(A.fb)[texel] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // the last band's rows below the image
        if (TRACKED) A.noise_s[texel] = 0.0f;
    }
    // the tile's heaviest pixel (finalize_kernel's cost), for the slot's next queue order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o2 = __shfl_xor(cost, off); cost = cost > o2 ? cost : o2; }
    if (lane == 0) {
        A.tile_cost[tile] = cost;
        A.tile_frames[tile] = nt == 0xFFFFFFFFu ? nt : nt + 1u;       // saturating, as frames_done
    }
    // the slot's tile queue is empty again for its next render launch (a list need not hold tile 0, so not finalize's rule)
    if (lane == 0 && blockIdx.x == 0) *A.tile_queue = 0u;
}

}  // namespace

int launch_tile_blend(const TileBlendArgs& a, void* stream) {
    if (a.n == 0) return 0;
    if (a.noise_s) hipLaunchKernelGGL(tile_blend_kernel<true>, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(tile_blend_kernel<false>, dim3(a.n), dim3(64), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mrt
