// The frame blend, in the pieces every kernel that blends is built from (finalize_kernel / finalize_tracked_kernel in
// kernels.hip, tile_blend_kernel in adaptive.hip), so that a tile blended by either comes out bit for bit the same: one wave per
// 8x8 tile sums the texel's PixAcc layers, divides by the samples per pixel, mixes with the previous texel (shader.wgsl:383-385),
// optionally updates the luminance variance S, and reduces the tile's cost.  Internal: not installed.
#pragma once
#include "mrt_internal.h"
#include "rt_math.h"

namespace mrt {

// What render_kernel leaves per pixel for the blend: the colour sum of the frame's samples
// and the pixel's cost (trips of the bounce loop).
struct alignas(16) PixAcc { float r, g, b; uint32_t cost; };

// lane `lane` of the wave that blends `tile` of shard `rank` of `world` (unsharded: 0 of 1): pixel (px, py = global row) and local texel
__device__ __forceinline__ void blend_locate(uint32_t lane, uint32_t tile, uint32_t tiles_x, uint32_t world, uint32_t rank,
                                             uint32_t W, uint32_t& px, uint32_t& py, size_t& texel) {
    const uint32_t tile_x = tile % tiles_x, band = tile / tiles_x;
    px = tile_x * kTileW + (lane & 7u);
    py = (band * world + rank) * kBandRows + (lane >> 3);
    texel = (size_t)(band * kBandRows + (lane >> 3)) * W + px;
}
// counter-RNG mode: the pixel's blocks of 64 samples were summed separately (possibly by different lanes);
// their sums are added in block order -- ((S0 + S1) + S2) ... -- which is how the mode defines the colour
__device__ __forceinline__ PixAcc blend_sum_layers(const PixAcc* acc, size_t texel, uint32_t n_blocks, uint32_t pix_stride) {
    PixAcc sa = acc[texel];
    for (uint32_t b = 1; b < n_blocks; b++) {
        const PixAcc sb = acc[(size_t)b * pix_stride + texel];
        sa.r += sb.r; sa.g += sb.g; sa.b += sb.b; sa.cost += sb.cost;
    }
    return sa;
}
// One texel: mean = sum / spp (:383), out = mix(mean, prev, w) (:385, framebuffer_load :366-369; alpha from 1), and with TRACKED
// the per-texel luminance variance S (noise_s, same texel index) by West's weighted recursion with the blend's own weights:
//   d = lum(mean) - lum(prev.rgb),   S' = (w == 0.0f) ? 0.0f : w * (S + (1.0f - w) * (d * d))
// (a select at w == 0: NaN / Inf from before a reset does not survive it).  prev and out may be the same buffer.
template <bool TRACKED>
__device__ __forceinline__ void blend_texel(const PixAcc sa, uint32_t spp, float w, const float4* prev_fb, float4* out_fb,
                                            float* noise_s, size_t texel) {
    const float n = (float)spp;
    const V3 mean = v3(sa.r / n, sa.g / n, sa.b / n);
    const float4 prev = prev_fb[texel];
    float4 res;
    res.x = mixf(mean.x, prev.x, w);
    res.y = mixf(mean.y, prev.y, w);
    res.z = mixf(mean.z, prev.z, w);
    res.w = mixf(1.0f, prev.w, w);
    out_fb[texel] = res;
    if (TRACKED) {
        const float d = lumf(mean.x, mean.y, mean.z) - lumf(prev.x, prev.y, prev.z);
        const float s = noise_s[texel];
        noise_s[texel] = w == 0.0f ? 0.0f : w * (s + (1.0f - w) * (d * d));
    }
}
// rows of the last band that lie below the image (shard padding rows): zero texels, S = 0
template <bool TRACKED>
__device__ __forceinline__ void blend_padding(float4* out_fb, float* noise_s, size_t texel) {
    out_fb[texel] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (TRACKED) noise_s[texel] = 0.0f;
}
// A pixel's samples form one sequential chain, so the frame's critical path is its longest
// pixel: tiles are ranked by their HEAVIEST pixel, not by their sum.  Maximum over the wave's 64 lanes, in every lane.
__device__ __forceinline__ uint32_t blend_max_cost(uint32_t cost) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o2 = __shfl_xor(cost, off); cost = cost > o2 ? cost : o2; }
    return cost;
}

}  // namespace mrt
