// Adaptive sampling (mrt_render_tiles / mrt_render_adaptive, include/myraytracer_amd.h "adaptive sampling"): the blend of a frame
// whose tiles each have their own frame count n_t.  Once a subset frame has been blended, the framebuffer is blended in place
// (frames.cpp): a subset frame then costs its listed tiles, not the image, and the unlisted tiles keep their texels and S bit for bit.
// The steps of the blend are blend.h's, the ones finalize_kernel / finalize_tracked_kernel (kernels.hip) are built from.
#include <hip/hip_runtime.h>
#include "mrt_internal.h"
#include "blend.h"

namespace mrt {
namespace {

// one wave per listed tile.  The same blend and S update as a whole frame's (blend.h), at the weight mrt_frame_weight(n_t, max_w)
// computes on the host: so a tile's texels are exactly what a uniform accumulation of its n_t + 1 frames gives.  In place:
// every texel is read and then written by its own lane.
template <bool TRACKED>
__global__ void __launch_bounds__(64) tile_blend_kernel(const TileBlendArgs A) {
    const uint32_t lane = threadIdx.x;
    const uint32_t tile = A.list ? A.list[blockIdx.x] : blockIdx.x;
    uint32_t px, py;
    size_t texel;
    blend_locate(lane, tile, A.tiles_x, 1u, 0u, A.width, px, py, texel);      // one context of world 1: local rows are image rows
    const uint32_t nt = A.tile_frames[tile];
    float w = 0.0f;                                                   // mrt_frame_weight (lib.rs:301-304, :424)
    if (nt != 0u) {
        w = (float)nt / (float)(nt + 1u);                             // (n_t = UINT32_MAX: x / 0 = +inf, then max_w)
        w = A.max_w < w ? A.max_w : w;
    }
    uint32_t cost = 0;
    float4* const fb = reinterpret_cast<float4*>(A.fb);
    if (px < A.width && py < A.height) {
        const PixAcc sa = blend_sum_layers(reinterpret_cast<const PixAcc*>(A.pix_acc), texel, A.n_blocks, A.pix_stride);
        cost = sa.cost;
        blend_texel<TRACKED>(sa, A.spp, w, fb, fb, A.noise_s, texel);
    } else if (px < A.width) {
        blend_padding<TRACKED>(fb, A.noise_s, texel);                 // the last band's rows below the image
    }
    // the tile's heaviest pixel, for the slot's next queue order
    cost = blend_max_cost(cost);
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
