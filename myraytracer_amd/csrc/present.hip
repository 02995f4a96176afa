// The present pass (mrt_present, include/myraytracer_amd.h): the reference samples its accumulated RGBA32F texture onto the
// window surface (sample_framebuffer.wgsl, the Y flip at :24), an 8-bit sRGB format (lib.rs:349-351, :1133), so the hardware
// applies the sRGB OETF to colour, stores alpha linearly and rounds both to 8 bits.  This kernel does the same on the device,
// bit-identical to the host's mrt_srgb8 (image_io.cpp) for every float: it counts the thresholds of present_thresholds() that
// a value reaches, by an 8-step binary search over the table in LDS.  A translation unit of its own, outside the render path's
// (kernels.hip).  Memory-bound: 16 B in and 4 B out per pixel.
// The linear formats (MRT_PRESENT_RGBA16F_LINEAR / RGBA32F_LINEAR) go through a kernel of their own below, present_float_kernel:
// no table, no clamp, alpha like colour; 16 B in and 8 or 16 B out per pixel.
#include <hip/hip_runtime.h>
#include "mrt_internal.h"

namespace mrt {
namespace {

constexpr uint32_t kPresentBlock = 256;

// the number of t[1..255] (non-decreasing) that are <= v; NaN reaches none
__device__ __forceinline__ uint32_t code_of(const float* t, float v) {
    uint32_t k = 0;
#pragma unroll
    for (uint32_t step = 128; step != 0; step >>= 1) k += t[k + step] <= v ? step : 0u;
    return k;
}

__device__ __forceinline__ uint32_t pack_texel(const float* tc, const float* ta, float4 v, uint32_t bgra) {
    const uint32_t r = code_of(tc, v.x), g = code_of(tc, v.y), b = code_of(tc, v.z), a = code_of(ta, v.w);
    return (bgra ? b | r << 16 : r | b << 16) | g << 8 | a << 24;
}

// One thread per 4 horizontally adjacent texels of a row: four 16-B loads and one 16-B store (kAligned: rows a multiple of 4
// texels wide) or four 4-B stores, and a row's last quad may be partial.  src: `rows` rows of `width` texels, row 0 = bottom;
// dst: the same rows, or top-down with `flip`.  tables: the 2 x 256 thresholds (colour, alpha) of present_thresholds().
template <bool kAligned>
__global__ void __launch_bounds__(kPresentBlock) present_kernel(const float4* __restrict__ src, uint32_t* __restrict__ dst,
                                                                uint32_t width, uint32_t rows, uint32_t flip, uint32_t bgra,
                                                                const float* __restrict__ tables) {
    __shared__ float tc[256], ta[256];
    tc[threadIdx.x] = tables[threadIdx.x];
    ta[threadIdx.x] = tables[256 + threadIdx.x];
    __syncthreads();
    const uint32_t quads = (width + 3u) / 4u;
    const size_t n = (size_t)quads * rows;
    for (size_t q = (size_t)blockIdx.x * kPresentBlock + threadIdx.x; q < n; q += (size_t)gridDim.x * kPresentBlock) {
        const uint32_t y = (uint32_t)(q / quads), x0 = (uint32_t)(q - (size_t)y * quads) * 4u;
        const float4* s = src + (size_t)y * width + x0;
        uint32_t* d = dst + (size_t)(flip ? rows - 1u - y : y) * width + x0;
        if (kAligned) {
            const float4 v0 = s[0], v1 = s[1], v2 = s[2], v3 = s[3];
            *reinterpret_cast<uint4*>(d) = make_uint4(pack_texel(tc, ta, v0, bgra), pack_texel(tc, ta, v1, bgra),
                                                      pack_texel(tc, ta, v2, bgra), pack_texel(tc, ta, v3, bgra));
        } else {
            const uint32_t m = width - x0 < 4u ? width - x0 : 4u;
            for (uint32_t i = 0; i < m; i++) d[i] = pack_texel(tc, ta, s[i], bgra);
        }
    }
}

// The linear formats.  kMode 0: RGBA32F, the source's bits (loaded and stored as integers: a NaN keeps its payload), one 16-B
// store per texel; 1: RGBA16F (half_bits per channel, mrt_internal.h) in rows a multiple of 4 texels wide, two 16-B stores per
// quad; 2: RGBA16F in rows of any width, one 8-B store per texel.  One thread per 4 horizontally adjacent texels, as above.
__device__ __forceinline__ uint2 half_texel(uint4 v) {
    return make_uint2((uint32_t)half_bits(__uint_as_float(v.x)) | (uint32_t)half_bits(__uint_as_float(v.y)) << 16,
                      (uint32_t)half_bits(__uint_as_float(v.z)) | (uint32_t)half_bits(__uint_as_float(v.w)) << 16);
}

template <int kMode>
__global__ void __launch_bounds__(kPresentBlock) present_float_kernel(const uint4* __restrict__ src, void* __restrict__ dst,
                                                                      uint32_t width, uint32_t rows, uint32_t flip) {
    const uint32_t quads = (width + 3u) / 4u;
    const size_t n = (size_t)quads * rows;
    for (size_t q = (size_t)blockIdx.x * kPresentBlock + threadIdx.x; q < n; q += (size_t)gridDim.x * kPresentBlock) {
        const uint32_t y = (uint32_t)(q / quads), x0 = (uint32_t)(q - (size_t)y * quads) * 4u;
        const uint4* s = src + (size_t)y * width + x0;
        const size_t at = (size_t)(flip ? rows - 1u - y : y) * width + x0;
        const uint32_t m = width - x0 < 4u ? width - x0 : 4u;
        if (m == 4u) {
            const uint4 v0 = s[0], v1 = s[1], v2 = s[2], v3 = s[3];
            if (kMode == 0) {
                uint4* d = static_cast<uint4*>(dst) + at;
                d[0] = v0; d[1] = v1; d[2] = v2; d[3] = v3;
            } else if (kMode == 1) {
                const uint2 h0 = half_texel(v0), h1 = half_texel(v1), h2 = half_texel(v2), h3 = half_texel(v3);
                uint4* d = reinterpret_cast<uint4*>(static_cast<uint2*>(dst) + at);
                d[0] = make_uint4(h0.x, h0.y, h1.x, h1.y);
                d[1] = make_uint4(h2.x, h2.y, h3.x, h3.y);
            } else {
                uint2* d = static_cast<uint2*>(dst) + at;
                d[0] = half_texel(v0); d[1] = half_texel(v1); d[2] = half_texel(v2); d[3] = half_texel(v3);
            }
        } else if (kMode == 0) {
            uint4* d = static_cast<uint4*>(dst) + at;
            for (uint32_t i = 0; i < m; i++) d[i] = s[i];
        } else {            // (kMode 1 has no partial quad)
            uint2* d = static_cast<uint2*>(dst) + at;
            for (uint32_t i = 0; i < m; i++) d[i] = half_texel(s[i]);
        }
    }
}

}  // namespace

int launch_present_float(const float* src, uint8_t* dst, uint32_t width, uint32_t rows, uint32_t flip, uint32_t half, void* stream) {
    const size_t quads = (size_t)((width + 3u) / 4u) * rows;
    if (quads == 0) return 0;
    const dim3 grid((uint32_t)std::min<size_t>((quads + kPresentBlock - 1) / kPresentBlock, 2048)), block(kPresentBlock);
    const uint4* s = reinterpret_cast<const uint4*>(src);
    if (!half)
        hipLaunchKernelGGL(present_float_kernel<0>, grid, block, 0, (hipStream_t)stream, s, (void*)dst, width, rows, flip);
    else if (width % 4u == 0u)
        hipLaunchKernelGGL(present_float_kernel<1>, grid, block, 0, (hipStream_t)stream, s, (void*)dst, width, rows, flip);
    else
        hipLaunchKernelGGL(present_float_kernel<2>, grid, block, 0, (hipStream_t)stream, s, (void*)dst, width, rows, flip);
    return (int)hipGetLastError();
}

int launch_present(const float* src, uint8_t* dst, uint32_t width, uint32_t rows, uint32_t flip, uint32_t bgra,
                   const float* d_tables, void* stream) {
    const size_t quads = (size_t)((width + 3u) / 4u) * rows;
    if (quads == 0) return 0;
    const size_t blocks = std::min<size_t>((quads + kPresentBlock - 1) / kPresentBlock, 2048);
    if (width % 4u == 0u)
        hipLaunchKernelGGL(present_kernel<true>, dim3((uint32_t)blocks), dim3(kPresentBlock), 0, (hipStream_t)stream,
                           reinterpret_cast<const float4*>(src), reinterpret_cast<uint32_t*>(dst), width, rows, flip, bgra, d_tables);
    else
        hipLaunchKernelGGL(present_kernel<false>, dim3((uint32_t)blocks), dim3(kPresentBlock), 0, (hipStream_t)stream,
                           reinterpret_cast<const float4*>(src), reinterpret_cast<uint32_t*>(dst), width, rows, flip, bgra, d_tables);
    return (int)hipGetLastError();
}

}  // namespace mrt
