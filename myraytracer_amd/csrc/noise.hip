// The noise report (mrt_noise_query, include/myraytracer_amd.h "noise estimate"): one pass over a context's texels that reads
// the per-texel luminance variance S (kept by finalize_tracked_kernel, kernels.hip) and the framebuffer, and reduces them to
// the image-level report and a per-8x8-tile map.  Per finite pixel, in float32:
//   var_p = S_p * (float)K,  se_p = sqrtf(var_p),  L_p = lum(fb_p),  rel_p = se_p / fmaxf(L_p, floor),  above = rel_p > threshold
// with K = +inf ("no estimate yet") giving se_p = +inf without forming 0 * inf.  A pixel whose S or L is not finite counts in
// non_finite only.  Deterministic: every block writes its partial sums, a single-block pass adds them in block order; no
// float atomics.  lum() is rt_math.h's, the one the blend's S update uses (blend.h).  Memory-bound: 20 B per pixel.
#include <hip/hip_runtime.h>
#include "mrt_internal.h"
#include "rt_math.h"

namespace mrt {
namespace {

constexpr uint32_t kNoiseWaves = kBandRows;          // one wave per row of a band
constexpr uint32_t kNoiseCols = 256;                 // columns per block: 4 pixels per lane
constexpr uint32_t kNoiseFinalBlock = 256;

struct NoisePartial {                                // 32 B, one per block
    double sum_s, sum_l;
    uint32_t pixels, non_finite, above;
    float max_se;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// grid (ceil(width / 256), local_bands), 8 waves: wave r takes local row 8 band + r, lane l the pixels 64 i + l (i = 0..3) of
// the block's 256 columns -- every load instruction covers 64 consecutive texels (256 B of S, 1 KB of colour).  A local row
// counts only if its image row (the shard packing of mrt_shard_global_row) is < height: shard padding rows are skipped.
__global__ void __launch_bounds__(64 * kNoiseWaves) noise_reduce_kernel(const float* __restrict__ S, const float4* __restrict__ fb,
                                                                        uint32_t width, uint32_t height, uint32_t rank,
                                                                        uint32_t world, float K, float threshold, float floor_,
                                                                        NoisePartial* __restrict__ partials,
                                                                        float* __restrict__ tiles, uint32_t tiles_x) {
    __shared__ NoisePartial wave_part[kNoiseWaves];
    __shared__ float tile_part[kNoiseWaves][kNoiseCols / kTileW];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t band = blockIdx.y, x_base = blockIdx.x * kNoiseCols;
    const uint32_t lrow = band * kBandRows + wave;
    const bool row_ok = (band * world + rank) * kBandRows + wave < height;
    const bool no_estimate = __builtin_isinf(K);
    const size_t row = (size_t)lrow * width;
    double sum_s = 0.0, sum_l = 0.0;
    uint32_t pixels = 0, non_finite = 0, above = 0;
    float max_se = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < kNoiseCols / 64u; i++) {
        const uint32_t x = x_base + 64u * i + lane;
        float rel_max = 0.0f;
        if (row_ok && x < width) {
            const float s = S[row + x];
            const float4 c = fb[row + x];
            const float L = lumf(c.x, c.y, c.z);
            if (__builtin_isfinite(s) && __builtin_isfinite(L)) {
                pixels++;
                sum_s += (double)s;
                sum_l += (double)L;
                const float se = no_estimate ? __builtin_inff() : sqrtf(s * K);
                const float rel = se / fmaxf(L, floor_);
                above += rel > threshold ? 1u : 0u;
                max_se = fmaxf(max_se, se);
                rel_max = fmaxf(rel_max, rel);
            } else {
                non_finite++;
            }
        }
        // the tile's maximum over the 8 lanes of its columns, then (below) over the 8 rows
        rel_max = fmaxf(rel_max, __shfl_xor(rel_max, 1));
        rel_max = fmaxf(rel_max, __shfl_xor(rel_max, 2));
        rel_max = fmaxf(rel_max, __shfl_xor(rel_max, 4));
        if ((lane & 7u) == 0u) tile_part[wave][i * 8u + (lane >> 3)] = rel_max;
    }
    sum_s = wave_sum(sum_s);
    sum_l = wave_sum(sum_l);
    pixels = wave_sum(pixels);
    non_finite = wave_sum(non_finite);
    above = wave_sum(above);
    max_se = wave_max(max_se);
    if (lane == 0) wave_part[wave] = NoisePartial{sum_s, sum_l, pixels, non_finite, above, max_se};
    __syncthreads();
    if (threadIdx.x < kNoiseCols / kTileW) {
        const uint32_t tx = blockIdx.x * (kNoiseCols / kTileW) + threadIdx.x;
        float m = 0.0f;
#pragma unroll
        for (uint32_t r = 0; r < kNoiseWaves; r++) m = fmaxf(m, tile_part[r][threadIdx.x]);
        if (tx < tiles_x) tiles[(size_t)band * tiles_x + tx] = m;
    }
    if (threadIdx.x == 0) {
        NoisePartial p = wave_part[0];
        for (uint32_t r = 1; r < kNoiseWaves; r++) {
            const NoisePartial& q = wave_part[r];
            p.sum_s += q.sum_s; p.sum_l += q.sum_l;
            p.pixels += q.pixels; p.non_finite += q.non_finite; p.above += q.above;
            p.max_se = fmaxf(p.max_se, q.max_se);
        }
        partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
    }
}

// one block: thread t adds partials t, t + 256, ... in order, then a fixed tree over the threads
__global__ void __launch_bounds__(kNoiseFinalBlock) noise_final_kernel(const NoisePartial* __restrict__ partials, uint32_t n,
                                                                       NoiseSums* __restrict__ out) {
    __shared__ double ss[kNoiseFinalBlock], sl[kNoiseFinalBlock];
    __shared__ unsigned long long cp[kNoiseFinalBlock], cn[kNoiseFinalBlock], ca[kNoiseFinalBlock];
    __shared__ float mx[kNoiseFinalBlock];
    const uint32_t t = threadIdx.x;
    double s = 0.0, l = 0.0;
    unsigned long long p = 0, nf = 0, a = 0;
    float m = 0.0f;
    for (uint32_t i = t; i < n; i += kNoiseFinalBlock) {
        const NoisePartial q = partials[i];
        s += q.sum_s; l += q.sum_l;
        p += q.pixels; nf += q.non_finite; a += q.above;
        m = fmaxf(m, q.max_se);
    }
    ss[t] = s; sl[t] = l; cp[t] = p; cn[t] = nf; ca[t] = a; mx[t] = m;
    __syncthreads();
    for (uint32_t h = kNoiseFinalBlock / 2u; h > 0; h >>= 1) {
        if (t < h) {
            ss[t] += ss[t + h]; sl[t] += sl[t + h];
            cp[t] += cp[t + h]; cn[t] += cn[t + h]; ca[t] += ca[t + h];
            mx[t] = fmaxf(mx[t], mx[t + h]);
        }
        __syncthreads();
    }
    if (t == 0) *out = NoiseSums{ss[0], sl[0], cp[0], cn[0], ca[0], mx[0], 0u};
}

// noise_reduce_kernel after adaptive sampling has diverged (launch_noise_reduce_tiles): the same pass, with K per tile.  Pixel p of
// tile t (band x tiles_x + x / 8) takes K_t = Kf[tile_frames[t]] for var_p and adds (double)S_p * Kd[tile_frames[t]] to sum_s, so
// the partials' sum_s is sum_var itself; a tile whose K is +inf gives its pixels se = +inf and adds nothing (the report is "no
// estimate yet" then).  A kernel of its own: noise_reduce_kernel is left as it was.
__global__ void __launch_bounds__(64 * kNoiseWaves) noise_reduce_tiles_kernel(const float* __restrict__ S, const float4* __restrict__ fb,
                                                                              uint32_t width, uint32_t height,
                                                                              const uint32_t* __restrict__ tile_frames,
                                                                              const float* __restrict__ Kf, const double* __restrict__ Kd,
                                                                              float threshold, float floor_,
                                                                              NoisePartial* __restrict__ partials,
                                                                              float* __restrict__ tiles, uint32_t tiles_x) {
    __shared__ NoisePartial wave_part[kNoiseWaves];
    __shared__ float tile_part[kNoiseWaves][kNoiseCols / kTileW];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t band = blockIdx.y, x_base = blockIdx.x * kNoiseCols;
    const uint32_t lrow = band * kBandRows + wave;
    const bool row_ok = lrow < height;
    const size_t row = (size_t)lrow * width;
    double sum_s = 0.0, sum_l = 0.0;
    uint32_t pixels = 0, non_finite = 0, above = 0;
    float max_se = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < kNoiseCols / 64u; i++) {
        const uint32_t x = x_base + 64u * i + lane;
        float rel_max = 0.0f;
        if (row_ok && x < width) {
            const float s = S[row + x];
            const float4 c = fb[row + x];
            const float L = lumf(c.x, c.y, c.z);
            if (__builtin_isfinite(s) && __builtin_isfinite(L)) {
                const uint32_t nt = tile_frames[(size_t)band * tiles_x + x / kTileW];
                const float K = Kf[nt];
                const bool no_estimate = __builtin_isinf(K);
                pixels++;
                sum_s += no_estimate ? 0.0 : (double)s * Kd[nt];
                sum_l += (double)L;
                const float se = no_estimate ? __builtin_inff() : sqrtf(s * K);
                const float rel = se / fmaxf(L, floor_);
                above += rel > threshold ? 1u : 0u;
                max_se = fmaxf(max_se, se);
                rel_max = fmaxf(rel_max, rel);
            } else {
                non_finite++;
            }
        }
        rel_max = fmaxf(rel_max, __shfl_xor(rel_max, 1));
        rel_max = fmaxf(rel_max, __shfl_xor(rel_max, 2));
        rel_max = fmaxf(rel_max, __shfl_xor(rel_max, 4));
        if ((lane & 7u) == 0u) tile_part[wave][i * 8u + (lane >> 3)] = rel_max;
    }
    sum_s = wave_sum(sum_s);
    sum_l = wave_sum(sum_l);
    pixels = wave_sum(pixels);
    non_finite = wave_sum(non_finite);
    above = wave_sum(above);
    max_se = wave_max(max_se);
    if (lane == 0) wave_part[wave] = NoisePartial{sum_s, sum_l, pixels, non_finite, above, max_se};
    __syncthreads();
    if (threadIdx.x < kNoiseCols / kTileW) {
        const uint32_t tx = blockIdx.x * (kNoiseCols / kTileW) + threadIdx.x;
        float m = 0.0f;
#pragma unroll
        for (uint32_t r = 0; r < kNoiseWaves; r++) m = fmaxf(m, tile_part[r][threadIdx.x]);
        if (tx < tiles_x) tiles[(size_t)band * tiles_x + tx] = m;
    }
    if (threadIdx.x == 0) {
        NoisePartial p = wave_part[0];
        for (uint32_t r = 1; r < kNoiseWaves; r++) {
            const NoisePartial& q = wave_part[r];
            p.sum_s += q.sum_s; p.sum_l += q.sum_l;
            p.pixels += q.pixels; p.non_finite += q.non_finite; p.above += q.above;
            p.max_se = fmaxf(p.max_se, q.max_se);
        }
        partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
    }
}

// The reductions above with the other kind of tile map (mrt_noise_query_map, MRT_TILE_MAP_SUM_S): the partials are theirs,
// statement for statement -- kPerTile = false noise_reduce_kernel's, true noise_reduce_tiles_kernel's -- and the map entry is
// the tile's summed S instead of its largest rel: a counted pixel (in the image, S and L finite) gives (double)S_p, any other
// +0.0; a tile row's eight columns are added by the same three xor-shuffles the maximum takes -- the tree ((p0 + p1) + (p2 +
// p3)) + ((p4 + p5) + (p6 + p7)) in every lane, addition being commutative -- and the eight row sums through LDS, from the
// band's bottom row up, starting at 0.0; the entry is that double rounded to float.  No K and no n_t enter the map.
template <bool kPerTile>
__global__ void __launch_bounds__(64 * kNoiseWaves) noise_reduce_sum_kernel(const float* __restrict__ S, const float4* __restrict__ fb,
                                                                            uint32_t width, uint32_t height, uint32_t rank,
                                                                            uint32_t world, float K_uniform,
                                                                            const uint32_t* __restrict__ tile_frames,
                                                                            const float* __restrict__ Kf, const double* __restrict__ Kd,
                                                                            float threshold, float floor_,
                                                                            NoisePartial* __restrict__ partials,
                                                                            float* __restrict__ tiles, uint32_t tiles_x) {
    __shared__ NoisePartial wave_part[kNoiseWaves];
    __shared__ double tile_part[kNoiseWaves][kNoiseCols / kTileW];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t band = blockIdx.y, x_base = blockIdx.x * kNoiseCols;
    const uint32_t lrow = band * kBandRows + wave;
    const bool row_ok = kPerTile ? lrow < height : (band * world + rank) * kBandRows + wave < height;
    const size_t row = (size_t)lrow * width;
    double sum_s = 0.0, sum_l = 0.0;
    uint32_t pixels = 0, non_finite = 0, above = 0;
    float max_se = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < kNoiseCols / 64u; i++) {
        const uint32_t x = x_base + 64u * i + lane;
        double tile_s = 0.0;
        if (row_ok && x < width) {
            const float s = S[row + x];
            const float4 c = fb[row + x];
            const float L = lumf(c.x, c.y, c.z);
            if (__builtin_isfinite(s) && __builtin_isfinite(L)) {
                float K = K_uniform;
                bool no_estimate;
                pixels++;
                if (kPerTile) {
                    const uint32_t nt = tile_frames[(size_t)band * tiles_x + x / kTileW];
                    K = Kf[nt];
                    no_estimate = __builtin_isinf(K);
                    sum_s += no_estimate ? 0.0 : (double)s * Kd[nt];
                } else {
                    no_estimate = __builtin_isinf(K);
                    sum_s += (double)s;
                }
                sum_l += (double)L;
                const float se = no_estimate ? __builtin_inff() : sqrtf(s * K);
                const float rel = se / fmaxf(L, floor_);
                above += rel > threshold ? 1u : 0u;
                max_se = fmaxf(max_se, se);
                tile_s = (double)s;
            } else {
                non_finite++;
            }
        }
        tile_s += __shfl_xor(tile_s, 1);
        tile_s += __shfl_xor(tile_s, 2);
        tile_s += __shfl_xor(tile_s, 4);
        if ((lane & 7u) == 0u) tile_part[wave][i * 8u + (lane >> 3)] = tile_s;
    }
    sum_s = wave_sum(sum_s);
    sum_l = wave_sum(sum_l);
    pixels = wave_sum(pixels);
    non_finite = wave_sum(non_finite);
    above = wave_sum(above);
    max_se = wave_max(max_se);
    if (lane == 0) wave_part[wave] = NoisePartial{sum_s, sum_l, pixels, non_finite, above, max_se};
    __syncthreads();
    if (threadIdx.x < kNoiseCols / kTileW) {
        const uint32_t tx = blockIdx.x * (kNoiseCols / kTileW) + threadIdx.x;
        double m = 0.0;
#pragma unroll
        for (uint32_t r = 0; r < kNoiseWaves; r++) m += tile_part[r][threadIdx.x];
        if (tx < tiles_x) tiles[(size_t)band * tiles_x + tx] = (float)m;
    }
    if (threadIdx.x == 0) {
        NoisePartial p = wave_part[0];
        for (uint32_t r = 1; r < kNoiseWaves; r++) {
            const NoisePartial& q = wave_part[r];
            p.sum_s += q.sum_s; p.sum_l += q.sum_l;
            p.pixels += q.pixels; p.non_finite += q.non_finite; p.above += q.above;
            p.max_se = fmaxf(p.max_se, q.max_se);
        }
        partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
    }
}

}  // namespace

size_t noise_partials_bytes(uint32_t width, uint32_t local_bands) {
    return (size_t)((width + kNoiseCols - 1) / kNoiseCols) * local_bands * sizeof(NoisePartial);
}

int launch_noise_reduce(const float* S, const float* rgba, uint32_t width, uint32_t local_bands, uint32_t height,
                        uint32_t rank, uint32_t world, float K, float threshold, float floor_, void* partials, float* tiles,
                        NoiseSums* out, void* stream) {
    const uint32_t gx = (width + kNoiseCols - 1) / kNoiseCols;
    if (gx == 0 || local_bands == 0) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(noise_reduce_kernel, dim3(gx, local_bands), dim3(64 * kNoiseWaves), 0, st, S,
                       reinterpret_cast<const float4*>(rgba), width, height, rank, world, K, threshold, floor_,
                       reinterpret_cast<NoisePartial*>(partials), tiles, (width + kTileW - 1) / kTileW);
    hipLaunchKernelGGL(noise_final_kernel, dim3(1), dim3(kNoiseFinalBlock), 0, st,
                       reinterpret_cast<const NoisePartial*>(partials), gx * local_bands, out);
    return (int)hipGetLastError();
}

int launch_noise_reduce_tiles(const float* S, const float* rgba, uint32_t width, uint32_t local_bands, uint32_t height,
                              const uint32_t* tile_frames, const float* Kf, const double* Kd, float threshold, float floor_,
                              void* partials, float* tiles, NoiseSums* out, void* stream) {
    const uint32_t gx = (width + kNoiseCols - 1) / kNoiseCols;
    if (gx == 0 || local_bands == 0) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(noise_reduce_tiles_kernel, dim3(gx, local_bands), dim3(64 * kNoiseWaves), 0, st, S,
                       reinterpret_cast<const float4*>(rgba), width, height, tile_frames, Kf, Kd, threshold, floor_,
                       reinterpret_cast<NoisePartial*>(partials), tiles, (width + kTileW - 1) / kTileW);
    hipLaunchKernelGGL(noise_final_kernel, dim3(1), dim3(kNoiseFinalBlock), 0, st,
                       reinterpret_cast<const NoisePartial*>(partials), gx * local_bands, out);
    return (int)hipGetLastError();
}

int launch_noise_reduce_sum(const float* S, const float* rgba, uint32_t width, uint32_t local_bands, uint32_t height,
                            uint32_t rank, uint32_t world, float K, const uint32_t* tile_frames, const float* Kf, const double* Kd,
                            float threshold, float floor_, void* partials, float* tiles, NoiseSums* out, void* stream) {
    const uint32_t gx = (width + kNoiseCols - 1) / kNoiseCols;
    if (gx == 0 || local_bands == 0) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    auto* kernel = tile_frames ? noise_reduce_sum_kernel<true> : noise_reduce_sum_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(gx, local_bands), dim3(64 * kNoiseWaves), 0, st, S, reinterpret_cast<const float4*>(rgba), width,
                       height, rank, world, K, tile_frames, Kf, Kd, threshold, floor_, reinterpret_cast<NoisePartial*>(partials),
                       tiles, (width + kTileW - 1) / kTileW);
    hipLaunchKernelGGL(noise_final_kernel, dim3(1), dim3(kNoiseFinalBlock), 0, st,
                       reinterpret_cast<const NoisePartial*>(partials), gx * local_bands, out);
    return (int)hipGetLastError();
}

}  // namespace mrt
