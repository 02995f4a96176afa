// The noise report (mrt_noise_query, include/myraytracer_amd.h "noise estimate"): one pass over a context's texels that reads
// the per-texel luminance variance S (kept by finalize_tracked_kernel, kernels.hip) and the framebuffer, and reduces them to
// the image-level report and a per-8x8-tile map.  Per finite pixel, in float32:
//   var_p = S_p * (float)K,  se_p = sqrtf(var_p),  L_p = lum(fb_p),  rel_p = se_p / fmaxf(L_p, floor),  above = rel_p > threshold
// with K = +inf ("no estimate yet") giving se_p = +inf without forming 0 * inf.  A pixel whose S or L is not finite counts in
// non_finite only.  Deterministic: every block writes its partial sums, a single-block pass adds them in block order; no
// float atomics.  lum() is rt_math.h's, the one the blend's S update uses (blend.h).  Memory-bound: 20 B per pixel.
#include <hip/hip_runtime.h>
#include <type_traits>
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
// One body for the four forms of launch_noise_reduce (mrt_internal.h states the arithmetic); they differ in two places:
//   kPerTile  where K comes from and what a pixel adds to sum_s: the launch's K and (double)S_p, or K_t = Kf[n_t] and (double)S_p *
//             Kd[n_t] (nothing where K_t is +inf) with n_t = tile_frames[band x tiles_x + x / 8];
//   kSumMap   a tile's map entry: the largest rel of its counted pixels (float, fmaxf from 0) or their summed S (double, + from
//             0.0), joined over a row's eight columns by three xor-shuffles and over the eight rows through LDS, row 0 first.
__device__ __forceinline__ float tile_join(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double tile_join(double a, double b) { return a + b; }

template <bool kPerTile, bool kSumMap>
__global__ void __launch_bounds__(64 * kNoiseWaves) noise_reduce_kernel(const float* __restrict__ S, const float4* __restrict__ fb,
                                                                        uint32_t width, uint32_t height, uint32_t rank,
                                                                        uint32_t world, float K_uniform,
                                                                        const uint32_t* __restrict__ tile_frames,
                                                                        const float* __restrict__ Kf, const double* __restrict__ Kd,
                                                                        float threshold, float floor_,
                                                                        NoisePartial* __restrict__ partials,
                                                                        float* __restrict__ tiles, uint32_t tiles_x) {
    using Entry = std::conditional_t<kSumMap, double, float>;
    __shared__ NoisePartial wave_part[kNoiseWaves];
    __shared__ Entry tile_part[kNoiseWaves][kNoiseCols / kTileW];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t band = blockIdx.y, x_base = blockIdx.x * kNoiseCols;
    const uint32_t lrow = band * kBandRows + wave;
    const bool row_ok = (band * world + rank) * kBandRows + wave < height;
    const size_t row = (size_t)lrow * width;
    double sum_s = 0.0, sum_l = 0.0;
    uint32_t pixels = 0, non_finite = 0, above = 0;
    float max_se = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < kNoiseCols / 64u; i++) {
        const uint32_t x = x_base + 64u * i + lane;
        Entry entry = 0;
        if (row_ok && x < width) {
            const float s = S[row + x];
            const float4 c = fb[row + x];
            const float L = lumf(c.x, c.y, c.z);
            if (__builtin_isfinite(s) && __builtin_isfinite(L)) {
                float K = K_uniform;
                double s_term = (double)s;
                if constexpr (kPerTile) {
                    const uint32_t nt = tile_frames[(size_t)band * tiles_x + x / kTileW];
                    K = Kf[nt];
                    s_term = __builtin_isinf(K) ? 0.0 : (double)s * Kd[nt];
                }
                const bool no_estimate = __builtin_isinf(K);
                pixels++;
                sum_s += s_term;
                sum_l += (double)L;
                const float se = no_estimate ? __builtin_inff() : sqrtf(s * K);
                const float rel = se / fmaxf(L, floor_);
                above += rel > threshold ? 1u : 0u;
                max_se = fmaxf(max_se, se);
                if constexpr (kSumMap) entry = (double)s;
                else entry = fmaxf(entry, rel);
            } else {
                non_finite++;
            }
        }
        // the tile row's entry over the 8 lanes of its columns, then (below) over the 8 rows
        entry = tile_join(entry, __shfl_xor(entry, 1));
        entry = tile_join(entry, __shfl_xor(entry, 2));
        entry = tile_join(entry, __shfl_xor(entry, 4));
        if ((lane & 7u) == 0u) tile_part[wave][i * 8u + (lane >> 3)] = entry;
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
        Entry m = 0;
#pragma unroll
        for (uint32_t r = 0; r < kNoiseWaves; r++) m = tile_join(m, tile_part[r][threadIdx.x]);
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

}  // namespace

size_t noise_partials_bytes(uint32_t width, uint32_t local_bands) {
    return (size_t)((width + kNoiseCols - 1) / kNoiseCols) * local_bands * sizeof(NoisePartial);
}

int launch_noise_reduce(const NoiseReduceArgs& a, void* stream) {
    const uint32_t gx = (a.width + kNoiseCols - 1) / kNoiseCols;
    if (gx == 0 || a.local_bands == 0) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const bool sum_map = a.map_kind == MRT_TILE_MAP_SUM_S;
    auto* kernel = a.tile_frames ? (sum_map ? noise_reduce_kernel<true, true> : noise_reduce_kernel<true, false>)
                                 : (sum_map ? noise_reduce_kernel<false, true> : noise_reduce_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(gx, a.local_bands), dim3(64 * kNoiseWaves), 0, st, a.S, reinterpret_cast<const float4*>(a.rgba),
                       a.width, a.height, a.rank, a.world, a.K, a.tile_frames, a.Kf, a.Kd, a.threshold, a.floor,
                       reinterpret_cast<NoisePartial*>(a.partials), a.tiles, (a.width + kTileW - 1) / kTileW);
    hipLaunchKernelGGL(noise_final_kernel, dim3(1), dim3(kNoiseFinalBlock), 0, st,
                       reinterpret_cast<const NoisePartial*>(a.partials), gx * a.local_bands, a.out);
    return (int)hipGetLastError();
}

}  // namespace mrt
