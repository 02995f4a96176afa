// The denoiser (include/myraytracer_amd.h, "denoiser"): first-hit guide buffers and a variance-guided,
// edge-aware a-trous filter over the framebuffer (the spatial filter of SVGF without its temporal part: the accumulation is
// the temporal part; a moving scene's is temporal.hip, whose history the same iterations filter).  A translation unit of its own, outside the render path's (kernels.hip).
//
// Guides (once per camera / scene): guide_rays_kernel writes one ray per pixel through the mean of the render's sample
// positions; the closest hits come from the DBG instantiation of render_kernel (launch_debug_world_hit, no candidate bitmap);
// guide_fill_kernel turns them into the per-texel record the filter reads.
// Filter: atrous_pixel is the a-trous iteration of one pixel, colour and variance ping-ponged as one float4, one launch per
// iteration.  Its three entry points are a bounds check and a call each, and differ in the centre's luminance stop alone:
// atrous_kernel (uniform, A.lum_stop), atrous_prefilter_kernel (always, on the prefiltered variance: the variance modes of
// mrt_set_denoise_variance) and atrous_tiles_kernel (per pixel, from its tile's frame count: an adaptive accumulation).
// Estimate: spatial_estimate is the 7 x 7 weighted luminance variance of one pixel, for a field that has none of its own yet.
// Its entry points make the field iteration 0 reads: spatial_variance_kernel (a short uniform history), tile_variance_kernel (per
// tile) and temporal_variance_kernel (the short histories of the temporal image).
// Blend (mrt_set_denoise_mix): mix_kernel, one launch behind the iterations of an accumulation, mixes the filtered with the
// accumulated image per pixel from 5 x 5 records held in LDS.
// Only + - * /, sqrtf, fminf, fmaxf in a fixed order (-ffp-contract=off; hipcc's `/` and sqrtf are correctly rounded), so
// tests/denoise_ref.py and its siblings restate all of it bit for bit in float32 numpy.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "mrt_internal.h"
#include "rt_math.h"

namespace mrt {
namespace {

constexpr uint32_t kTileX = 32, kTileY = 8;          // one workgroup: 32 x 8 pixels (4 waves of 32 x 2)

// Tukey's biweight: compact support, no transcendental
__device__ __forceinline__ float tukey(float x) {
    const float u = 1.0f - x * x;
    return x < 1.0f ? u * u : 0.0f;
}
__device__ __forceinline__ bool finite3(float4 v) {            // (the colour of a texel alone)
    return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z);
}
__device__ __forceinline__ bool finite4(float4 v) { return finite3(v) && __builtin_isfinite(v.w); }

// One ray per image pixel (world 1: texel = y * width + x), as render_kernel's new_sample_head makes a sample's camera ray
// with u = v = 0.5 (fs_main :373-381) and, for the look-at camera, the lens centre; normalised as the render normalises
// (WGSL normalize: v / sqrt(dot(v, v)), dot = fma(z, z, fma(y, y, x * x))).  6 floats per ray: origin, direction.
__global__ void __launch_bounds__(256) guide_rays_kernel(float* __restrict__ rays, uint32_t width, uint32_t height,
                                                         const mrt_camera_raw cam) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
    if (x >= width) return;
    const float pixel_side = 2.0f / (float)height;
    const float base_x = (((float)x + 0.5f) - 0.5f * (float)width) * pixel_side;
    const float base_y = (((float)y + 0.5f) - 0.5f * (float)height) * pixel_side;
    const float vx = base_x + 0.5f * pixel_side, vy = base_y + 0.5f * pixel_side;
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {vx, vy, -1.0f};
    if (cam.mode != 0) {
        for (int k = 0; k < 3; k++) {
            d[k] = (vx * cam.su[k] + vy * cam.sv[k]) - cam.fw[k];
            o[k] = cam.origin[k];
        }
    }
    const float len = __builtin_sqrtf(__builtin_fmaf(d[2], d[2], __builtin_fmaf(d[1], d[1], d[0] * d[0])));
    float* r = rays + 6u * ((size_t)y * width + x);
    r[0] = o[0]; r[1] = o[1]; r[2] = o[2];
    r[3] = d[0] / len; r[4] = d[1] / len; r[5] = d[2] / len;
}

// hits {sphere | -1, bits of t} -> guides {n.x, n.y, n.z, t} {albedo r, g, b, bits of the sphere index}.  The normal is
// sphere_hit's (shader.wgsl:298-309): at = o + t d, (at - centre) / radius, negated unless dot(normal, d) <= 0.
// Albedo: Lambertian / Metal albedo, (1, 1, 1) for a Dielectric, (0, 0, 0) for an unknown type.  A miss: t = +inf,
// normal = -d, albedo (1, 1, 1).
__global__ void __launch_bounds__(256) guide_fill_kernel(const float* __restrict__ rays, const int32_t* __restrict__ hits,
                                                         const float4* __restrict__ shade, const int32_t* __restrict__ mat_ty,
                                                         float4* __restrict__ guides, uint32_t width) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
    if (x >= width) return;
    const size_t i = (size_t)y * width + x;
    const float* r = rays + 6u * i;
    const float ox = r[0], oy = r[1], oz = r[2], dx = r[3], dy = r[4], dz = r[5];
    const int32_t s = hits[2u * i];
    float4 g0, g1;
    if (s < 0) {
        g0 = make_float4(-dx, -dy, -dz, __builtin_inff());
        g1 = make_float4(1.0f, 1.0f, 1.0f, __int_as_float(-1));
    } else {
        const float t = __int_as_float(hits[2u * i + 1u]);
        const float4 sh0 = shade[2u * s], sh1 = shade[2u * s + 1u];
        float nx = ((ox + t * dx) - sh0.x) / sh0.w;
        float ny = ((oy + t * dy) - sh0.y) / sh0.w;
        float nz = ((oz + t * dz) - sh0.z) / sh0.w;
        if (!(__builtin_fmaf(nz, dz, __builtin_fmaf(ny, dy, nx * dx)) <= 0.0f)) { nx = -nx; ny = -ny; nz = -nz; }
        const int32_t ty = mat_ty[s];
        const float a = ty == MRT_DIELECTRIC ? 1.0f : 0.0f;
        const bool coloured = ty == MRT_LAMBERTIAN || ty == MRT_METAL;
        g0 = make_float4(nx, ny, nz, t);
        g1 = make_float4(coloured ? sh1.x : a, coloured ? sh1.y : a, coloured ? sh1.z : a, __int_as_float(s));
    }
    guides[2u * i] = g0;
    guides[2u * i + 1u] = g1;
}

struct AtrousArgs {
    const float4* fb;            // the frame (FIRST: its colour; LAST: its alpha)
    const float* S;              // FIRST: the luminance variance S, var = S * K
    const float4* in;            // not FIRST: (r, g, b, var) of the previous iteration
    const float4* guides;        // 2 per texel
    float4* out;                 // (r, g, b, var), LAST: (r, g, b, alpha of fb)
    uint32_t width, height, step;
    float K;                     // FIRST only; +inf: no luminance stop
    uint32_t lum_stop;           // K finite
    float sigma_l, sigma_z, inv_sigma_a;
    uint32_t normal_exp;
};

// (r, g, b, var) of texel i.  FIRST: var = S * K; without a luminance stop (K = +inf) var = 0 for a finite S (so that 0 * inf
// is never formed) and S itself otherwise (non-finite: the texel passes through).
template <bool FIRST>
__device__ __forceinline__ float4 load_cv(const AtrousArgs& A, size_t i) {
    if (!FIRST) return A.in[i];
    const float4 c = A.fb[i];
    const float s = A.S[i];
    const float var = A.lum_stop ? s * A.K : (__builtin_isfinite(s) ? 0.0f : s);
    return make_float4(c.x, c.y, c.z, var);
}

// g_p of a finite texel p: the {1/4, 1/2, 1/4}^2 mean of var over the 3 x 3 texels around it, rows then columns in increasing
// order, a tap outside the image or not finite skipped (p itself never is).
template <bool FIRST>
__device__ __forceinline__ float prefiltered_var(const AtrousArgs& A, uint32_t x, uint32_t y, float4 cp) {
    const float k3[3] = {0.25f, 0.5f, 0.25f};
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int ty = 0; ty < 3; ty++) {
        const int yq = (int)y + (ty - 1);
        if (yq < 0 || yq >= (int)A.height) continue;
#pragma unroll
        for (int tx = 0; tx < 3; tx++) {
            const int xq = (int)x + (tx - 1);
            if (xq < 0 || xq >= (int)A.width) continue;
            const float kxy = k3[tx] * k3[ty];
            float4 cq = cp;
            if (!(tx == 1 && ty == 1)) {
                cq = load_cv<FIRST>(A, (size_t)yq * A.width + (uint32_t)xq);
                if (!finite4(cq)) continue;
            }
            num = num + kxy * cq.w;
            den = den + kxy;
        }
    }
    return num / den;
}

// The edge stops of a tap q of p that read the guides alone (the luminance stop is the filter's own)
__device__ __forceinline__ float stop_normal(const AtrousArgs& A, float4 gp0, float4 gq0) {
    float wn = fmaxf(0.0f, (gp0.x * gq0.x + gp0.y * gq0.y) + gp0.z * gq0.z);
    for (uint32_t e = 0; e < A.normal_exp; e++) wn = wn * wn;
    return wn;
}
__device__ __forceinline__ float stop_depth(float4 gp0, float4 gq0, bool miss_p, bool miss_q, float inv_z) {
    return miss_p != miss_q ? 0.0f : miss_p ? 1.0f : tukey(fabsf(gp0.w - gq0.w) * inv_z);
}
__device__ __forceinline__ float stop_albedo(const AtrousArgs& A, float4 gp1, float4 gq1) {
    const float da = fmaxf(fmaxf(fabsf(gp1.x - gq1.x), fabsf(gp1.y - gq1.y)), fabsf(gp1.z - gq1.z));
    return tukey(da * A.inv_sigma_a);
}

// The a-trous iteration of pixel (x, y), inside the image.  Taps at offsets {-2..2} x step, rows then columns in increasing
// order, B3-spline weights {1/16, 1/4, 3/8, 1/4, 1/16}; outside the image or not finite: skipped.  The centre tap weighs (3/8)^2
// without stops; any other tap k_x k_y w_lum w_normal w_depth w_albedo, multiplied in that order.  The CENTRE decides on the
// luminance stop (a tap's own is never read).  With `stop`: w_lum is Tukey's weight of the luminance difference over sigma_l
// sqrt(var_p), and a variance of 0 passes the texel through; with PF both read g_p instead of var_p (prefiltered_var: 9 more
// loads, for the centre texel only), while the propagated variance still sums the unfiltered var_q.  Without: w_lum = 1 for all
// its taps, no prefilter, and a variance of 0 does not pass through.  FIRST: the taps are the frame's (load_cv); LAST: the alpha is.
template <bool FIRST, bool PF, bool LAST>
__device__ __forceinline__ void atrous_pixel(const AtrousArgs& A, uint32_t x, uint32_t y, bool stop) {
    const size_t i = (size_t)y * A.width + x;
    const float4 cp = load_cv<FIRST>(A, i);
    float4 res = cp;
    const bool fin = finite4(cp);
    float gv = cp.w;
    if (PF && stop && fin) gv = prefiltered_var<FIRST>(A, x, y, cp);
    // passed through: not finite, or (with a luminance stop) a (prefiltered) variance of 0
    if (fin && !(stop && gv == 0.0f)) {
        const float4 gp0 = A.guides[2u * i], gp1 = A.guides[2u * i + 1u];
        const bool miss_p = __float_as_int(gp1.w) < 0;
        const float lp = lumf(cp.x, cp.y, cp.z);
        const float inv_l = stop ? 1.0f / (A.sigma_l * sqrtf(gv) + 1.0e-6f) : 0.0f;
        const float inv_z = miss_p ? 0.0f : 1.0f / (A.sigma_z * gp0.w);
        const float kern[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
        float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
        const int step = (int)A.step;
#pragma unroll
        for (int ty = 0; ty < 5; ty++) {
            const int yq = (int)y + (ty - 2) * step;
            if (yq < 0 || yq >= (int)A.height) continue;
#pragma unroll
            for (int tx = 0; tx < 5; tx++) {
                const int xq = (int)x + (tx - 2) * step;
                if (xq < 0 || xq >= (int)A.width) continue;
                float w = kern[tx] * kern[ty];
                float4 cq = cp;
                if (!(tx == 2 && ty == 2)) {
                    const size_t q = (size_t)yq * A.width + (uint32_t)xq;
                    cq = load_cv<FIRST>(A, q);
                    if (!finite4(cq)) continue;
                    const float4 gq0 = A.guides[2u * q], gq1 = A.guides[2u * q + 1u];
                    const bool miss_q = __float_as_int(gq1.w) < 0;
                    w = w * (stop ? tukey(fabsf(lp - lumf(cq.x, cq.y, cq.z)) * inv_l) : 1.0f);
                    w = w * stop_normal(A, gp0, gq0);
                    w = w * stop_depth(gp0, gq0, miss_p, miss_q, inv_z);
                    w = w * stop_albedo(A, gp1, gq1);
                }
                sw = sw + w;
                sr = sr + w * cq.x;
                sg = sg + w * cq.y;
                sb = sb + w * cq.z;
                sv = sv + (w * w) * cq.w;
            }
        }
        res = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
    }
    if (LAST) res.w = A.fb[i].w;
    A.out[i] = res;
}

// The entry points of the iteration: grid (ceil(W / 32), ceil(H / 8)), 32 x 8 threads, one pixel per thread.
// The default mode (ACCUMULATED), and every mode without an estimate (K = +inf): the stop is uniform, var = S * K.
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(kTileX * kTileY) atrous_kernel(const AtrousArgs A) {
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    atrous_pixel<FIRST, false, LAST>(A, x, y, A.lum_stop != 0);
}

// PREFILTERED, SPATIAL_EARLY and the temporal image (launched only with a luminance stop): the stop reads g_p.
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(kTileX * kTileY) atrous_prefilter_kernel(const AtrousArgs A) {
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    atrous_pixel<FIRST, true, LAST>(A, x, y, true);
}

// The 7 x 7 weighted variance of the luminance around pixel (x, y) of A.fb: the weights are the filter's own normal, depth and
// albedo stops (the centre's 1); a tap counts if it lies inside the image, its colour is finite and tap_ok(cq, q) says so.  A
// centre whose colour is not finite: 0 (the texel passes through the filter anyway).  Two passes over the taps (the mean, then
// the squares about it): the 49 weights and luminances of the first stay in registers (the loops are fully unrolled, every
// index a constant), so the second pass loads nothing -- recomputing them would cost 49 x 52 more bytes of loads and the stops'
// arithmetic per pixel.  Some 132 VGPRs, no scratch: 3 waves per SIMD.
template <class TapOk>
__device__ __forceinline__ float spatial_estimate(const AtrousArgs& A, uint32_t x, uint32_t y, float4 cp, TapOk tap_ok) {
    if (!finite3(cp)) return 0.0f;
    const size_t i = (size_t)y * A.width + x;
    const float4 gp0 = A.guides[2u * i], gp1 = A.guides[2u * i + 1u];
    const bool miss_p = __float_as_int(gp1.w) < 0;
    const float inv_z = miss_p ? 0.0f : 1.0f / (A.sigma_z * gp0.w);
    float w[49], l[49];
    uint64_t used = 0;
    float m0 = 0.0f, m1 = 0.0f;
#pragma unroll
    for (int ty = 0; ty < 7; ty++) {
#pragma unroll
        for (int tx = 0; tx < 7; tx++) {
            const int t = ty * 7 + tx;
            w[t] = 0.0f;
            l[t] = 0.0f;
            const int yq = (int)y + (ty - 3), xq = (int)x + (tx - 3);
            if (yq < 0 || yq >= (int)A.height || xq < 0 || xq >= (int)A.width) continue;
            float wq, lq;
            if (tx == 3 && ty == 3) {
                wq = 1.0f;
                lq = lumf(cp.x, cp.y, cp.z);
            } else {
                const size_t q = (size_t)yq * A.width + (uint32_t)xq;
                const float4 cq = A.fb[q];
                const bool fin_q = finite3(cq), ok = tap_ok(cq, q);     // (both, always: what tap_ok loads is loaded with the colour)
                if (!(fin_q && ok)) continue;
                const float4 gq0 = A.guides[2u * q], gq1 = A.guides[2u * q + 1u];
                const bool miss_q = __float_as_int(gq1.w) < 0;
                wq = (stop_normal(A, gp0, gq0) * stop_depth(gp0, gq0, miss_p, miss_q, inv_z)) * stop_albedo(A, gp1, gq1);
                lq = lumf(cq.x, cq.y, cq.z);
            }
            w[t] = wq;
            l[t] = lq;
            used |= 1ull << t;
            m0 = m0 + wq;
            m1 = m1 + wq * lq;
        }
    }
    const float mean = m1 / m0;
    float m2 = 0.0f;
#pragma unroll
    for (int t = 0; t < 49; t++) {
        if (!(used >> t & 1ull)) continue;
        const float d = l[t] - mean;
        m2 = m2 + w[t] * (d * d);
    }
    return m2 / m0;
}

// The spatial initial variance of a texel of an accumulation (colour A.fb, luminance variance A.S): the estimate over the taps
// with a finite S; an S that is not finite is kept (the texel passes through).
__device__ __forceinline__ float spatial_initial_variance(const AtrousArgs& A, uint32_t x, uint32_t y, float4 cp, float sp) {
    if (!__builtin_isfinite(sp)) return sp;
    return spatial_estimate(A, x, y, cp, [&A](float4, size_t q) { return __builtin_isfinite(A.S[q]); });
}

// The entry points of the estimate make the field iteration 0 then reads "as the previous iteration's", out = (r, g, b, var).
// Same grid and block as atrous_kernel.  SPATIAL_EARLY while the history is short: every texel takes the estimate.
__global__ void __launch_bounds__(kTileX * kTileY) spatial_variance_kernel(const AtrousArgs A) {
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const size_t i = (size_t)y * A.width + x;
    const float4 cp = A.fb[i];
    A.out[i] = make_float4(cp.x, cp.y, cp.z, spatial_initial_variance(A, x, y, cp, A.S[i]));
}

// The temporal image's field (include/myraytracer_amd.h, "temporal reprojection", 5): A.fb is the history's H0 = (r, g, b, len),
// h1 its H1 = (m1, m2, t, index).  A history of len >= max(2, spatial_len) takes the variance of its own luminance moments.  A
// shorter one -- a disocclusion, the first frames -- takes the estimate over L of the history's colours, a tap counting with
// len >= 1: 49 taps for those pixels alone, so the kernel is divergent by design, and the pixels that pay are the few that just
// restarted.  Any other texel -- len < 1, or short with a colour that is not finite -- gets var 0.
__global__ void __launch_bounds__(kTileX * kTileY) temporal_variance_kernel(const AtrousArgs A, const float4* __restrict__ h1,
                                                                            float min_len) {
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const size_t i = (size_t)y * A.width + x;
    const float4 cp = A.fb[i];
    const float N = cp.w;
    float var = 0.0f;
    if (N >= min_len) {
        const float4 mp = h1[i];
        var = fmaxf(0.0f, mp.y - mp.x * mp.x) / (N - 1.0f);
    } else if (N >= 1.0f) {
        var = spatial_estimate(A, x, y, cp, [](float4 cq, size_t) { return cq.w >= 1.0f; });
    }
    A.out[i] = make_float4(cp.x, cp.y, cp.z, var);
}

// ---- the filter of an adaptive accumulation (include/myraytracer_amd.h, "Adaptive accumulations") ----------------------------
// Every 8 x 8 tile has its own frame count n_t, hence its own K and its own choice between the spatial estimate and S * K.  The
// per-pixel state is read from tile_frames and the K table by both kernels below; it is uniform over a tile, so a wave (32 x 2
// pixels: four tiles) splits at 8-lane granularity at worst.
struct TilePixel {
    bool spatial;               // SPATIAL_EARLY and n_p < spatial_frames: iteration 0's variance is the spatial estimate
    bool stop;                  // spatial, or K_p finite: the centre has a luminance stop (constant over the iterations)
    float K;
};
__device__ __forceinline__ TilePixel tile_pixel(const TileField& T, uint32_t x, uint32_t y) {
    const uint32_t n = T.tile_frames[(size_t)(y / kBandRows) * T.tiles_x + x / kTileW];
    TilePixel s;
    s.K = T.Kf[n];
    s.spatial = T.mode == MRT_DENOISE_VAR_SPATIAL_EARLY && n < T.spatial_frames;
    s.stop = s.spatial || !__builtin_isinf(s.K);
    return s;
}

// The per-tile field.  A pixel of a tile that is still in its spatial phase takes the estimate as spatial_variance_kernel does
// (its taps need a finite colour and S, whatever their own tile's count): 49 taps for those pixels alone, divergent by design, as
// temporal_variance_kernel is.  Any other pixel: S * K_p, or without an estimate (K_p = +inf) 0 for a finite S and S itself
// otherwise.
__global__ void __launch_bounds__(kTileX * kTileY) tile_variance_kernel(const AtrousArgs A, const TileField T) {
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const size_t i = (size_t)y * A.width + x;
    const TilePixel tp = tile_pixel(T, x, y);
    const float4 cp = A.fb[i];
    const float sp = A.S[i];
    float var;
    if (tp.spatial) var = spatial_initial_variance(A, x, y, cp, sp);
    else var = !__builtin_isinf(tp.K) ? sp * tp.K : (__builtin_isfinite(sp) ? 0.0f : sp);
    A.out[i] = make_float4(cp.x, cp.y, cp.z, var);
}

// The iteration's entry point for the per-tile field; PF: PREFILTERED / SPATIAL_EARLY.  Never the first reader of the
// framebuffer: A.in is tile_variance_kernel's field or the previous iteration's output.
template <bool PF, bool LAST>
__global__ void __launch_bounds__(kTileX * kTileY) atrous_tiles_kernel(const AtrousArgs A, const TileField T) {
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    atrous_pixel<false, PF, LAST>(A, x, y, tile_pixel(T, x, y).stop);
}

// ---- the blend of the filtered and the accumulated image (include/myraytracer_amd.h, "Blend with the accumulation") -----------
// One launch behind the last iteration, which has then run as a non-LAST one: f = (colour, propagated variance u) of that
// iteration, c and S the frame's.  A workgroup first makes the record (d^2, n, index bits, valid) of its 32 x 8 pixels and a
// 2-pixel halo -- 36 x 12 records, 6912 bytes of LDS, at most two a thread -- then every pixel sums the 25 records around it from
// LDS and blends.  The halo costs 1.7 x the records' loads (52 bytes a pixel: f, c, S, half a guide), most of them cache hits of
// the neighbouring workgroups'; 25 direct taps would load those 52 bytes 25 times, and a records pass of its own would write and
// read 16 more bytes a pixel through memory and add a launch.  TILES: K per pixel from its tile (T), +inf making it not valid.
struct MixArgs {
    const float4* fb;            // the frame: c, alpha
    const float* S;
    const float4* f;             // the last iteration's (r, g, b, var)
    const float4* guides;
    float4* out;
    uint32_t width, height;
    float K, gain;               // K: not TILES; finite
};
constexpr int kMixR = 2, kMixW = (int)kTileX + 2 * kMixR, kMixH = (int)kTileY + 2 * kMixR;

template <bool TILES>
__global__ void __launch_bounds__(kTileX * kTileY) mix_kernel(const MixArgs A, const TileField T) {
    __shared__ float4 rec[kMixW * kMixH];
    const int x0 = (int)(blockIdx.x * kTileX) - kMixR, y0 = (int)(blockIdx.y * kTileY) - kMixR;
    for (int s = (int)(threadIdx.y * kTileX + threadIdx.x); s < kMixW * kMixH; s += (int)(kTileX * kTileY)) {
        const int xq = x0 + s % kMixW, yq = y0 + s / kMixW;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);         // (w = 0: the tap does not count)
        if (xq >= 0 && xq < (int)A.width && yq >= 0 && yq < (int)A.height) {
            const size_t q = (size_t)yq * A.width + (uint32_t)xq;
            const float4 cq = A.fb[q], fq = A.f[q];
            const float sq = A.S[q];
            const float K = TILES ? tile_pixel(T, (uint32_t)xq, (uint32_t)yq).K : A.K;
            if (finite3(cq) && __builtin_isfinite(sq) && finite4(fq) && !(TILES && __builtin_isinf(K))) {
                const float d = lumf(fq.x, fq.y, fq.z) - lumf(cq.x, cq.y, cq.z);
                r = make_float4(d * d, fmaxf(sq * K - fq.w, 0.0f), A.guides[2u * q + 1u].w, 1.0f);
            }
        }
        rec[s] = r;
    }
    __syncthreads();
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const size_t i = (size_t)y * A.width + x;
    const int at = ((int)threadIdx.y + kMixR) * kMixW + (int)threadIdx.x + kMixR;
    const float4 rp = rec[at], cp = A.fb[i];
    float4 res = A.f[i];                                        // not valid: the filter's own colour
    if (rp.w != 0.0f) {
        float e = 0.0f, m = 0.0f;
#pragma unroll
        for (int dy = -kMixR; dy <= kMixR; dy++) {
#pragma unroll
            for (int dx = -kMixR; dx <= kMixR; dx++) {
                const float4 rq = rec[at + dy * kMixW + dx];
                if (rq.w != 0.0f && __float_as_int(rq.z) == __float_as_int(rp.z)) {
                    e = e + rq.x;
                    m = m + rq.y;
                }
            }
        }
        const float a = e > 0.0f ? fminf(m / (A.gain * e), 1.0f) : 0.0f;
        res.x = cp.x + a * (res.x - cp.x);
        res.y = cp.y + a * (res.y - cp.y);
        res.z = cp.z + a * (res.z - cp.z);
    }
    res.w = cp.w;
    A.out[i] = res;
}

// f(std::bool_constant<a>, std::bool_constant<b>): two run-time flags as the template arguments of a launch
template <class F>
void with_flags(bool a, bool b, F f) {
    if (a && b) f(std::true_type{}, std::true_type{});
    else if (a) f(std::true_type{}, std::false_type{});
    else if (b) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}

}  // namespace

int launch_guide_rays(float* rays, uint32_t width, uint32_t height, const mrt_camera_raw& cam, void* stream) {
    if (width == 0 || height == 0) return 0;
    hipLaunchKernelGGL(guide_rays_kernel, dim3((width + 255) / 256, height), dim3(256), 0, (hipStream_t)stream, rays, width,
                       height, cam);
    return (int)hipGetLastError();
}

int launch_guide_fill(const float* rays, const int32_t* hits, const float* shade, const int32_t* mat_ty, float* guides,
                      uint32_t width, uint32_t height, void* stream) {
    if (width == 0 || height == 0) return 0;
    hipLaunchKernelGGL(guide_fill_kernel, dim3((width + 255) / 256, height), dim3(256), 0, (hipStream_t)stream, rays, hits,
                       reinterpret_cast<const float4*>(shade), mat_ty, reinterpret_cast<float4*>(guides), width);
    return (int)hipGetLastError();
}

int launch_denoise(const DenoiseJob& job, void* stream) {
    const uint32_t width = job.width, height = job.height, n = job.prm.iterations;
    if (width == 0 || height == 0) return 0;
    AtrousArgs A;
    A.fb = reinterpret_cast<const float4*>(job.fb);
    A.S = job.S;
    A.in = nullptr;
    A.guides = reinterpret_cast<const float4*>(job.guides);
    A.width = width; A.height = height; A.step = 1;
    A.K = 0.0f; A.lum_stop = 1u;                // (the uniform source's own below; K is read by an accumulated first iteration alone)
    A.sigma_l = job.prm.sigma_l; A.sigma_z = job.prm.sigma_z;
    A.inv_sigma_a = 1.0f / job.prm.sigma_a;
    A.normal_exp = job.prm.normal_exp;
    const dim3 grid((width + kTileX - 1) / kTileX, (height + kTileY - 1) / kTileY), block(kTileX, kTileY);
    hipStream_t st = (hipStream_t)stream;
    float4* buf[2] = {reinterpret_cast<float4*>(job.ping), reinterpret_cast<float4*>(job.pong)};
    // A field made before iteration 0 goes into pong, where iteration 0 reads it as "the previous iteration's" (and iteration 1
    // writes pong after it); without one, iteration 0 is the first reader of the frame.
    bool field = true, prefilter = true;
    A.out = buf[1];
    switch (job.source) {
    case DenoiseSource::Uniform: {
        const UniformField& u = job.uniform;
        field = u.variance == UniformVariance::Spatial;
        if (!field) {
            A.K = u.K;
            A.lum_stop = !__builtin_isinf(u.K) ? 1u : 0u;
        }
        // without a luminance stop there is nothing to prefilter
        prefilter = u.variance != UniformVariance::Accumulated && A.lum_stop;
        if (field) hipLaunchKernelGGL(spatial_variance_kernel, grid, block, 0, st, A);
        break;
    }
    case DenoiseSource::Temporal: {
        const TemporalField& t = job.temporal;
        const uint32_t min_len = t.spatial_len > 2u ? t.spatial_len : 2u;
        A.fb = reinterpret_cast<const float4*>(t.h0);
        hipLaunchKernelGGL(temporal_variance_kernel, grid, block, 0, st, A, reinterpret_cast<const float4*>(t.h1), (float)min_len);
        A.fb = reinterpret_cast<const float4*>(job.fb);
        break;
    }
    case DenoiseSource::Tiles: {            // an adaptive accumulation: the per-pixel field, then iterations whose centre decides
        const TileField& T = job.tiles;
        if (T.mode > MRT_DENOISE_VAR_SPATIAL_EARLY || !T.tile_frames || !T.Kf || T.tiles_x != (width + kTileW - 1) / kTileW)
            return (int)hipErrorInvalidValue;
        A.lum_stop = 0u;                        // (not read: K and the stop are per pixel)
        prefilter = T.mode != MRT_DENOISE_VAR_ACCUMULATED;
        hipLaunchKernelGGL(tile_variance_kernel, grid, block, 0, st, A, T);
        break;
    }
    default:
        return (int)hipErrorInvalidValue;
    }
    // The blend (job.mix) follows an accumulation's iterations wherever a K is finite: uniformly, or per pixel in the kernel.
    const bool mix = job.mix.enabled && (job.source == DenoiseSource::Tiles ||
                                         (job.source == DenoiseSource::Uniform && !__builtin_isinf(job.uniform.K)));
    for (uint32_t it = 0; it < n; it++) {
        const bool first = it == 0 && !field, last = it + 1 == n && !mix;     // (with the blend no iteration is the LAST one)
        A.step = 1u << it;
        A.in = first ? nullptr : buf[(it + 1) & 1u];
        A.out = last ? reinterpret_cast<float4*>(job.out) : buf[it & 1u];
        if (job.source == DenoiseSource::Tiles)
            with_flags(prefilter, last, [&](auto PF, auto LAST) {
                hipLaunchKernelGGL((atrous_tiles_kernel<decltype(PF)::value, decltype(LAST)::value>), grid, block, 0, st, A, job.tiles);
            });
        else
            with_flags(first, last, [&](auto FIRST, auto LAST) {
                if (prefilter) hipLaunchKernelGGL((atrous_prefilter_kernel<decltype(FIRST)::value, decltype(LAST)::value>), grid, block, 0, st, A);
                else hipLaunchKernelGGL((atrous_kernel<decltype(FIRST)::value, decltype(LAST)::value>), grid, block, 0, st, A);
            });
    }
    if (mix) {                                  // f: where the last iteration wrote as a non-last one
        MixArgs M;
        M.fb = A.fb; M.S = A.S; M.f = buf[(n - 1u) & 1u]; M.guides = A.guides;
        M.out = reinterpret_cast<float4*>(job.out);
        M.width = width; M.height = height;
        M.K = job.uniform.K; M.gain = job.mix.gain;
        if (job.source == DenoiseSource::Tiles) hipLaunchKernelGGL(mix_kernel<true>, grid, block, 0, st, M, job.tiles);
        else hipLaunchKernelGGL(mix_kernel<false>, grid, block, 0, st, M, TileField{});
    }
    return (int)hipGetLastError();
}

}  // namespace mrt
