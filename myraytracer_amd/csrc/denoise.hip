// The denoiser (include/myraytracer_amd.h, "denoiser"): first-hit guide buffers and a variance-guided,
// edge-aware a-trous filter over the framebuffer (the spatial filter of SVGF without its temporal part: the accumulation is
// the temporal part; a moving scene's is temporal.hip, whose history the same iterations filter).  A translation unit of its own, outside the render path's (kernels.hip).
//
// Guides (once per camera / scene): guide_rays_kernel writes one ray per pixel through the mean of the render's sample
// positions; the closest hits come from the DBG instantiation of render_kernel (launch_debug_world_hit, no candidate bitmap);
// guide_fill_kernel turns them into the per-texel record the filter reads.
// Filter: atrous_kernel, one launch per iteration, colour and variance ping-ponged as one float4; with a variance mode
// (mrt_set_denoise_variance) atrous_prefilter_kernel instead, behind spatial_variance_kernel while the history is short.  Only + - * /, sqrtf, fminf,
// fmaxf in a fixed order (-ffp-contract=off; hipcc's `/` and sqrtf are correctly rounded), so tests/denoise_ref.py restates it
// bit for bit in float32 numpy.
#include <hip/hip_runtime.h>
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
__device__ __forceinline__ bool finite4(float4 v) {
    return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z) && __builtin_isfinite(v.w);
}

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

// grid (ceil(W / 32), ceil(H / 8)), 32 x 8 threads; one pixel per thread.  Taps at offsets {-2..2} x step, rows then columns in
// increasing order, B3-spline weights {1/16, 1/4, 3/8, 1/4, 1/16}; outside the image or not finite: skipped.  The centre tap
// weighs (3/8)^2 without stops; any other tap k_x k_y w_lum w_normal w_depth w_albedo, multiplied in that order.
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(kTileX * kTileY) atrous_kernel(const AtrousArgs A) {
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const size_t i = (size_t)y * A.width + x;
    const float4 cp = load_cv<FIRST>(A, i);
    float4 res = cp;
    // passed through: not finite, or (with a luminance stop) a variance of 0
    if (finite4(cp) && !(A.lum_stop && cp.w == 0.0f)) {
        const float4 gp0 = A.guides[2u * i], gp1 = A.guides[2u * i + 1u];
        const bool miss_p = __float_as_int(gp1.w) < 0;
        const float lp = lumf(cp.x, cp.y, cp.z);
        const float inv_l = A.lum_stop ? 1.0f / (A.sigma_l * sqrtf(cp.w) + 1.0e-6f) : 0.0f;
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
                const float kxy = kern[tx] * kern[ty];
                float w;
                float4 cq;
                if (tx == 2 && ty == 2) {
                    cq = cp;
                    w = kxy;
                } else {
                    const size_t q = (size_t)yq * A.width + (uint32_t)xq;
                    cq = load_cv<FIRST>(A, q);
                    if (!finite4(cq)) continue;
                    const float4 gq0 = A.guides[2u * q], gq1 = A.guides[2u * q + 1u];
                    const bool miss_q = __float_as_int(gq1.w) < 0;
                    const float wl = A.lum_stop ? tukey(fabsf(lp - lumf(cq.x, cq.y, cq.z)) * inv_l) : 1.0f;
                    float wn = fmaxf(0.0f, (gp0.x * gq0.x + gp0.y * gq0.y) + gp0.z * gq0.z);
                    for (uint32_t e = 0; e < A.normal_exp; e++) wn = wn * wn;
                    const float wz = miss_p != miss_q ? 0.0f : miss_p ? 1.0f : tukey(fabsf(gp0.w - gq0.w) * inv_z);
                    const float da = fmaxf(fmaxf(fabsf(gp1.x - gq1.x), fabsf(gp1.y - gq1.y)), fabsf(gp1.z - gq1.z));
                    const float wa = tukey(da * A.inv_sigma_a);
                    w = kxy * wl;
                    w = w * wn;
                    w = w * wz;
                    w = w * wa;
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

// The edge stops of a tap q of p, as atrous_kernel forms them (for the kernels of the variance modes below; atrous_kernel keeps
// its own text, so that the default mode's four instantiations stay the same instructions).
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

// The prefiltering a-trous iteration (PREFILTERED, SPATIAL_EARLY; launched only with a luminance stop): atrous_kernel, except
// that the luminance stop and the pass-through rule read g_p (prefiltered_var: 9 more loads, for the centre texel only).  The
// propagated variance still sums the unfiltered var_q.
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(kTileX * kTileY) atrous_prefilter_kernel(const AtrousArgs A) {
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const size_t i = (size_t)y * A.width + x;
    const float4 cp = load_cv<FIRST>(A, i);
    float4 res = cp;
    const float gv = finite4(cp) ? prefiltered_var<FIRST>(A, x, y, cp) : 0.0f;
    // passed through: not finite, or a prefiltered variance of 0
    if (finite4(cp) && gv != 0.0f) {
        const float4 gp0 = A.guides[2u * i], gp1 = A.guides[2u * i + 1u];
        const bool miss_p = __float_as_int(gp1.w) < 0;
        const float lp = lumf(cp.x, cp.y, cp.z);
        const float inv_l = 1.0f / (A.sigma_l * sqrtf(gv) + 1.0e-6f);
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
                    w = w * tukey(fabsf(lp - lumf(cq.x, cq.y, cq.z)) * inv_l);
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

// The spatial initial variance (SPATIAL_EARLY while the history is short): per texel the weighted variance of the luminance over
// the 7 x 7 window, the weights the filter's own normal, depth and albedo stops (the centre's 1); out = (r, g, b, var), which the
// first a-trous iteration then reads as a non-first one.  Same grid and block as atrous_kernel.  Two passes over the taps (the
// mean, then the squares about it): the 49 weights and luminances of the first stay in registers (the loops are fully unrolled,
// every index a constant), so the second pass loads nothing -- recomputing them would cost 49 x 52 more bytes of loads and the
// stops' arithmetic per pixel.  132 VGPRs, no scratch: 3 waves per SIMD.
__global__ void __launch_bounds__(kTileX * kTileY) spatial_variance_kernel(const AtrousArgs A) {
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const size_t i = (size_t)y * A.width + x;
    const float4 cp = A.fb[i];
    const float sp = A.S[i];
    float var = sp;                             // S not finite: kept (the texel passes through)
    if (__builtin_isfinite(sp)) {
        var = 0.0f;                             // a colour that is not finite: passes through as well
        if (__builtin_isfinite(cp.x) && __builtin_isfinite(cp.y) && __builtin_isfinite(cp.z)) {
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
                        const float sq = A.S[q];
                        if (!(__builtin_isfinite(cq.x) && __builtin_isfinite(cq.y) && __builtin_isfinite(cq.z) && __builtin_isfinite(sq)))
                            continue;
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
            var = m2 / m0;
        }
    }
    A.out[i] = make_float4(cp.x, cp.y, cp.z, var);
}

template <bool PF>
void launch_atrous(bool first, bool last, dim3 grid, dim3 block, hipStream_t st, const AtrousArgs& A) {
    if (PF) {
        if (first && last) hipLaunchKernelGGL((atrous_prefilter_kernel<true, true>), grid, block, 0, st, A);
        else if (first) hipLaunchKernelGGL((atrous_prefilter_kernel<true, false>), grid, block, 0, st, A);
        else if (last) hipLaunchKernelGGL((atrous_prefilter_kernel<false, true>), grid, block, 0, st, A);
        else hipLaunchKernelGGL((atrous_prefilter_kernel<false, false>), grid, block, 0, st, A);
    } else {
        if (first && last) hipLaunchKernelGGL((atrous_kernel<true, true>), grid, block, 0, st, A);
        else if (first) hipLaunchKernelGGL((atrous_kernel<true, false>), grid, block, 0, st, A);
        else if (last) hipLaunchKernelGGL((atrous_kernel<false, true>), grid, block, 0, st, A);
        else hipLaunchKernelGGL((atrous_kernel<false, false>), grid, block, 0, st, A);
    }
}

// The temporal image's field (variance 3; include/myraytracer_amd.h, "temporal reprojection", 5): A.fb is the history's H0 =
// (r, g, b, len), h1 its H1 = (m1, m2, t, index); out = (r, g, b, var).  A history of len >= max(2, spatial_len) takes the variance
// of its own luminance moments.  A shorter one -- a disocclusion, the first frames -- takes spatial_variance_kernel's estimate
// over L of the history's colours, "S finite" read as len >= 1: 49 taps for those pixels alone, so the kernel is divergent by
// design, and the pixels that pay are the few that just restarted.  Any other texel -- len < 1, or short with a colour that is
// not finite -- gets var 0.
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
    } else if (N >= 1.0f && __builtin_isfinite(cp.x) && __builtin_isfinite(cp.y) && __builtin_isfinite(cp.z)) {
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
                    if (!(__builtin_isfinite(cq.x) && __builtin_isfinite(cq.y) && __builtin_isfinite(cq.z) && cq.w >= 1.0f))
                        continue;
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
        var = m2 / m0;
    }
    A.out[i] = make_float4(cp.x, cp.y, cp.z, var);
}

// ---- the filter of an adaptive accumulation (include/myraytracer_amd.h, "Adaptive accumulations") ----------------------------
// Every 8 x 8 tile has its own frame count n_t, hence its own K and its own choice between the spatial estimate and S * K.  The
// per-pixel state is read from tile_frames and the K table by every kernel below; it is uniform over a tile, so a wave (32 x 2
// pixels: four tiles) splits at 8-lane granularity at worst.  Kernels of their own: the uniform path's keep their text.
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

// The field iteration 0 reads "as the previous iteration's": out = (r, g, b, var0).  A pixel of a tile that is still in its
// spatial phase takes spatial_variance_kernel's estimate (its taps need a finite colour and S, whatever their own tile's count):
// 49 taps for those pixels alone, divergent by design, as temporal_variance_kernel is.  Any other pixel: S * K_p, or without an
// estimate (K_p = +inf) 0 for a finite S and S itself otherwise.
__global__ void __launch_bounds__(kTileX * kTileY) tile_variance_kernel(const AtrousArgs A, const TileField T) {
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const size_t i = (size_t)y * A.width + x;
    const TilePixel tp = tile_pixel(T, x, y);
    const float4 cp = A.fb[i];
    const float sp = A.S[i];
    float var;
    if (!tp.spatial) {
        var = !__builtin_isinf(tp.K) ? sp * tp.K : (__builtin_isfinite(sp) ? 0.0f : sp);
    } else {
        var = sp;                               // S not finite: kept (the texel passes through)
        if (__builtin_isfinite(sp)) {
            var = 0.0f;                         // a colour that is not finite: passes through as well
            if (__builtin_isfinite(cp.x) && __builtin_isfinite(cp.y) && __builtin_isfinite(cp.z)) {
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
                            const float sq = A.S[q];
                            if (!(__builtin_isfinite(cq.x) && __builtin_isfinite(cq.y) && __builtin_isfinite(cq.z) && __builtin_isfinite(sq)))
                                continue;
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
                var = m2 / m0;
            }
        }
    }
    A.out[i] = make_float4(cp.x, cp.y, cp.z, var);
}

// An a-trous iteration whose CENTRE decides (a tap's own stop is never read).  A centre with a stop: atrous_kernel's luminance
// stop and pass-through rule, with PF (PREFILTERED / SPATIAL_EARLY) on g_p as in atrous_prefilter_kernel.  A centre without
// one: w_lum = 1 for all its taps, no prefilter, and a variance of 0 does not pass through.  Never the first reader of the
// framebuffer: A.in is tile_variance_kernel's field or the previous iteration's output.
template <bool PF, bool LAST>
__global__ void __launch_bounds__(kTileX * kTileY) atrous_tiles_kernel(const AtrousArgs A, const TileField T) {
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const size_t i = (size_t)y * A.width + x;
    const bool stop = tile_pixel(T, x, y).stop;
    const float4 cp = A.in[i];
    float4 res = cp;
    const bool fin = finite4(cp);
    float gv = cp.w;
    if (PF && stop && fin) gv = prefiltered_var<false>(A, x, y, cp);
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
                    cq = A.in[q];
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

int launch_denoise(const float* fb, const float* S, float K, const float* guides, float* ping, float* pong, float* out,
                   uint32_t width, uint32_t height, const mrt_denoise_params& prm, uint32_t variance, void* stream,
                   const TemporalField* temporal, const TileField* tiles) {
    if (width == 0 || height == 0) return 0;
    if ((variance == 3) != (temporal != nullptr) || (tiles && temporal)) return (int)hipErrorInvalidValue;
    const bool spatial = variance >= 2;         // (iteration 0 reads a field made before it: the spatial estimate's, the history's)
    AtrousArgs A;
    A.fb = reinterpret_cast<const float4*>(fb);
    A.S = S;
    A.in = nullptr;
    A.guides = reinterpret_cast<const float4*>(guides);
    A.width = width; A.height = height; A.step = 1;
    A.K = spatial ? 0.0f : K;
    A.lum_stop = spatial || !__builtin_isinf(K) ? 1u : 0u;
    A.sigma_l = prm.sigma_l; A.sigma_z = prm.sigma_z;
    A.inv_sigma_a = 1.0f / prm.sigma_a;
    A.normal_exp = prm.normal_exp;
    const dim3 grid((width + kTileX - 1) / kTileX, (height + kTileY - 1) / kTileY), block(kTileX, kTileY);
    hipStream_t st = (hipStream_t)stream;
    float4* buf[2] = {reinterpret_cast<float4*>(ping), reinterpret_cast<float4*>(pong)};
    if (tiles) {            // an adaptive accumulation: the per-pixel field into pong, then iterations whose centre decides
        if (tiles->mode > MRT_DENOISE_VAR_SPATIAL_EARLY || !tiles->tile_frames || !tiles->Kf ||
            tiles->tiles_x != (width + kTileW - 1) / kTileW)
            return (int)hipErrorInvalidValue;
        A.K = 0.0f; A.lum_stop = 0u;            // (not read: K and the stop are per pixel)
        A.out = buf[1];
        hipLaunchKernelGGL(tile_variance_kernel, grid, block, 0, st, A, *tiles);
        const bool pf = tiles->mode != MRT_DENOISE_VAR_ACCUMULATED;
        for (uint32_t it = 0; it < prm.iterations; it++) {
            const bool last = it + 1 == prm.iterations;
            A.step = 1u << it;
            A.in = buf[(it + 1) & 1u];
            A.out = last ? reinterpret_cast<float4*>(out) : buf[it & 1u];
            if (pf && last) hipLaunchKernelGGL((atrous_tiles_kernel<true, true>), grid, block, 0, st, A, *tiles);
            else if (pf) hipLaunchKernelGGL((atrous_tiles_kernel<true, false>), grid, block, 0, st, A, *tiles);
            else if (last) hipLaunchKernelGGL((atrous_tiles_kernel<false, true>), grid, block, 0, st, A, *tiles);
            else hipLaunchKernelGGL((atrous_tiles_kernel<false, false>), grid, block, 0, st, A, *tiles);
        }
        return (int)hipGetLastError();
    }
    // without a luminance stop there is nothing to prefilter: today's kernels
    const bool prefilter = variance != 0 && A.lum_stop;
    if (spatial) {          // into pong, where iteration 0 reads it as "the previous iteration's" (and iteration 1 writes pong after it)
        A.out = buf[1];
        if (temporal) {
            const uint32_t min_len = temporal->spatial_len > 2u ? temporal->spatial_len : 2u;
            A.fb = reinterpret_cast<const float4*>(temporal->h0);
            hipLaunchKernelGGL(temporal_variance_kernel, grid, block, 0, st, A, reinterpret_cast<const float4*>(temporal->h1), (float)min_len);
            A.fb = reinterpret_cast<const float4*>(fb);
        } else {
            hipLaunchKernelGGL(spatial_variance_kernel, grid, block, 0, st, A);
        }
    }
    const uint32_t n = prm.iterations;
    for (uint32_t it = 0; it < n; it++) {
        const bool first = it == 0 && !spatial, last = it + 1 == n;
        A.step = 1u << it;
        A.in = first ? nullptr : buf[(it + 1) & 1u];
        A.out = last ? reinterpret_cast<float4*>(out) : buf[it & 1u];
        if (prefilter) launch_atrous<true>(first, last, grid, block, st, A);
        else launch_atrous<false>(first, last, grid, block, st, A);
    }
    return (int)hipGetLastError();
}

}  // namespace mrt
