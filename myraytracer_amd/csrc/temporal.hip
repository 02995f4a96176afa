// Temporal reprojection (include/myraytracer_amd.h, "temporal reprojection"): a per-pixel history of colour and
// luminance moments, carried through the spheres' and the camera's motion.  A hit point rides its sphere, so the motion vector
// is analytic: the first-hit guides hold the sphere index and distance, `shade` the spheres as they are, prev_xyzr the spheres as
// they were at the previous step.  Only + - * /, sqrtf, floorf, fminf, fmaxf and comparisons in a fixed order (-ffp-contract=off),
// so tests/temporal_ref.py restates it bit for bit in float32 numpy.  The variance of the history and the filter over it are
// denoise.hip's (temporal_variance_kernel, launch_denoise's Temporal source).  The response (steps 4b and 4c): a fast
// history H2 carried by the same taps, and temporal_clamp_kernel behind the step; tests/temporal_response_ref.py restates both.
#include <hip/hip_runtime.h>
#include "mrt_internal.h"
#include "rt_math.h"

namespace mrt {
namespace {

constexpr uint32_t kTileX = 32, kTileY = 8;          // one workgroup: 32 x 8 pixels, as the filter's

__device__ __forceinline__ bool finite3(float4 v) {
    return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z);
}

// Steps 1 to 4 for one pixel: the ONE body of both reprojection kernels, as text.  FAST (a literal): the response's fast colour H2
// rides along (the same taps, the same weights; Fx is named only then).  A macro and not an inlined function on purpose: inlined,
// the kernel without the response came out with the operands of some commutative instructions exchanged, and that kernel is
// held to the machine code it always had (scripts/isa_diff.py).
#define MRT_TEMPORAL_REPROJECT_PIXEL(FAST) \
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y; \
    if (x >= A.width || y >= A.height) return; \
    const size_t i = (size_t)y * A.width + x; \
    const float4 cur = reinterpret_cast<const float4*>(A.fb)[i]; \
    const float4 g0 = reinterpret_cast<const float4*>(A.guides)[2u * i], g1 = reinterpret_cast<const float4*>(A.guides)[2u * i + 1u]; \
    const int32_t s = __float_as_int(g1.w); \
    const float t = g0.w; \
    float4* h0_out = reinterpret_cast<float4*>(A.h0_out); \
    float4* h1_out = reinterpret_cast<float4*>(A.h1_out); \
    if (!finite3(cur)) {  /* kept as it is with an empty history: never a tap, passed through by the filter */ \
        h0_out[i] = make_float4(cur.x, cur.y, cur.z, 0.0f); \
        h1_out[i] = make_float4(0.0f, 0.0f, t, g1.w); \
        if (FAST) reinterpret_cast<float4*>(Fx.h2_out)[i] = make_float4(cur.x, cur.y, cur.z, 0.0f); \
        return; \
    } \
    const float* r = A.rays + 6u * i; \
    const float dx = r[3], dy = r[4], dz = r[5]; \
    const bool hit = s >= 0; \
    /* 1. where the point this pixel shows was at the previous step */ \
    float px, py, pz; \
    bool known = true; \
    if (hit) { \
        known = (uint32_t)s < A.n_spheres;  /* (the guides are the library's own: always; keeps the loads in bounds) */ \
        const uint32_t si = known ? (uint32_t)s : 0u; \
        const float4 s1 = reinterpret_cast<const float4*>(A.shade)[2u * si]; \
        const float4 s0 = reinterpret_cast<const float4*>(A.prev_xyzr)[si]; \
        const float X = r[0] + t * dx, Y = r[1] + t * dy, Z = r[2] + t * dz; \
        const float k = s0.w / s1.w; \
        px = s0.x + (X - s1.x) * k; \
        py = s0.y + (Y - s1.y) * k; \
        pz = s0.z + (Z - s1.z) * k; \
    } else { \
        px = A.o_prev[0] + dx; \
        py = A.o_prev[1] + dy; \
        pz = A.o_prev[2] + dz; \
    } \
    /* 2. the previous camera's pixel of that point */ \
    const float vx = px - A.o_prev[0], vy = py - A.o_prev[1], vz = pz - A.o_prev[2]; \
    const float a = (A.M[0] * vx + A.M[1] * vy) + A.M[2] * vz; \
    const float b = (A.M[3] * vx + A.M[4] * vy) + A.M[5] * vz; \
    const float l = (A.M[6] * vx + A.M[7] * vy) + A.M[8] * vz; \
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, s1m = 0.0f, s2m = 0.0f, lmin = __builtin_inff(); \
    float fr = 0.0f, fg = 0.0f, fb = 0.0f;  /* FAST: sf */ \
    if (known && l > 0.0f) { \
        const float Wf = (float)A.width, Hf = (float)A.height; \
        const float fx = (a / l) * (0.5f * Hf) + (0.5f * Wf - 1.0f); \
        const float fy = (b / l) * (0.5f * Hf) + (0.5f * Hf - 1.0f); \
        const float te = sqrtf((vx * vx + vy * vy) + vz * vz); \
        const float tol = A.depth_tol * te; \
        /* 3. the four taps around it, j then i */ \
        const float x0 = floorf(fx), y0 = floorf(fy); \
        const float wx = fx - x0, wy = fy - y0; \
        const float4* h0_in = reinterpret_cast<const float4*>(A.h0_in); \
        const float4* h1_in = reinterpret_cast<const float4*>(A.h1_in); \
_Pragma("unroll") \
        for (int j = 0; j < 2; j++) { \
_Pragma("unroll") \
            for (int ii = 0; ii < 2; ii++) { \
                const float xq = x0 + (float)ii, yq = y0 + (float)j; \
                /* (compared as floats: a NaN or a position beyond the int range is outside) */ \
                if (!(xq >= 0.0f && xq < Wf && yq >= 0.0f && yq < Hf)) continue; \
                const float bw = (ii ? wx : 1.0f - wx) * (j ? wy : 1.0f - wy); \
                if (!(bw > 0.0f)) continue; \
                const size_t q = (size_t)(uint32_t)yq * A.width + (uint32_t)xq; \
                const float4 q0 = h0_in[q]; \
                if (!(q0.w >= 1.0f) || !finite3(q0)) continue; \
                const float4 q1 = h1_in[q]; \
                if (__float_as_int(q1.w) != s) continue; \
                if (hit && !(fabsf(q1.z - te) <= tol)) continue; \
                sw = sw + bw; \
                sr = sr + bw * q0.x; \
                sg = sg + bw * q0.y; \
                sb = sb + bw * q0.z; \
                s1m = s1m + bw * q1.x; \
                s2m = s2m + bw * q1.y; \
                lmin = fminf(lmin, q0.w); \
                if (FAST) { \
                    const float4 q2 = reinterpret_cast<const float4*>(Fx.h2_in)[q]; \
                    fr = fr + bw * q2.x; \
                    fg = fg + bw * q2.y; \
                    fb = fb + bw * q2.z; \
                } \
            } \
        } \
    } \
    /* 4. the newest frame blended into what was found */ \
    const float Lc = lumf(cur.x, cur.y, cur.z); \
    float4 o0 = make_float4(cur.x, cur.y, cur.z, 1.0f); \
    float m1 = Lc, m2 = Lc * Lc; \
    float4 o2 = make_float4(cur.x, cur.y, cur.z, 1.0f); \
    if (sw > 0.0f) { \
        const float cr = sr / sw, cg = sg / sw, cb = sb / sw, m1p = s1m / sw, m2p = s2m / sw; \
        const float N = fminf(lmin + 1.0f, A.max_history); \
        const float alpha = 1.0f / N; \
        o0 = make_float4(cr + alpha * (cur.x - cr), cg + alpha * (cur.y - cg), cb + alpha * (cur.z - cb), N); \
        m1 = m1p + alpha * (Lc - m1p); \
        m2 = m2p + alpha * (Lc * Lc - m2p); \
        if (FAST) { \
            const float pr = fr / sw, pg = fg / sw, pb = fb / sw; \
            const float af = 1.0f / fminf(N, Fx.fast_history); \
            o2 = make_float4(pr + af * (cur.x - pr), pg + af * (cur.y - pg), pb + af * (cur.z - pb), 1.0f); \
        } \
    } \
    h0_out[i] = o0; \
    h1_out[i] = make_float4(m1, m2, t, g1.w); \
    if (FAST) reinterpret_cast<float4*>(Fx.h2_out)[i] = o2;

// grid (ceil(W / 32), ceil(H / 8)), 32 x 8 threads; one pixel per thread.  Per pixel 72 B of inputs (the framebuffer texel, the
// guide ray, the guide record), two 16-B sphere records on a hit, up to four 32-B history taps (neighbouring pixels share them:
// they come from L2) and 32 B written.  Reads h0_in / h1_in, writes h0_out / h1_out: never the same buffers.
__global__ void __launch_bounds__(kTileX * kTileY) temporal_reproject_kernel(const TemporalArgs A) {
    const TemporalFastArgs Fx{nullptr, nullptr, 0.0f};       // (named by the body, never read)
    MRT_TEMPORAL_REPROJECT_PIXEL(false)
}

// ... and with the response on: four 16-B taps of H2 more (through L2, as the others) and 16 B more written, h2_in -> h2_out
__global__ void __launch_bounds__(kTileX * kTileY) temporal_reproject_fast_kernel(const TemporalArgs A, const TemporalFastArgs Fx) {
    MRT_TEMPORAL_REPROJECT_PIXEL(true)
}

// Steps 4b and 4c: the long history's colour clamped to the fast history's local statistics, its length pulled towards the fast
// one where the clamp acted.  The same 32 x 8 tiles.  The tile and its 2-texel halo -- 36 x 12 texels of H2' with "counts so far"
// (inside the image, valid == 1, a finite colour) folded into .w, and the index bits of H1' -- are staged in LDS (8,640 B); each
// thread then walks the 5 x 5 window there, dy then dx.  It reads and writes H0' of its own pixel only, so it runs in place on
// the step's output: nothing it writes is read by another thread.
constexpr int kHalo = 2, kLdsX = (int)kTileX + 2 * kHalo, kLdsY = (int)kTileY + 2 * kHalo;

__global__ void __launch_bounds__(kTileX * kTileY) temporal_clamp_kernel(const TemporalClampArgs A) {
    __shared__ float4 lds_f[kLdsY * kLdsX];
    __shared__ int32_t lds_s[kLdsY * kLdsX];
    const int bx = (int)(blockIdx.x * kTileX), by = (int)(blockIdx.y * kTileY);
    const float4* h2 = reinterpret_cast<const float4*>(A.h2);
    for (int k = (int)(threadIdx.y * kTileX + threadIdx.x); k < kLdsY * kLdsX; k += (int)(kTileX * kTileY)) {
        const int gx = bx + k % kLdsX - kHalo, gy = by + k / kLdsX - kHalo;
        float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        int32_t sq = 0;
        if (gx >= 0 && gx < (int)A.width && gy >= 0 && gy < (int)A.height) {
            const size_t q = (size_t)gy * A.width + (size_t)gx;
            f = h2[q];
            f.w = (f.w == 1.0f && finite3(f)) ? 1.0f : 0.0f;
            sq = __float_as_int(A.h1[4u * q + 3u]);
        }
        lds_f[k] = f;
        lds_s[k] = sq;
    }
    __syncthreads();
    const uint32_t x = (uint32_t)bx + threadIdx.x, y = (uint32_t)by + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const size_t i = (size_t)y * A.width + x;
    float4* h0 = reinterpret_cast<float4*>(A.h0);
    const float4 c = h0[i];
    if (!(c.w >= 2.0f)) return;             // found no history: nothing to clamp
    const int centre = ((int)threadIdx.y + kHalo) * kLdsX + (int)threadIdx.x + kHalo;
    const int32_t s = lds_s[centre];
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, br = 0.0f, bg = 0.0f, bb = 0.0f, n = 0.0f;
#pragma unroll
    for (int dy = -kHalo; dy <= kHalo; dy++) {
#pragma unroll
        for (int dx = -kHalo; dx <= kHalo; dx++) {
            const float4 f = lds_f[centre + dy * kLdsX + dx];
            const bool cnt = f.w == 1.0f && lds_s[centre + dy * kLdsX + dx] == s;
            // (a tap that does not count adds +0: the sums, which start at +0, keep their bits)
            ar = ar + (cnt ? f.x : 0.0f);
            ag = ag + (cnt ? f.y : 0.0f);
            ab = ab + (cnt ? f.z : 0.0f);
            br = br + (cnt ? f.x * f.x : 0.0f);
            bg = bg + (cnt ? f.y * f.y : 0.0f);
            bb = bb + (cnt ? f.z * f.z : 0.0f);
            n = n + (cnt ? 1.0f : 0.0f);
        }
    }
    if (!(n >= 2.0f)) return;
    const float mr = ar / n, mg = ag / n, mb = ab / n;
    const float er = A.clamp_sigma * sqrtf(fmaxf(0.0f, br / n - mr * mr));
    const float eg = A.clamp_sigma * sqrtf(fmaxf(0.0f, bg / n - mg * mg));
    const float eb = A.clamp_sigma * sqrtf(fmaxf(0.0f, bb / n - mb * mb));
    const float cr = fminf(fmaxf(c.x, mr - er), mr + er);
    const float cg = fminf(fmaxf(c.y, mg - eg), mg + eg);
    const float cb = fminf(fmaxf(c.z, mb - eb), mb + eb);
    // 4c. anti-lag: how far the clamp moved the colour, in box half-widths
    const float d = fmaxf(fmaxf(fabsf(cr - c.x), fabsf(cg - c.y)), fabsf(cb - c.z));
    const float emax = fmaxf(fmaxf(er, eg), eb);
    const float r = fminf(1.0f, d / (emax + 1e-6f));
    const float N = c.w;
    h0[i] = make_float4(cr, cg, cb, N + (A.antilag * r) * (fminf(N, A.fast_history) - N));
}

// "previous" for the next step: the spheres' (cx, cy, cz, r) as they are now (floats 0..3 of the 8 of `shade`)
__global__ void __launch_bounds__(256) temporal_snapshot_kernel(const float4* __restrict__ shade, float4* __restrict__ prev_xyzr,
                                                                uint32_t n_spheres) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_spheres) prev_xyzr[i] = shade[2u * i];
}

}  // namespace

int launch_temporal_reproject(const TemporalArgs& a, void* stream) {
    if (a.width == 0 || a.height == 0) return 0;
    const dim3 grid((a.width + kTileX - 1) / kTileX, (a.height + kTileY - 1) / kTileY), block(kTileX, kTileY);
    hipLaunchKernelGGL(temporal_reproject_kernel, grid, block, 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_temporal_reproject_fast(const TemporalArgs& a, const TemporalFastArgs& f, void* stream) {
    if (a.width == 0 || a.height == 0) return 0;
    const dim3 grid((a.width + kTileX - 1) / kTileX, (a.height + kTileY - 1) / kTileY), block(kTileX, kTileY);
    hipLaunchKernelGGL(temporal_reproject_fast_kernel, grid, block, 0, (hipStream_t)stream, a, f);
    return (int)hipGetLastError();
}

int launch_temporal_clamp(const TemporalClampArgs& a, void* stream) {
    if (a.width == 0 || a.height == 0) return 0;
    const dim3 grid((a.width + kTileX - 1) / kTileX, (a.height + kTileY - 1) / kTileY), block(kTileX, kTileY);
    hipLaunchKernelGGL(temporal_clamp_kernel, grid, block, 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_temporal_snapshot(const float* shade, float* prev_xyzr, uint32_t n_spheres, void* stream) {
    if (n_spheres == 0) return 0;
    hipLaunchKernelGGL(temporal_snapshot_kernel, dim3((n_spheres + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(shade), reinterpret_cast<float4*>(prev_xyzr), n_spheres);
    return (int)hipGetLastError();
}

}  // namespace mrt
