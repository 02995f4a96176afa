// Temporal reprojection (include/myraytracer_amd.h, "temporal reprojection"): a per-pixel history of colour and
// luminance moments, carried through the spheres' and the camera's motion.  A hit point rides its sphere, so the motion vector
// is analytic: the first-hit guides hold the sphere index and distance, `shade` the spheres as they are, prev_xyzr the spheres as
// they were at the previous step.  Only + - * /, sqrtf, floorf, fminf, fmaxf and comparisons in a fixed order (-ffp-contract=off),
// so tests/temporal_ref.py restates it bit for bit in float32 numpy.  The variance of the history and the filter over it are
// denoise.hip's (temporal_variance_kernel, launch_denoise's variance 3).
#include <hip/hip_runtime.h>
#include "mrt_internal.h"
#include "rt_math.h"

namespace mrt {
namespace {

constexpr uint32_t kTileX = 32, kTileY = 8;          // one workgroup: 32 x 8 pixels, as the filter's

__device__ __forceinline__ bool finite3(float4 v) {
    return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z);
}

// grid (ceil(W / 32), ceil(H / 8)), 32 x 8 threads; one pixel per thread.  Per pixel 72 B of inputs (the framebuffer texel, the
// guide ray, the guide record), two 16-B sphere records on a hit, up to four 32-B history taps (neighbouring pixels share them:
// they come from L2) and 32 B written.  Reads h0_in / h1_in, writes h0_out / h1_out: never the same buffers.
__global__ void __launch_bounds__(kTileX * kTileY) temporal_reproject_kernel(const TemporalArgs A) {
    const uint32_t x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= A.width || y >= A.height) return;
    const size_t i = (size_t)y * A.width + x;
    const float4 cur = reinterpret_cast<const float4*>(A.fb)[i];
    const float4 g0 = reinterpret_cast<const float4*>(A.guides)[2u * i], g1 = reinterpret_cast<const float4*>(A.guides)[2u * i + 1u];
    const int32_t s = __float_as_int(g1.w);
    const float t = g0.w;
    float4* h0_out = reinterpret_cast<float4*>(A.h0_out);
    float4* h1_out = reinterpret_cast<float4*>(A.h1_out);
    if (!finite3(cur)) {                    // kept as it is with an empty history: never a tap, passed through by the filter
        h0_out[i] = make_float4(cur.x, cur.y, cur.z, 0.0f);
        h1_out[i] = make_float4(0.0f, 0.0f, t, g1.w);
        return;
    }
    const float* r = A.rays + 6u * i;
    const float dx = r[3], dy = r[4], dz = r[5];
    const bool hit = s >= 0;
    // 1. where the point this pixel shows was at the previous step
    float px, py, pz;
    bool known = true;
    if (hit) {
        known = (uint32_t)s < A.n_spheres;          // (the guides are the library's own: always; keeps the loads in bounds)
        const uint32_t si = known ? (uint32_t)s : 0u;
        const float4 s1 = reinterpret_cast<const float4*>(A.shade)[2u * si];
        const float4 s0 = reinterpret_cast<const float4*>(A.prev_xyzr)[si];
        const float X = r[0] + t * dx, Y = r[1] + t * dy, Z = r[2] + t * dz;
        const float k = s0.w / s1.w;
        px = s0.x + (X - s1.x) * k;
        py = s0.y + (Y - s1.y) * k;
        pz = s0.z + (Z - s1.z) * k;
    } else {
        px = A.o_prev[0] + dx;
        py = A.o_prev[1] + dy;
        pz = A.o_prev[2] + dz;
    }
    // 2. the previous camera's pixel of that point
    const float vx = px - A.o_prev[0], vy = py - A.o_prev[1], vz = pz - A.o_prev[2];
    const float a = (A.M[0] * vx + A.M[1] * vy) + A.M[2] * vz;
    const float b = (A.M[3] * vx + A.M[4] * vy) + A.M[5] * vz;
    const float l = (A.M[6] * vx + A.M[7] * vy) + A.M[8] * vz;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, s1m = 0.0f, s2m = 0.0f, lmin = __builtin_inff();
    if (known && l > 0.0f) {
        const float Wf = (float)A.width, Hf = (float)A.height;
        const float fx = (a / l) * (0.5f * Hf) + (0.5f * Wf - 1.0f);
        const float fy = (b / l) * (0.5f * Hf) + (0.5f * Hf - 1.0f);
        const float te = sqrtf((vx * vx + vy * vy) + vz * vz);
        const float tol = A.depth_tol * te;
        // 3. the four taps around it, j then i
        const float x0 = floorf(fx), y0 = floorf(fy);
        const float wx = fx - x0, wy = fy - y0;
        const float4* h0_in = reinterpret_cast<const float4*>(A.h0_in);
        const float4* h1_in = reinterpret_cast<const float4*>(A.h1_in);
#pragma unroll
        for (int j = 0; j < 2; j++) {
#pragma unroll
            for (int ii = 0; ii < 2; ii++) {
                const float xq = x0 + (float)ii, yq = y0 + (float)j;
                // (compared as floats: a NaN or a position beyond the int range is outside)
                if (!(xq >= 0.0f && xq < Wf && yq >= 0.0f && yq < Hf)) continue;
                const float bw = (ii ? wx : 1.0f - wx) * (j ? wy : 1.0f - wy);
                if (!(bw > 0.0f)) continue;
                const size_t q = (size_t)(uint32_t)yq * A.width + (uint32_t)xq;
                const float4 q0 = h0_in[q];
                if (!(q0.w >= 1.0f) || !finite3(q0)) continue;
                const float4 q1 = h1_in[q];
                if (__float_as_int(q1.w) != s) continue;
                if (hit && !(fabsf(q1.z - te) <= tol)) continue;
                sw = sw + bw;
                sr = sr + bw * q0.x;
                sg = sg + bw * q0.y;
                sb = sb + bw * q0.z;
                s1m = s1m + bw * q1.x;
                s2m = s2m + bw * q1.y;
                lmin = fminf(lmin, q0.w);
            }
        }
    }
    // 4. the newest frame blended into what was found
    const float Lc = lumf(cur.x, cur.y, cur.z);
    float4 o0 = make_float4(cur.x, cur.y, cur.z, 1.0f);
    float m1 = Lc, m2 = Lc * Lc;
    if (sw > 0.0f) {
        const float cr = sr / sw, cg = sg / sw, cb = sb / sw, m1p = s1m / sw, m2p = s2m / sw;
        const float N = fminf(lmin + 1.0f, A.max_history);
        const float alpha = 1.0f / N;
        o0 = make_float4(cr + alpha * (cur.x - cr), cg + alpha * (cur.y - cg), cb + alpha * (cur.z - cb), N);
        m1 = m1p + alpha * (Lc - m1p);
        m2 = m2p + alpha * (Lc * Lc - m2p);
    }
    h0_out[i] = o0;
    h1_out[i] = make_float4(m1, m2, t, g1.w);
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

int launch_temporal_snapshot(const float* shade, float* prev_xyzr, uint32_t n_spheres, void* stream) {
    if (n_spheres == 0) return 0;
    hipLaunchKernelGGL(temporal_snapshot_kernel, dim3((n_spheres + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(shade), reinterpret_cast<float4*>(prev_xyzr), n_spheres);
    return (int)hipGetLastError();
}

}  // namespace mrt
