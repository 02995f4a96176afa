// Device-side vector arithmetic and random numbers, as the reference's WGSL evaluates them (raytracer/src/shader.wgsl; the
// "MRT-F32" rules of DESIGN.md §3: fma only where written): V3 and its operators, dot / normalize / reflect / mix, the noise
// estimate's luminance, Xoshiro128+.  Shared by kernels.hip, adaptive.hip, noise.hip and denoise.hip.  Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrt {

struct V3 { float x, y, z; };

__device__ __forceinline__ V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ V3 operator-(V3 a) { return v3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return v3(a.x / s, a.y / s, a.z / s); }

// WGSL dot(): x*x first, then fma in y, then fma in z
__device__ __forceinline__ float dot3(V3 a, V3 b) {
    return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x));
}
// WGSL normalize(e) = e / length(e)
__device__ __forceinline__ V3 normalize3(V3 v) { return v / __builtin_sqrtf(dot3(v, v)); }
// WGSL reflect(e1, e2) = e1 - 2*dot(e2, e1)*e2  (shader.wgsl:230)
__device__ __forceinline__ V3 reflect3(V3 d, V3 n) {
    float k = 2.0f * dot3(n, d);
    return v3(d.x - k * n.x, d.y - k * n.y, d.z - k * n.z);
}
// WGSL mix(e1, e2, e3) = e1*(1-e3) + e2*e3
__device__ __forceinline__ float mixf(float a, float b, float t) { return a * (1.0f - t) + b * t; }
// luminance as noise tracking defines it (blend.h's S update, noise.hip, denoise.hip)
__device__ __forceinline__ float lumf(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// ---- Xoshiro128+ (shader.wgsl:36-94) -------------------------------------------------
struct Rng { uint32_t s0, s1, s2, s3; uint32_t draws; };

__device__ __forceinline__ uint32_t rng_next(Rng& r) {          // shader.wgsl:49-64
    uint32_t result = r.s0 + r.s3;
    uint32_t t = r.s1 << 9;
    r.s2 ^= r.s0;
    r.s3 ^= r.s1;
    r.s1 ^= r.s2;
    r.s0 ^= r.s3;
    r.s2 ^= t;
    r.s3 = (r.s3 << 11) | (r.s3 >> 21);                          // rotl_u32(.., 11), :36-38
    return result;
}
__device__ __forceinline__ float rng_f32(Rng& r) {               // shader.wgsl:66-69
    r.draws++;
    return (float)rng_next(r) * 0x1p-32f;                        // == f32(i) / 4294967296.0
}
__device__ __forceinline__ uint32_t fmix32(uint32_t z) {         // MurmurHash3 finaliser (counter mode)
    z ^= z >> 16; z *= 0x85EBCA6Bu; z ^= z >> 13; z *= 0xC2B2AE35u; z ^= z >> 16;
    return z;
}
// 2.0 * random_f32() - 1.0 (shader.wgsl:86) in one rounding: f32(i) * 2^-32 and the doubling are exact
// (powers of two, no underflow), so the reference's value is fl(f32(i) * 2^-31 - 1) = this fma, bit for bit
__device__ __forceinline__ float rng_pm1(Rng& r) {
    r.draws++;
    return __builtin_fmaf((float)rng_next(r), 0x1p-31f, -1.0f);
}

}  // namespace mrt
