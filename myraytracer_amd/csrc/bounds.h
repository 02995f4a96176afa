// The hierarchy's bounds, derived ONCE: the formulas and constants behind every bounding sphere, box and matrix-core operand row,
// for the host builder (hierarchy.cpp), the scene bookkeeping of world.cpp and the device refit (refit.hip) alike.  The
// conservativeness argument of DESIGN.md §4 rests on these constants; a change to one of them lands here and nowhere else
// (tests/golden/hierarchy_hashes.json holds both sides to their recorded bits).  Every translation unit of the library is
// compiled as HIP, so these are plain host + device functions.  Internal: not installed.
//
// The minimum and maximum of two doubles are fmin / fmax on the device (one instruction) and std::min / std::max's compare and
// select on the host, where fmin / fmax also order NaNs and measured 10 % of the builder's time in build_clusters' inner loop.
// For the finite values mrt_set_world_raw and mrt_update_spheres admit the two agree, except in which zero they return for a tie
// of -0.0 and +0.0 -- a span whose one edge is made by a sphere with a centre coordinate of -0.0f and radius 0 -- and a zero of
// either sign gives the same centre and extents.
#pragma once
#include <math.h>

#include "mrt_internal.h"

namespace mrt {

constexpr float kBoundFloor = 1e-30f;            // added to every stored radius: a bound of one point still has R > 0
constexpr double kBoxQuadKc = 1.3e-6;            // the quadratic slack: kc = kBoxQuadKc / r_min, kpad = kc |e|^2 + kBoxQuadRounding / kc
constexpr double kBoxQuadRounding = 4.4e-14;
constexpr double kBoxLinKc = 1.5e-3;             // the linear slack: kc, kpad = kc |e|_1
constexpr double kBoxExtentGrow = 1.0 + 1e-6;    // the extents: the three roundings of the test's right-hand side ...
constexpr double kBoxExtentFloor = 1e-37;        // ... and > 0 for a span of one point
constexpr float kBoxNeverExtent = -3.0e38f;      // a never-hit box: no line passes it
constexpr float kBoxOpenExtent = 3.0e37f;        // a box opened wide: the test never rejects (mrt_debug_set_boxes(0))
// the matrix-core sweep inflates R^2 by this share of o.o + C.C + R^2 (mfma_row)
constexpr double kMfmaSlack = 0x1p-13;

#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline double min_f64(double a, double b) { return fmin(a, b); }
__device__ inline double max_f64(double a, double b) { return fmax(a, b); }
#else
inline double min_f64(double a, double b) { return b < a ? b : a; }
inline double max_f64(double a, double b) { return a < b ? b : a; }
#endif
__host__ __device__ inline float round_up_f32(double v) {
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, INFINITY);
    return f;
}
__host__ __device__ inline float round_down_f32(double v) {
    float f = (float)v;
    if ((double)f > v) f = nextafterf(f, -INFINITY);
    return f;
}
__host__ __device__ inline uint16_t bf16_rne(float x) {
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);      // NaN stays NaN
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__host__ __device__ inline float bf16_value(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }

// Enclosing sphere of a set of spheres: centre of the members' common box, R = max(|c_m - centre| + |r_m|).  The record stores
// the centre as f32, so R is measured from the ROUNDED centre and stays an enclosure; the stored radius is kBoundInflate x R
// (rounding R to f32 moves it by 6e-8 R; the 1.5 % is for the proof of DESIGN.md §4).
struct Span {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    __host__ __device__ void add(const float c[3], double r) {                   // r = |radius|
        for (int q = 0; q < 3; q++) { lo[q] = min_f64(lo[q], (double)c[q] - r); hi[q] = max_f64(hi[q], (double)c[q] + r); }
    }
    __host__ __device__ bool empty() const { return !(lo[0] <= hi[0]); }
    __host__ __device__ void centre(float c[3]) const { for (int q = 0; q < 3; q++) c[q] = (float)(0.5 * (lo[q] + hi[q])); }
};
// how far the surface of the sphere (c, r) reaches from a span's centre
__host__ __device__ inline double reach_from(const float centre[3], const float c[3], double r) {
    const double dx = (double)c[0] - (double)centre[0], dy = (double)c[1] - (double)centre[1], dz = (double)c[2] - (double)centre[2];
    return sqrt(dx * dx + dy * dy + dz * dz) + r;
}
__host__ __device__ inline SphereRec bound_record(const float centre[3], double R) {
    const float Rf = (float)(R * kBoundInflate) + kBoundFloor;
    return SphereRec{centre[0], centre[1], centre[2], -(Rf * Rf)};
}
__host__ __device__ inline SphereRec never_hit_record() { return SphereRec{0.0f, 0.0f, 0.0f, INFINITY}; }     // -r^2 = +inf: a discriminant of -inf
__host__ __device__ inline BoxRec never_hit_box() { return BoxRec{0.0f, 0.0f, 0.0f, kBoxNeverExtent, kBoxNeverExtent, kBoxNeverExtent}; }

// The box of a span, for the walk of large scenes (sweep.h, box_may_touch).  The test is "the LINE of the ray passes the box
// grown by K on every side", three separating axes d x e_i; it must hold whenever the reference's discriminant of a member
// under the node is computed >= 0, i.e. whenever the line passes within h of the member's centre,
// h^2 <= r^2 + E, E = 14 eps |oc|^2 / a: h - r <= E / (2 r) (the quadratic form) and <= sqrt(E) (the linear form).  With
// |oc| <= |p| + |e| (p: origin - box centre, e: half extents) and |d_j| + |d_k| <= 1.4143:
//     quadratic   K = kc |p|^2 + kpad,  kc = 1.3e-6 / r_min,  kpad = kc |e|^2 + 4.4e-14 / kc
//     linear      K = kc |p|_1 + kpad,  kc = 1.5e-3,          kpad = kc |e|_1
// (each with >= 9 % to spare over 1.4143 x the bound; the 4.4e-14 / kc makes the quadratic form cover the test's own
// rounding, 4 eps |p|_1, by the inequality of the means).  The quadratic form is far smaller at moderate distances, the
// linear one at large distances from tiny spheres; the scene takes the one that is smaller at its own reach (build_boxes).
// kc is ONE value per scene (r_min = the scene's smallest radius, which only makes K larger for the other boxes): the kernel
// takes it from its arguments, and kpad -- the only other per-box part of K -- is folded into the extents the kernel reads
// (fold_kpad), so a box is 24 bytes on the device.
struct BoxExtents { float c[3], e[3]; double e1, e2; };      // f32 centre, half extents from it (rounded up), |e|_1, |e|^2
__host__ __device__ inline BoxExtents box_extents(const Span& s) {
    BoxExtents b;
    s.centre(b.c);
    b.e1 = b.e2 = 0.0;
    for (int q = 0; q < 3; q++) {
        b.e[q] = round_up_f32(max_f64(s.hi[q] - (double)b.c[q], (double)b.c[q] - s.lo[q]) * kBoxExtentGrow + kBoxExtentFloor);
        b.e1 += (double)b.e[q];
        b.e2 += (double)b.e[q] * (double)b.e[q];
    }
    return b;
}
// the quadratic form's kc for a smallest radius r = |radius|, unrounded; the scene's value is round_up_f32 of it
__host__ __device__ inline double quad_kc_for_radius(double r) { return kBoxQuadKc / max_f64(r, 1e-30); }
// kpad.  The quadratic form takes kc twice, and the two sides differ in what they pass: the host builder multiplies by the scene's
// f32 kc (rounded up) but divides by the unrounded double it came from; the refit has only the f32 kc of its call (world.cpp keeps
// it >= quad_kc_for_radius of every clustered sphere) and uses it for both.  Both are valid bounds -- kc e2 + c / kc covers the
// test's rounding for any kc > 0 -- and they differ by an ulp at most.  Nobody chose the difference; it is kept as it was found,
// because unifying it moves boxes.
__host__ __device__ inline float box_kpad(bool quad, double kc_product, double kc_quotient, double e1, double e2) {
    return quad ? round_up_f32(kc_product * e2 + kBoxQuadRounding / kc_quotient) : round_up_f32(kBoxLinKc * e1);
}
// What the kernel reads of an extent (mrt_internal.h, BoxRec): e' = e + kpad rounded up.  The test on the axis d x e_i then has
// the slack kc X + kpad (|d_j| + |d_k|) instead of kc X + kpad; what is needed there is rho |d x e_i| + (the test's rounding)
// (|d_j| + |d_k|), rho the distance beyond the box the line of a candidate can pass, and |d x e_i| <= s = |d_j| + |d_k| <= 1.4143:
// both sides are linear in s on [0, 1] and on [1, 1.4143], at s = 0 the left side is kc X >= 0, and at s = 1 and s = 1.4143 the
// inequality is the one box_kpad provides (kc X + kpad >= 1.4143 rho + the rounding: tests/test_hierarchy_host.py checks it box
// by box).
__host__ __device__ inline float fold_kpad(float e, float kpad) { return round_up_f32((double)e + (double)kpad); }

// The top level as the A operand of the matrix-core sweep (sweep.h, mfma_sweep_tile): per tile of 32 records 64 lanes x 8 bf16,
// lane l = row (l & 31), k = 8 (l >> 5) + j:
//     k 0..2 C_hi, 3..5 C_hi, 6..8 C_lo, 9..11 (1,1,1), 12..14 Ck (hi, mid, lo), 15: 0
// where row m of tile t is record mfma_source_record(t, m) -- the order in which the MFMA result registers come out, so that the
// two 16-bit sign words per tile are the masks of chunks 2t and 2t + 1 -- and slot q of row m sits at mfma_slot(m, q) of the
// tile's 512 values.  C is relative to the sweep's origin: exact in double, then rounded to f32 -- the rounding moves a bound by
// at most 2 eps |c|, which its radius absorbs (mfma_terms).  Ck = C.C - R^2 - kMfmaSlack (C.C + R^2), rounded DOWN: the record's
// share of the slack that covers what the bf16 split drops.  A never-hit record gets Ck = 3e38 (finite: an
// infinity would turn the other GEMM's 0 x Ck into NaN).
__host__ __device__ inline uint32_t mfma_source_record(uint32_t t, uint32_t m) { return 32u * t + 16u * ((m >> 2) & 1u) + 4u * (m >> 3) + (m & 3u); }
__host__ __device__ inline uint32_t mfma_slot(uint32_t m, uint32_t q) { return ((q >> 3) * 32u + m) * 8u + (q & 7u); }
__host__ __device__ inline SphereRec relative_record(const SphereRec& r, const float origin[3]) {
    return SphereRec{(float)((double)r.cx - (double)origin[0]), (float)((double)r.cy - (double)origin[1]), (float)((double)r.cz - (double)origin[2]), r.neg_r2};
}
struct MfmaTerms { double c2, R2; };             // of a real record relative to the origin: C.C, and R^2 with the rounding of C absorbed
__host__ __device__ inline MfmaTerms mfma_terms(const SphereRec& rel) {
    const double c2 = (double)rel.cx * rel.cx + (double)rel.cy * rel.cy + (double)rel.cz * rel.cz;
    const double R = sqrt(-(double)rel.neg_r2) + 2.0 * 0x1p-24 * sqrt(c2);
    return MfmaTerms{c2, R * R};
}
__host__ __device__ inline void mfma_row(const SphereRec& rel, uint16_t out16[16]) {
    float ck = 3.0e38f;
    if (rel.neg_r2 != INFINITY) {
        const MfmaTerms t = mfma_terms(rel);
        ck = round_down_f32(t.c2 - t.R2 - kMfmaSlack * (t.c2 + t.R2));
    }
    const float c[3] = {rel.cx, rel.cy, rel.cz};
    const uint16_t one = bf16_rne(1.0f), k0 = bf16_rne(ck);
    const float ck1 = ck - bf16_value(k0);
    const uint16_t k1 = bf16_rne(ck1);
    for (int q = 0; q < 3; q++) {
        out16[q] = out16[3 + q] = bf16_rne(c[q]);
        out16[6 + q] = bf16_rne(c[q] - bf16_value(out16[q]));
        out16[9 + q] = one;
    }
    out16[12] = k0; out16[13] = k1; out16[14] = bf16_rne(ck1 - bf16_value(k1)); out16[15] = 0;
}

}  // namespace mrt
