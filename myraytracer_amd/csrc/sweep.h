// The conservative sweep over the top level of the bounding-sphere hierarchy, and the box test of the large scenes' walk
// (render_kernel, kernels.hip): the hand-issued scalar loads and the VALU test of the SGPR-fed sweep, the line-vs-box test,
// and the bf16-split GEMMs of the matrix-core sweep.  The comments are the proof sketches.  Internal: not installed.
#pragma once
#include "rt_math.h"

namespace mrt {

// ---- the discriminant sweep over wave-uniform sphere records --------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));
// four SphereRec = 16 dwords = one s_load_dwordx16 from the constant address space
typedef const f32x16 __attribute__((address_space(4)))* SphQuadPtr;
struct Sph8 { f32x16 lo, hi; };

// Scalar loads are issued and waited for by hand (inline asm): hipcc schedules every
// s_load of an unrolled body first and then spills the SGPRs, and its waitcnt pass can only
// emit lgkmcnt(0) -- scalar loads return out of order -- which would also wait for a
// prefetch.  An asm load is invisible to that pass, so each group is tied to its own wait:
// smem_wait() "redefines" the group, and every use of the group therefore follows the wait.
__device__ __forceinline__ void smem_load8(Sph8& g, SphQuadPtr quads, uint32_t first_sphere) {
    const SphQuadPtr p = quads + first_sphere / 4u;
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40"
                 : "=&s"(g.lo), "=&s"(g.hi) : "s"(p));
}
// One statement = "group `cur` has landed; start fetching group `nxt`".  `bits` (produced by
// the previous group's tests) rides along so that those tests are scheduled BEFORE this
// point and the tests of `cur` after it, i.e. while the loads of `nxt` are in flight.
__device__ __forceinline__ void smem_wait_then_load8(Sph8& cur, Sph8& nxt, SphQuadPtr quads, uint32_t first_sphere,
                                                     uint32_t& bits) {
    const SphQuadPtr p = quads + first_sphere / 4u;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_load_dwordx16 %2, %5, 0x0\n\ts_load_dwordx16 %3, %5, 0x40"
                 : "+s"(cur.lo), "+s"(cur.hi), "=&s"(nxt.lo), "=&s"(nxt.hi), "+v"(bits) : "s"(p));
}
// The sweep's CONSERVATIVE line-vs-bounding-sphere test (10 fp32 VALU + 1 v_alignbit): with `ds` the
// ray direction stretched by kBoundStretch (1 + 1e-4), S = (oc.ds)^2 - (oc.oc - R^2) is >= 0 whenever the
// reference's discriminant b*b - a*c (shader.wgsl:277-282) of ANY sphere inside the bound is >= 0:
// the stretch adds >= 1.9e-4*|oc|^2 of slack against <= 1.2e-4*|oc|^2 of accumulated rounding error
// and R is 1.5 % larger than the enclosing radius (proof sketch: DESIGN.md §4).  False positives only
// cost a discriminant evaluation; a false negative cannot happen.  sign(S) is shifted into `bits`.
__device__ __forceinline__ void test1(float cx, float cy, float cz, float neg_R2, V3 o, V3 ds, uint32_t& bits) {
    const float ocx = o.x - cx, ocy = o.y - cy, ocz = o.z - cz;
    const float b = __builtin_fmaf(ocz, ds.z, __builtin_fmaf(ocy, ds.y, ocx * ds.x));
    const float c = __builtin_fmaf(ocz, ocz, __builtin_fmaf(ocy, ocy, __builtin_fmaf(ocx, ocx, neg_R2)));
    const float S = __builtin_fmaf(b, b, -c);
    bits = __builtin_amdgcn_alignbit(bits, __float_as_uint(S), 31);       // oldest record ends in the top bit
}
__device__ __forceinline__ void test4(const f32x16 q, V3 o, V3 ds, uint32_t& bits) {
    test1(q[0], q[1], q[2], q[3], o, ds, bits);
    test1(q[4], q[5], q[6], q[7], o, ds, bits);
    test1(q[8], q[9], q[10], q[11], o, ds, bits);
    test1(q[12], q[13], q[14], q[15], o, ds, bits);
}
__device__ __forceinline__ void test8(const Sph8& g, V3 o, V3 ds, uint32_t& bits) {
    test4(g.lo, o, ds, bits);
    test4(g.hi, o, ds, bits);
}

// ---- the walk's second bound for large scenes: the axis-aligned box of the member spheres under a node -----------------
// A kd-built group of spheres on a plane fills its box, not its bounding sphere: over C5's 100 x 100 grid a ray's LINE touches
// 7.2 + 7.4 + 1.4 bounding spheres of the three levels but 1.9 + 1.9 + 0.9 boxes (experiments/bound_stats.py).  The test is the
// line against the box grown by K on every side, through the three separating axes d x e_i:
//     |p_j d_k - p_k d_j| <= e_j |d_k| + e_k |d_j| + K        p = o - centre, (i, j, k) cyclic
// (necessary and sufficient for a line and a box; the parts of the line behind the origin are left to the sphere tests).
// K = kc X + kpad, X = |p|^2 or |p|_1 (per scene), is the slack that makes it CONSERVATIVE against the reference's own
// rounding: a member whose computed discriminant is >= 0 has the line within sqrt(r^2 + 14 eps |oc|^2 / a) of its centre,
// i.e. up to min(14 eps |oc|^2 / (2 r), sqrt(14 eps) |oc|) beyond its surface, hence beyond its box; the host (bounds.h,
// box_kpad) sets kc per scene and kpad per box so that K covers 1.4143 x that for every member under the node, plus the
// test's own rounding (4 eps |p|_1; the right-hand side's three roundings are in the extents).  The kernel reads kpad FOLDED
// INTO THE EXTENTS (e + kpad: on the axis d x e_i that is a slack of kpad (|d_j| + |d_k|), which covers what "+ kpad" covered:
// bounds.h, fold_kpad) and kc from its arguments, so a box is 24 bytes.  A never-hit box has extents
// -3e38: some axis' right-hand side is then hugely negative (a unit direction has a component >= 0.57).
// 24 VALU: 3 + 3 (X) + 1 (K) + 3 x 5 + 2.
// (c, e): a BoxRec -- the centre and the half extents with kpad folded in (mrt_internal.h); kc: the scene's coefficient of X.
template <bool QUAD>
__device__ __forceinline__ uint32_t box_separated_bits(const V3 c, const V3 e, const float kc, V3 o, V3 d) {
    const float px = o.x - c.x, py = o.y - c.y, pz = o.z - c.z;
    const float X = QUAD ? __builtin_fmaf(pz, pz, __builtin_fmaf(py, py, px * px))
                         : (__builtin_fabsf(px) + __builtin_fabsf(py)) + __builtin_fabsf(pz);
    const float K = kc * X;
    const float ex = e.x, ey = e.y, ez = e.z;
    const float adx = __builtin_fabsf(d.x), ady = __builtin_fabsf(d.y), adz = __builtin_fabsf(d.z);
    const float sx = __builtin_fmaf(ey, adz, __builtin_fmaf(ez, ady, K)) - __builtin_fabsf(__builtin_fmaf(-pz, d.y, py * d.z));
    const float sy = __builtin_fmaf(ez, adx, __builtin_fmaf(ex, adz, K)) - __builtin_fabsf(__builtin_fmaf(-px, d.z, pz * d.x));
    const float sz = __builtin_fmaf(ex, ady, __builtin_fmaf(ey, adx, K)) - __builtin_fabsf(__builtin_fmaf(-py, d.x, px * d.y));
    // separated on some axis <=> some difference is negative (finite operands: never NaN): the sign bit of the result
    return __float_as_uint(sx) | __float_as_uint(sy) | __float_as_uint(sz);
}
template <bool QUAD>
__device__ __forceinline__ bool box_may_touch(const V3 c, const V3 e, const float kc, V3 o, V3 d) {
    return (int32_t)box_separated_bits<QUAD>(c, e, kc, o, d) >= 0;
}

// ---- the same conservative test on the matrix cores -------------------------------------------------
// Expanding S = (oc.ds)^2 - (oc.oc - R^2) with oc = o - C turns its two dot products into products of a
// per-record vector with a per-ray vector:
//     -(oc.ds) = C.ds - o.ds                 S = (oc.ds)^2 - o.o - U
//     U        = -2 o.C + (C.C - R^2)
// i.e. two [32 records] x [32 rays] GEMMs per tile.  The f32 MFMA runs on the vector FMA units (measured:
// no overlap with VALU work), so the GEMMs run in bf16 on the matrix cores proper, with every f32 factor
// split into bf16 pieces x = hi + lo (+ mid) and the cross products laid out along K = 16:
//     k  0..2   C_hi (x,y,z)     . v_hi        v = K ds for the first GEMM, 2 K^2 o for the second
//     k  3..5   C_hi             . v_lo
//     k  6..8   C_lo             . v_hi
//     k  9..11  (1, 1, 1)        . (-K o.ds | -K^2 o.o (minus its slack)), each as hi, mid, lo
//     k 12..14  Ck (hi, mid, lo) . (0, 0, 0 | -K^2 x (1, 1, 1))       Ck = C.C - R^2 (minus its slack)
// so ONE A operand per tile serves both; the first GEMM's result g = -K oc.ds, squared where it is positive (the
// record's centre ahead of the origin), is the C input of the second, which therefore delivers
// K^2 (max(-oc.ds, 0)^2 - U - o.o) -- K^2 S for a centre ahead, K^2 (R^2 - |oc|^2) otherwise, which drops the bounds
// that lie entirely behind the origin: one multiply and one alignbit per (ray, record).  K, a power of two chosen by
// the host so that |g| <= 1/2 (KParams::mfma_scale), only makes the multiply's clamp to [0, 1] act as max(g, 0)^2; a
// power of two changes no rounding.  What the split drops (C_lo v_lo and the remainders: 3 x 2^-18 of
// every product) and the f32 accumulation err by at most 2.5e-5 o.o + 5e-5 C.C in S; the
// test gives away 2^-13 = 1.2e-4 of o.o + C.C + R^2: o.o is scaled by 1 - 2^-13 (in mfma_scale[2]) and the host
// lowers Ck by 2^-13 (C.C + R^2) (bounds.h, mfma_row).  o and C are taken relative to the centre of the
// records' bounding box (P.mfma_origin; the rounding of o - origin is relative to the difference), so the
// slack does not depend on where the scene sits, only on its extent against R: the host selects this
// variant only where it is small against R^2; elsewhere the SGPR-fed sweep above runs.
// Operand layout (lane l, r = l & 31, h = l >> 5): A[record r][k = 8h + j], B[k = 8h + j][ray r], j = 0..7;
// result register i of lane l is record (i&3) + 8(i>>2) + 4h for ray r.  v_permlane32_swap(a, b) =
// {(a.lo, b.lo), (a.hi, b.hi)} builds the B operands of both 32-ray halves from a lane's own k 0..7 and
// k 8..15 words and, applied to the two halves' sign words, hands every lane the signs of its OWN ray:
// r[0] = the records with (row & 4) == 0, r[1] = the others.  The host stores the records of a tile in that
// order, so r[0] / r[1] are the masks of chunks 2t / 2t+1.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct MfmaRay { u32x4 bp[2], bu[2]; };
__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {          // two round-to-nearest conversions
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ float bf16_round(float x) { return (float)(__bf16)x; }
__device__ __forceinline__ void swap32(uint32_t a, uint32_t b, uint32_t& r0, uint32_t& r1) {
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    r0 = r[0];
    r1 = r[1];
}
__device__ __forceinline__ void mfma_pack_ray(V3 v, float w0, float w1, float w2, uint32_t y2, uint32_t y3, u32x4 out[2]) {
    const V3 h = v3(bf16_round(v.x), bf16_round(v.y), bf16_round(v.z));
    const V3 l = v3(v.x - h.x, v.y - h.y, v.z - h.z);           // exact; rounded to bf16 by the packing below
    const uint32_t x0 = pk_bf16(h.x, h.y), x1 = pk_bf16(h.z, l.x), x2 = pk_bf16(l.y, l.z);      // k 0..5, 6..7 = x0
    const uint32_t y0 = pk_bf16(h.z, w0), y1 = pk_bf16(w1, w2);                                   // k 8..11
    uint32_t a0, a1, a2, a3, b0, b1, b2, b3;
    swap32(x0, y0, a0, b0);
    swap32(x1, y1, a1, b1);
    swap32(x2, y2, a2, b2);
    swap32(x0, y3, a3, b3);
    out[0] = u32x4{a0, a1, a2, a3};
    out[1] = u32x4{b0, b1, b2, b3};
}
// `dsk` = K x the stretched direction, o2 = o.o, s2k2 = 2 K^2, nsk2 = -(1 - 2^-13) K^2, nk2 = -K^2 as a bf16 pair, K the
// power of two of KParams::mfma_scale: the first GEMM comes out as K (C.ds - o.ds) = -K oc.ds, the second as
// -K^2 (U + o.o) with o.o lowered by its slack.  Scaling by a power of two changes no rounding.
__device__ __forceinline__ MfmaRay mfma_ray_operands(V3 o, V3 dsk, float o2, float s2k2, float nsk2, uint32_t nk2) {
    MfmaRay m;
    const float nk0 = -dot3(o, dsk);
    const float n0 = bf16_round(nk0), n1 = bf16_round(nk0 - n0), n2 = (nk0 - n0) - n1;    // hi + mid + lo, each difference exact
    mfma_pack_ray(dsk, n0, n1, n2, 0u, 0u, m.bp);
    const float k1p = o2 * nsk2;
    const float q0 = bf16_round(k1p), q1 = bf16_round(k1p - q0), q2 = (k1p - q0) - q1;
    mfma_pack_ray(v3(s2k2 * o.x, s2k2 * o.y, s2k2 * o.z), q0, q1, q2, nk2, nk2 & 0xFFFFu, m.bu);     // k 12..14: -K^2, k 15: 0
    return m;
}
// one tile of 32 records against the wave's 64 rays; `a` = this lane's 8 bf16 of the tile's A operand
// (bounds.h, mfma_row).  Returns the candidate mask of the tile's 32 records (record i at bit 31 - i) for this
// lane's own ray.  TIGHT (the small scenes' instantiations): each half's 16 signs are shifted into a word that starts at 0, so the
// halves are below 2^16 and join in one shift-or without the mask; the other instantiations keep the form they were built with.
template <bool TIGHT>
__device__ __forceinline__ uint32_t mfma_sweep_tile(const u32x4 a, const MfmaRay& m) {
    const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const bf16x8 av = __builtin_bit_cast(bf16x8, a);
    uint32_t hb[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        // The first GEMM gives g = -K oc.ds: positive where the record's centre lies AHEAD of the origin.  Its square
        // becomes the C input of the second GEMM -- but only where g > 0: x |x| clamped to [0, 1] (the output modifier
        // of the same multiply; |g| <= 1/2 by the choice of K) is max(g, 0)^2 -- which then delivers
        // K^2 (max(-oc.ds, 0)^2 - U - o.o) in the same 16 registers.  For a centre ahead that is K^2 S, the stretched
        // discriminant, positive for a true candidate by the margin of the slack; for a centre not ahead it is
        // -K^2 c, c = |oc|^2 - R^2 (inflated, minus the slack): positive only if the origin lies inside the bound.
        // A bound with its centre not ahead and the origin outside lies entirely behind the origin -- no root of
        // anything inside it is positive (see the node rounds) -- and is no candidate: candidate = sign bit clear.
        // (A g that is not > 0 only through rounding has g^2 far below the slack.)
        f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, __builtin_bit_cast(bf16x8, m.bp[h]), zero, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] = __builtin_amdgcn_fmed3f(acc[i] * __builtin_fabsf(acc[i]), 0.0f, 1.0f);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, __builtin_bit_cast(bf16x8, m.bu[h]), acc, 0, 0, 0);
        uint32_t bb = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) bb = __builtin_amdgcn_alignbit(bb, __float_as_uint(acc[i]), 31);
        hb[h] = bb;
    }
    const auto r = __builtin_amdgcn_permlane32_swap(hb[0], hb[1], false, false);
    if constexpr (TIGHT) {
        // (the joined word made opaque before and after the complement: hipcc otherwise forms the complement and the word it
        // compares with all ones separately, a shift and two three-operand instructions where a shift-or and a v_not do)
        uint32_t x = (r[0] << 16) | r[1];
        asm("" : "+v"(x));
        x = ~x;
        asm("" : "+v"(x));
        return x;
    } else return ~((r[0] << 16) | (r[1] & 0xFFFFu));         // record i of the tile at bit 31 - i
}

}  // namespace mrt
