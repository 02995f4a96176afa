// The refit behind mrt_update_spheres (world.cpp; include/myraytracer_amd.h "scene"): new centres and radii for spheres whose
// grouping stays.  Everything hierarchy.cpp derives from the spheres' geometry -- member records, the bounding spheres of the
// clusters / inner levels / top, the boxes of large scenes in the kernel's top-down numbering, the matrix-core sweep's A operand
// for D = I -- recomputed on the device with hierarchy.cpp's formulas, in double, queued in stream order.  Node j of level k
// covers the member slots [j 4^k, (j+1) 4^k) of the hierarchy part of level 0, so every bound is a segmented reduction over the
// members themselves and the levels do not depend on one another.  The outputs are held to the builder's invariants
// (tests/refit_ref.py), not to bit identity with it.  (The build's -ffp-contract=off holds here too: no fused rounding.)
#include <hip/hip_runtime.h>
#include "mrt_internal.h"

namespace mrt {
namespace {

constexpr uint32_t kRefitBlock = 256;

__device__ __forceinline__ float round_up_f32(double v) {
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, INFINITY);
    return f;
}

// One lane per updated sphere of the batch: the four device copies of a sphere's geometry.  The batch rides in the kernel
// arguments, so the host stages nothing.
__global__ void __launch_bounds__(kRefitBlock) refit_scatter_kernel(const RefitScatterArgs a) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= a.count) return;
    const float x = a.xyzr[4 * i], y = a.xyzr[4 * i + 1], z = a.xyzr[4 * i + 2], r = a.xyzr[4 * i + 3];
    const size_t s = (size_t)a.first + i;
    a.spheres[s] = SphereRec{x, y, z, -(r * r)};
    float* sh = a.shade + 8 * s;
    sh[0] = x; sh[1] = y; sh[2] = z; sh[3] = r;
    float* ctr = a.centres + 4 * s;                     // (the fourth float of a centre stays the caller's)
    ctr[0] = x; ctr[1] = y; ctr[2] = z;
    a.radii[s] = r;
}

// level 0: slot m takes its record from sphere member_index[m]; a never-hit padding slot stays as it is
__global__ void __launch_bounds__(kRefitBlock) refit_members_kernel(const RefitArgs a) {
    const uint32_t m = blockIdx.x * kRefitBlock + threadIdx.x;
    if (m >= a.n_members) return;
    if (a.nodes[m].neg_r2 == INFINITY) return;
    a.nodes[m] = a.spheres[a.member_index[m]];
}

template <uint32_t L> __device__ __forceinline__ double group_min(double v) {
#pragma unroll
    for (uint32_t off = L / 2; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, (int)off));
    return v;
}
template <uint32_t L> __device__ __forceinline__ double group_max(double v) {
#pragma unroll
    for (uint32_t off = L / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, (int)off));
    return v;
}

// Level k (1 .. levels; the top is level `levels`): L = min(4^k, 64) lanes per node, each taking every L-th member slot of the
// node's span -- a lane per member up to level 3, a whole wave with four slots a lane at level 4.  Two passes over the members,
// as enclose / build_hierarchy make them: their common box (-> the f32 centre), then R = max(|c_m - centre| + |r_m|) measured
// from the ROUNDED centre.  The node's box (large scenes) comes from the first pass: build_boxes' extents, pack_boxes' 24 bytes.
template <uint32_t L>
__global__ void __launch_bounds__(kRefitBlock) refit_level_kernel(const RefitArgs a, const uint32_t k) {
    const uint32_t g = blockIdx.x * kRefitBlock + threadIdx.x, j = g / L, sub = g % L;
    const uint32_t n_k = k == a.levels ? a.n_padded : (k + 1 < a.levels ? a.level_base[k + 1] : a.n_nodes) - a.level_base[k];
    const uint64_t span = 1ull << (2 * k);
    const uint64_t m0 = min((uint64_t)a.n_hier, (uint64_t)j * span), m1 = min((uint64_t)a.n_hier, ((uint64_t)j + 1) * span);
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (uint64_t m = m0 + sub; m < m1; m += L) {
        const SphereRec s = a.nodes[m];
        if (s.neg_r2 == INFINITY) continue;
        const double r = fabs((double)a.shade[8 * (size_t)a.member_index[m] + 3]);
        const double c[3] = {s.cx, s.cy, s.cz};
#pragma unroll
        for (int q = 0; q < 3; q++) { lo[q] = fmin(lo[q], c[q] - r); hi[q] = fmax(hi[q], c[q] + r); }
    }
#pragma unroll
    for (int q = 0; q < 3; q++) { lo[q] = group_min<L>(lo[q]); hi[q] = group_max<L>(hi[q]); }
    const bool any = lo[0] <= hi[0];
    double ctr[3];
#pragma unroll
    for (int q = 0; q < 3; q++) ctr[q] = (double)(float)(0.5 * (lo[q] + hi[q]));
    double R = 0.0;
    for (uint64_t m = m0 + sub; m < m1; m += L) {
        const SphereRec s = a.nodes[m];
        if (s.neg_r2 == INFINITY) continue;
        const double r = fabs((double)a.shade[8 * (size_t)a.member_index[m] + 3]);
        const double dx = (double)s.cx - ctr[0], dy = (double)s.cy - ctr[1], dz = (double)s.cz - ctr[2];
        R = fmax(R, sqrt(dx * dx + dy * dy + dz * dz) + r);
    }
    R = group_max<L>(R);
    if (sub != 0 || j >= n_k) return;
    SphereRec* const out = k == a.levels ? a.clusters : a.nodes + a.level_base[k];
    if (any) {
        const float Rf = (float)(R * kBoundInflate) + 1e-30f;
        out[j] = SphereRec{(float)ctr[0], (float)ctr[1], (float)ctr[2], -(Rf * Rf)};
    } else {
        out[j] = SphereRec{0.0f, 0.0f, 0.0f, INFINITY};
    }
    if (!a.boxes) return;
    // depth t = levels - k of the top-down numbering starts at n_padded (4^t - 1) / 3 and has n_padded 4^t slots
    const uint32_t t = a.levels - k;
    const uint64_t width = (uint64_t)a.n_padded << (2 * t), at = (width - a.n_padded) / 3 + j;
    if (j >= width) return;
    if (!any) {
        a.boxes[at] = a.boxes_open[at] = BoxRec{0.0f, 0.0f, 0.0f, -3.0e38f, -3.0e38f, -3.0e38f};
        return;
    }
    float c[3], e[3];
    double e1 = 0.0, e2 = 0.0;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        c[q] = (float)(0.5 * (lo[q] + hi[q]));
        e[q] = round_up_f32(fmax(hi[q] - (double)c[q], (double)c[q] - lo[q]) * (1.0 + 1e-6) + 1e-37);
        e1 += (double)e[q];
        e2 += (double)e[q] * (double)e[q];
    }
    // kpad for the kc of THIS call (the host keeps kc >= 1.3e-6 / the smallest radius: world.cpp), folded into the extents
    const double kc = (double)a.box_kc;
    const float kpad = a.box_quad ? round_up_f32(kc * e2 + 4.4e-14 / kc) : round_up_f32(1.5e-3 * e1);
    a.boxes[at] = BoxRec{c[0], c[1], c[2], round_up_f32((double)e[0] + (double)kpad), round_up_f32((double)e[1] + (double)kpad),
                         round_up_f32((double)e[2] + (double)kpad)};
    a.boxes_open[at] = BoxRec{c[0], c[1], c[2], 3.0e37f, 3.0e37f, 3.0e37f};
}

__device__ __forceinline__ uint16_t bf16_rne(float x) {
    uint32_t u = __float_as_uint(x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float bf16_value(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// The top records as the matrix-core sweep's A operand for D = I, relative to the kept origin: pack_top_mfma's layout, bf16
// splits and round-down of Ck, one lane per row (record) of a tile.  After the top level's kernel in stream order.
__global__ void __launch_bounds__(kRefitBlock) refit_mfma_kernel(const RefitArgs a) {
    const uint32_t g = blockIdx.x * kRefitBlock + threadIdx.x;
    if (g >= a.n_padded) return;
    const uint32_t t = g / 32u, m = g % 32u;
    const SphereRec rec = a.clusters[32u * t + 16u * ((m >> 2) & 1u) + 4u * (m >> 3) + (m & 3u)];
    const float c[3] = {(float)((double)rec.cx - (double)a.origin[0]), (float)((double)rec.cy - (double)a.origin[1]),
                        (float)((double)rec.cz - (double)a.origin[2])};
    float ck = 3.0e38f;
    if (rec.neg_r2 != INFINITY) {
        const double c2 = (double)c[0] * c[0] + (double)c[1] * c[1] + (double)c[2] * c[2];
        const double R = sqrt(-(double)rec.neg_r2) + 2.0 * 0x1p-24 * sqrt(c2), R2 = R * R;
        const double v = c2 - R2 - 0x1p-13 * (c2 + R2);
        ck = (float)v;
        if ((double)ck > v) ck = nextafterf(ck, -INFINITY);
    }
    uint16_t hi[3], lo16[3];
#pragma unroll
    for (int q = 0; q < 3; q++) { hi[q] = bf16_rne(c[q]); lo16[q] = bf16_rne(c[q] - bf16_value(hi[q])); }
    const uint16_t k0 = bf16_rne(ck);
    const float ck1 = ck - bf16_value(k0);
    const uint16_t k1 = bf16_rne(ck1), k2 = bf16_rne(ck1 - bf16_value(k1)), one = bf16_rne(1.0f);
    const uint16_t kvals[16] = {hi[0], hi[1], hi[2], hi[0], hi[1], hi[2], lo16[0], lo16[1], lo16[2], one, one, one, k0, k1, k2, 0};
    uint16_t* const o = a.top_mfma + (size_t)t * 512;
#pragma unroll
    for (int q = 0; q < 16; q++) o[((q >> 3) * 32 + m) * 8 + (q & 7)] = kvals[q];
}

template <uint32_t L> void launch_level(const RefitArgs& a, uint32_t k, uint32_t n_k, hipStream_t st) {
    const uint64_t lanes = (uint64_t)n_k * L;
    hipLaunchKernelGGL(refit_level_kernel<L>, dim3((uint32_t)((lanes + kRefitBlock - 1) / kRefitBlock)), dim3(kRefitBlock), 0, st, a, k);
}

}  // namespace

int launch_refit_scatter(const RefitScatterArgs& a, void* stream) {
    if (a.count == 0 || a.count > kRefitBatch) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(refit_scatter_kernel, dim3((a.count + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_refit(const RefitArgs& a, void* stream) {
    if (a.levels < 1 || a.levels > kMaxLevels || a.n_padded == 0 || a.n_members == 0) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(refit_members_kernel, dim3((a.n_members + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, a);
    for (uint32_t k = 1; k <= a.levels; k++) {
        const uint32_t n_k = k == a.levels ? a.n_padded : (k + 1 < a.levels ? a.level_base[k + 1] : a.n_nodes) - a.level_base[k];
        if (n_k == 0) continue;
        if (k == 1) launch_level<4>(a, k, n_k, st);
        else if (k == 2) launch_level<16>(a, k, n_k, st);
        else launch_level<64>(a, k, n_k, st);
    }
    hipLaunchKernelGGL(refit_mfma_kernel, dim3((a.n_padded + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace mrt
