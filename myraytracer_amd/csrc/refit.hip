// The refit behind mrt_update_spheres (world.cpp; include/myraytracer_amd.h "scene"): new centres and radii for spheres whose
// grouping stays.  Everything hierarchy.cpp derives from the spheres' geometry -- member records, the bounding spheres of the
// clusters / inner levels / top, the boxes of large scenes in the kernel's top-down numbering, the matrix-core sweep's A operand
// for D = I -- recomputed on the device by the functions of bounds.h, which the builder calls too, in double, queued in stream
// order.  Node j of level k covers the member slots [j 4^k, (j+1) 4^k) of the hierarchy part of level 0, so every bound is a
// segmented reduction over the members themselves and the levels do not depend on one another.  What is the device's own here:
// which lane takes which member, the shuffles, the top-down slot of a box, the launches.  The outputs are held to the builder's
// invariants (tests/refit_ref.py) and to their recorded bits (tests/golden/hierarchy_hashes.json), not to bit identity with the
// builder: box_kpad (bounds.h) says where the two differ.  (The build's -ffp-contract=off holds here too: no fused rounding.)
#include <hip/hip_runtime.h>
#include "bounds.h"

namespace mrt {
namespace {

constexpr uint32_t kRefitBlock = 256;

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

// mrt_update_materials: one lane per edited sphere of the batch, which rides in the kernel arguments like a geometry update's.
// The upper half of the shade record in one 16-byte store (records are 32 bytes, the array hipMalloc's: aligned), the type word,
// and with restart_history a NaN for the radius of the temporal step's "previous" sphere (world.cpp says why).
__global__ void __launch_bounds__(kRefitBlock) material_scatter_kernel(const MaterialScatterArgs a) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= a.count) return;
    const size_t s = (size_t)a.first + i;
    reinterpret_cast<float4*>(a.shade)[2 * s + 1] = make_float4(a.words[4 * i], a.words[4 * i + 1], a.words[4 * i + 2], a.words[4 * i + 3]);
    a.types[s] = a.ty[i];
    if (a.restart_history) a.prev_xyzr[4 * s + 3] = __builtin_nanf("");
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
// node's span -- a lane per member up to level 3, a whole wave with four slots a lane at level 4.  Two passes over the members:
// their common box (bounds.h, Span: -> the f32 centre), then R measured from that centre.  The node's box (large scenes) comes
// from the first pass.
template <uint32_t L>
__global__ void __launch_bounds__(kRefitBlock) refit_level_kernel(const RefitArgs a, const uint32_t k) {
    const uint32_t g = blockIdx.x * kRefitBlock + threadIdx.x, j = g / L, sub = g % L;
    const uint32_t n_k = k == a.levels ? a.n_padded : (k + 1 < a.levels ? a.level_base[k + 1] : a.n_nodes) - a.level_base[k];
    const uint64_t span = 1ull << (2 * k);
    const uint64_t m0 = min((uint64_t)a.n_hier, (uint64_t)j * span), m1 = min((uint64_t)a.n_hier, ((uint64_t)j + 1) * span);
    Span s;
    for (uint64_t m = m0 + sub; m < m1; m += L) {
        const SphereRec rec = a.nodes[m];
        if (rec.neg_r2 == INFINITY) continue;
        s.add(&rec.cx, fabs((double)a.shade[8 * (size_t)a.member_index[m] + 3]));
    }
#pragma unroll
    for (int q = 0; q < 3; q++) { s.lo[q] = group_min<L>(s.lo[q]); s.hi[q] = group_max<L>(s.hi[q]); }
    float ctr[3];
    s.centre(ctr);
    double R = 0.0;
    for (uint64_t m = m0 + sub; m < m1; m += L) {
        const SphereRec rec = a.nodes[m];
        if (rec.neg_r2 == INFINITY) continue;
        R = fmax(R, reach_from(ctr, &rec.cx, fabs((double)a.shade[8 * (size_t)a.member_index[m] + 3])));
    }
    R = group_max<L>(R);
    if (sub != 0 || j >= n_k) return;
    SphereRec* const out = k == a.levels ? a.clusters : a.nodes + a.level_base[k];
    if (s.empty()) out[j] = never_hit_record();
    else out[j] = bound_record(ctr, R);
    if (!a.boxes) return;
    // depth t = levels - k of the top-down numbering starts at n_padded (4^t - 1) / 3 and has n_padded 4^t slots
    const uint32_t t = a.levels - k;
    const uint64_t width = (uint64_t)a.n_padded << (2 * t), at = (width - a.n_padded) / 3 + j;
    if (j >= width) return;
    if (s.empty()) {
        a.boxes[at] = a.boxes_open[at] = never_hit_box();
        return;
    }
    // kpad for the kc of THIS call (the host keeps kc >= quad_kc_for_radius of every clustered sphere: world.cpp)
    const BoxExtents b = box_extents(s);
    const float kpad = box_kpad(a.box_quad, (double)a.box_kc, (double)a.box_kc, b.e1, b.e2);
    a.boxes[at] = BoxRec{b.c[0], b.c[1], b.c[2], fold_kpad(b.e[0], kpad), fold_kpad(b.e[1], kpad), fold_kpad(b.e[2], kpad)};
    a.boxes_open[at] = BoxRec{b.c[0], b.c[1], b.c[2], kBoxOpenExtent, kBoxOpenExtent, kBoxOpenExtent};
}

// The top records as the matrix-core sweep's A operand for D = I, relative to the kept origin (bounds.h, mfma_row): one lane per
// row (record) of a tile.  After the top level's kernel in stream order.
__global__ void __launch_bounds__(kRefitBlock) refit_mfma_kernel(const RefitArgs a) {
    const uint32_t g = blockIdx.x * kRefitBlock + threadIdx.x;
    if (g >= a.n_padded) return;
    const uint32_t t = g / 32u, m = g % 32u;
    uint16_t row[16];
    mfma_row(relative_record(a.clusters[mfma_source_record(t, m)], a.origin), row);
    uint16_t* const o = a.top_mfma + (size_t)t * 512;
#pragma unroll
    for (uint32_t q = 0; q < 16; q++) o[mfma_slot(m, q)] = row[q];
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

int launch_material_scatter(const MaterialScatterArgs& a, void* stream) {
    if (a.count == 0 || a.count > kMaterialBatch) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(material_scatter_kernel, dim3((a.count + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, (hipStream_t)stream, a);
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
