// Camera-ray cluster masks (the proof sketch: DESIGN_HISTORY.md §4): for a small scene with at most kCamMaskRecords
// top records, one 128-bit entry per 8 consecutive texels of the shard's row-major texel order -- entry e covers texels 8 e ..
// 8 e + 7 -- in the sweep's own bit layout (record 32 w + i at bit 31 - i of word w).  A bit is set whenever ANY camera ray the
// render kernel can generate for ANY texel of the entry (any jitter, any lens point, either camera mode) could have a reference
// discriminant >= 0 against ANY member of that cluster, unless the member lies entirely behind the ray's origin.  The render
// kernel ANDs the entry onto the sweep's candidate words of its camera rays (kernels.hip).
//
// The bundle of one texel: a ray runs from O + off, |off| <= rho in the lens plane, through O + p, with p in the texel's patch
// around pc, |p - pc| <= h; at the affine parameter s >= 0 its point O + off + s (p - off) lies within |1 - s| rho + s h of the
// axis point O + s pc.  Every member sphere is tested against that widening axis in double, its radius inflated for the
// reference's own rounding (bounds.h, box_kpad: the line of a ray whose computed discriminant is >= 0 passes within
// sqrt(r^2 + 14 eps |oc|^2 / a) of the centre; twice that here) and rho, h and the positions widened by 1e-5 relative.
// The kernel reads the device's own member records (level 0 of `nodes`, members 4 m .. 4 m + 3 of cluster m), so it is right after
// mrt_update_spheres and mrt_regroup_spheres; it creates nothing and runs in stream order.
//
// Camera-ray sphere lists: the same launch and the same member loop also keep the per-member answer the cluster bit is the OR of.
// List entry e (the masks' indexing) is 4 words: x = the number of level-0 member slots whose bundle test passes for any valid
// texel of the entry, at most kCamListCap, or kCamListOverflow when there are more; y, z, w = their slot ids in ascending order,
// 10 bits each (a small scene's slots are below 1,024), id k at bits 10 k .. 10 k + 9 of the 96-bit word w:z:y.  The render
// kernel resolves the camera ray of a texel against its entry's slots in the lane (kernels.hip, primary hit); an overflowed
// entry's camera rays take world_hit.
#include <hip/hip_runtime.h>
#include "mrt_internal.h"

namespace mrt {
namespace {

constexpr uint32_t kCamMaskBlock = 256;
constexpr uint32_t kCamMaskMembers = kClusterK * kCamMaskRecords;
constexpr double kCamMaskMargin = 1.0e-5;               // relative widening of rho, h and the positions
constexpr double kCamMaskRound = 28.0 * 0x1p-23;        // 2 x (14 eps), eps taken as 2^-23: E = kCamMaskRound |oc|^2

// Does the widening axis O + s pc, s >= 0, of half width |1 - s| rho + s hp come within R of the centre?  q = O - centre, Q2 =
// q.q, P2 = pc.pc.  On [0, 1] the allowance is a1 + b1 s, on [1, inf) a2 + b2 s (both >= 0 there), so either piece asks for the
// minimum of the quadratic |q + s pc|^2 - (a + b s)^2 = A s^2 + 2 B s + C over its interval: the ends, and the vertex where it is
// a minimum inside.  A cone at least as wide as its axis is long (A2 <= 0) reaches everything.
__device__ __forceinline__ bool bundle_touches(double qx, double qy, double qz, double Q2, double R, double px, double py, double pz,
                                               double P2, double hp, double rho) {
    const double D = qx * px + qy * py + qz * pz;
    const double a1 = R + rho, b1 = hp - rho, a2 = R - rho, b2 = hp + rho;
    const double C1 = Q2 - a1 * a1;
    if (C1 <= 0.0) return true;                                     // s = 0
    const double A1 = P2 - b1 * b1, B1 = D - a1 * b1;
    if (A1 + 2.0 * B1 + C1 <= 0.0) return true;                     // s = 1
    if (A1 > 0.0 && B1 < 0.0 && -B1 < A1 && C1 * A1 <= B1 * B1) return true;
    const double A2 = P2 - b2 * b2, B2 = D - a2 * b2, C2 = Q2 - a2 * a2;
    if (A2 <= 0.0) return true;
    return -B2 > A2 && C2 * A2 <= B2 * B2;
}

// One thread per entry.  The workgroup first leaves every member's (O - centre, inflated radius) in LDS.
__global__ void __launch_bounds__(kCamMaskBlock) cam_mask_kernel(const KParams P, uint32_t* __restrict__ out, uint32_t* __restrict__ lists,
                                                                  uint32_t entries) {
    __shared__ double mem[kCamMaskMembers][4];
    const uint32_t W = P.locals.shape[0], H = P.locals.shape[1];
    const uint32_t local_rows = P.tiles_x ? (P.n_tiles / P.tiles_x) * kBandRows : 0u;
    const uint32_t n_top = P.n_padded < kCamMaskRecords ? P.n_padded : kCamMaskRecords;
    // the camera as the render kernel's new_sample_head / new_sample_lens read it; mode 0: the pinhole at the origin
    double O[3] = {0.0, 0.0, 0.0}, su[3] = {1.0, 0.0, 0.0}, sv[3] = {0.0, 1.0, 0.0}, fw[3] = {0.0, 0.0, 1.0};
    double rho = 0.0;
    if (P.cam.mode != 0) {
        double uu = 0.0, vv = 0.0, uv = 0.0;
        for (int k = 0; k < 3; k++) {
            O[k] = (double)P.cam.origin[k]; su[k] = (double)P.cam.su[k]; sv[k] = (double)P.cam.sv[k]; fw[k] = (double)P.cam.fw[k];
            uu += (double)P.cam.ru[k] * (double)P.cam.ru[k]; vv += (double)P.cam.rv[k] * (double)P.cam.rv[k];
            uv += (double)P.cam.ru[k] * (double)P.cam.rv[k];
        }
        // |lx ru + ly rv|^2 <= max(|ru|^2, |rv|^2) + |ru.rv| on the unit disk
        if (P.cam.defocus != 0) rho = sqrt(fmax(uu, vv) + fabs(uv)) * (1.0 + kCamMaskMargin);
    }
    const double o_len = sqrt(O[0] * O[0] + O[1] * O[1] + O[2] * O[2]);
    const double kappa = kCamMaskMargin * (o_len + rho);            // the rounding of the ray's own origin, at every s
    for (uint32_t m = threadIdx.x; m < kClusterK * n_top; m += kCamMaskBlock) {
        double R = -1.0, qx = 0.0, qy = 0.0, qz = 0.0;
        if (m < P.direct_first) {                                   // the hierarchy's part of level 0
            const SphereRec s = P.nodes[m];
            const double r2 = -(double)s.neg_r2;
            if (r2 >= 0.0 && r2 < 1.0e30) {                         // (a never-hit padding slot: neg_r2 = +inf)
                qx = O[0] - (double)s.cx; qy = O[1] - (double)s.cy; qz = O[2] - (double)s.cz;
                const double oc = sqrt(qx * qx + qy * qy + qz * qz) + rho;
                R = sqrt(r2 + kCamMaskRound * oc * oc) + kappa;
            }
        }
        mem[m][0] = qx; mem[m][1] = qy; mem[m][2] = qz; mem[m][3] = R;
    }
    __syncthreads();
    const uint32_t e = blockIdx.x * kCamMaskBlock + threadIdx.x;
    if (e >= entries) return;
    // the entry's texels: the centre of the texel's patch of the focal plane, pc, and the patch's half diagonal
    const double ps = (double)(2.0f / (float)H);                    // fs_main :373, as the kernel rounds it
    double suu = 0.0, svv = 0.0, suv = 0.0;
    for (int k = 0; k < 3; k++) { suu += su[k] * su[k]; svv += sv[k] * sv[k]; suv += su[k] * sv[k]; }
    const double half = 0.5 * ps;
    const double h = sqrt(half * half * (suu + svv + 2.0 * fabs(suv)));
    double pcx[8], pcy[8], pcz[8], P2[8], hp[8];
    uint32_t valid = 0;
#pragma unroll
    for (uint32_t t = 0; t < 8; t++) {
        const uint64_t texel = 8ull * e + t;
        const uint32_t lrow = (uint32_t)(texel / W), px = (uint32_t)(texel % W);
        const uint32_t py = ((lrow / kBandRows) * P.shard_world + P.shard_rank) * kBandRows + (lrow % kBandRows);
        pcx[t] = pcy[t] = pcz[t] = P2[t] = hp[t] = 0.0;
        if (lrow >= local_rows || py >= H) continue;
        const double vx = (((double)px + 0.5) - 0.5 * (double)W) * ps + half;          // fs_main :374, the jitter's mid-point
        const double vy = (((double)py + 0.5) - 0.5 * (double)H) * ps + half;
        pcx[t] = vx * su[0] + vy * sv[0] - fw[0];
        pcy[t] = vx * su[1] + vy * sv[1] - fw[1];
        pcz[t] = vx * su[2] + vy * sv[2] - fw[2];
        P2[t] = pcx[t] * pcx[t] + pcy[t] * pcy[t] + pcz[t] * pcz[t];
        hp[t] = h * (1.0 + kCamMaskMargin) + kCamMaskMargin * sqrt(P2[t]);
        valid |= 1u << t;
    }
    uint32_t words[4] = {0u, 0u, 0u, 0u};
    uint32_t count = 0;
    uint64_t ids_lo = 0, ids_hi = 0;                                // the list's 96 bits: ids 0 .. 5 and a part of 6 | the rest
    for (uint32_t c = 0; c < n_top; c++) {
        bool set = false;
        for (uint32_t k = 0; k < kClusterK; k++) {
            const uint32_t slot = kClusterK * c + k;
            const double qx = mem[slot][0], qy = mem[slot][1], qz = mem[slot][2];
            const double R = mem[slot][3];
            if (!(R >= 0.0)) continue;
            const double Q2 = qx * qx + qy * qy + qz * qz;
            bool touched = false;
#pragma unroll
            for (uint32_t t = 0; t < 8; t++)
                if (!touched && (valid >> t & 1u) != 0u) touched = bundle_touches(qx, qy, qz, Q2, R, pcx[t], pcy[t], pcz[t], P2[t], hp[t], rho);
            if (!touched) continue;
            set = true;
            if (count < kCamListCap) {
                const uint32_t pos = 10u * count;
                if (pos < 64u) ids_lo |= (uint64_t)slot << pos;
                if (pos + 10u > 64u) ids_hi |= pos >= 64u ? (uint64_t)slot << (pos - 64u) : (uint64_t)slot >> (64u - pos);
            }
            count++;
        }
        if (set) words[c >> 5] |= 0x80000000u >> (c & 31u);
    }
    reinterpret_cast<uint4*>(out)[e] = make_uint4(words[0], words[1], words[2], words[3]);
    reinterpret_cast<uint4*>(lists)[e] = count <= kCamListCap ? make_uint4(count, (uint32_t)ids_lo, (uint32_t)(ids_lo >> 32), (uint32_t)ids_hi)
                                                               : make_uint4(kCamListOverflow, 0u, 0u, 0u);
}

}  // namespace

int launch_cam_masks(const KParams& p, uint32_t* masks, uint32_t* lists, uint32_t entries, void* stream) {
    if (entries == 0) return 0;
    hipLaunchKernelGGL(cam_mask_kernel, dim3((entries + kCamMaskBlock - 1) / kCamMaskBlock), dim3(kCamMaskBlock), 0, (hipStream_t)stream,
                       p, masks, lists, entries);
    return (int)hipGetLastError();
}

}  // namespace mrt
