// The regroup behind mrt_regroup_spheres (world.cpp; include/myraytracer_amd.h "scene"): the pooled spheres permuted over the
// member slots they already occupy, so that the groups mean something again after the spheres have moved.  Node j of level k
// covers the member slots [j 4^k, (j+1) 4^k), so the grouping IS member_index: nothing else is written here, and refit.hip's
// launch_refit, queued behind it, derives every bound from the new order.
//
// The ordering is tests/regroup_ref.py's, reproduced bit for bit.  Clusters [0, n_pool) hold the pool; pref[k] = the real member
// slots of the clusters before k.  Depth d cuts the clusters into aligned segments of size0 >> d (size0 = n_pool rounded up to a
// power of two; only the last segment can be short).  A segment longer than half its size is sorted -- stably, by the key form
// of the f32 centre coordinate along the axis on which its centres extend furthest -- and falls into its two halves at the next
// depth; a shorter one passes through.  All segments of a depth are sorted by ONE sort on the composite key
//     segment (12 bits) | key (32 bits) | rank in the current order (20 bits)
// whose low bits make it stable (and every key distinct: a bitonic network sorts it deterministically).
//   Depths whose segments are wider than a block of `block` clusters run over global memory: a box kernel (segmented min / max
// of the keys by atomics, one per wave where the wave's lanes share a segment), a key kernel, a bitonic sort whose steps below
// 2,048 elements run in LDS, and a gather of the order.  The rest -- every remaining depth of a block, at most 2,048 spheres --
// is one workgroup of regroup_block_kernel in LDS, which then writes member_index: the spheres at ranks [pref[k], pref[k+1]) to
// the real slots of cluster k, ascending by index (build_clusters' rule).  A pool of at most `block` clusters is that one launch.
//   (The build's -ffp-contract=off holds here too; the only float operation is the extent hi - lo.)
#include <hip/hip_runtime.h>
#include "mrt_internal.h"

namespace mrt {
namespace {

constexpr uint32_t kThreads = 1024;                 // the block kernel and the LDS sort: two elements a thread
constexpr uint32_t kFlat = 256;                     // the one-element-a-thread kernels
constexpr uint32_t kRankBits = 20, kKeyBits = 32;
constexpr uint32_t kRankMask = (1u << kRankBits) - 1u;
static_assert(kMaxSpheres <= (1u << kRankBits), "a rank fits the composite key's low bits");
static_assert(kRegroupChunk == 2 * kThreads && kRegroupChunk <= 2048, "two elements a thread; a local rank fits 11 bits");

// the total order of f32 as an integer: -0.0 before +0.0
__device__ __forceinline__ uint32_t key_of(float v) {
    const uint32_t u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// the first axis on which the box (min x, y, z, max x, y, z in key form) extends furthest, extents in f32
__device__ __forceinline__ uint32_t widest_axis(const uint32_t* box) {
    float ext[3];
#pragma unroll
    for (int q = 0; q < 3; q++) ext[q] = value_of(box[3 + q]) - value_of(box[q]);
    uint32_t q = 0;
    if (ext[1] > ext[0]) q = 1;
    if (ext[2] > ext[q]) q = 2;
    return q;
}

// is segment `seg` of the depth with segments of `size` clusters, over clusters [0, n), sorted there (longer than half its size)?
__device__ __forceinline__ bool segment_sorted(uint32_t seg, uint32_t size, uint32_t n) {
    const uint32_t first = seg * size, len = (n - first < size ? n - first : size);
    return len > size / 2;
}

__device__ __forceinline__ uint64_t composite(uint32_t seg, uint32_t key, uint32_t rank) {
    return ((uint64_t)seg << (kKeyBits + kRankBits)) | ((uint64_t)key << kRankBits) | rank;
}

// One element of a segmented min / max into box[6 seg ..]: where the wave's active lanes share a segment, one lane adds the
// wave's result; otherwise every lane adds its own.  Called by every lane of the wave (`active`: this lane has an element).
template <typename Box>
__device__ __forceinline__ void box_add(Box* box, bool active, uint32_t seg, const uint32_t k[3]) {
    const unsigned long long mask = __ballot(active);
    if (mask == 0ull) return;
    const int lead = __ffsll((long long)mask) - 1;
    const uint32_t seg0 = (uint32_t)__shfl((int)seg, lead);
    if (__all(!active || seg == seg0)) {
        uint32_t lo[3], hi[3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            lo[q] = active ? k[q] : 0xFFFFFFFFu;
            hi[q] = active ? k[q] : 0u;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                lo[q] = min(lo[q], (uint32_t)__shfl_xor((int)lo[q], off));
                hi[q] = max(hi[q], (uint32_t)__shfl_xor((int)hi[q], off));
            }
        }
        if ((int)(threadIdx.x & 63u) == lead) {
#pragma unroll
            for (int q = 0; q < 3; q++) { atomicMin(&box[6 * seg0 + q], lo[q]); atomicMax(&box[6 * seg0 + 3 + q], hi[q]); }
        }
    } else if (active) {
#pragma unroll
        for (int q = 0; q < 3; q++) { atomicMin(&box[6 * seg + q], k[q]); atomicMax(&box[6 * seg + 3 + q], k[q]); }
    }
}

// Bitonic steps on n keys in LDS (n a power of two, at most kRegroupChunk), the keys being the elements [gbase, gbase + n) of a
// sort whose direction at stage k is ascending where (index & k) == 0: stages k_first .. k_last, of each the steps j < n.
// Every thread of the workgroup calls it; the keys are in place and visible (a barrier has passed) before and after.
__device__ __forceinline__ void lds_bitonic(uint64_t* sh, uint32_t n, uint32_t gbase, uint32_t k_first, uint32_t k_last) {
    for (uint32_t k = k_first; k != 0 && k <= k_last; k <<= 1) {
        for (uint32_t j = (k >> 1) < (n >> 1) ? (k >> 1) : (n >> 1); j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < n / 2; t += kThreads) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
                const bool up = ((gbase + i) & k) == 0u;
                const uint64_t x = sh[i], y = sh[l];
                if ((x > y) == up) { sh[i] = y; sh[l] = x; }
            }
            __syncthreads();
        }
    }
}

// The gate of a regroup queued behind the auto-regroup policy's judgement (regroup_policy.hip): null, or a word that kernel wrote --
// 0: the hierarchy is good enough, every kernel of launch_regroup returns at once.  One uniform read for the whole grid, taken
// before any barrier or LDS use, so that no barrier is ever reached by part of a workgroup.
__device__ __forceinline__ bool gate_shut(const uint32_t* gate) { return gate != nullptr && *gate == 0u; }

// ---- the depths above a block: global memory ----

__global__ void __launch_bounds__(kFlat) regroup_box_clear_kernel(uint32_t* box, uint32_t n_seg, const uint32_t* gate) {
    if (gate_shut(gate)) return;
    const uint32_t i = blockIdx.x * kFlat + threadIdx.x;
    if (i < 6u * n_seg) box[i] = (i % 6u) < 3u ? 0xFFFFFFFFu : 0u;
}

// one lane per rank of the current order: its centre into its segment's box (only sorted segments read theirs)
__global__ void __launch_bounds__(kFlat) regroup_box_kernel(const RegroupArgs a, const uint32_t* order, const uint32_t* clus,
                                                            uint32_t* box, uint32_t size) {
    if (gate_shut(a.gate)) return;
    const uint32_t i = blockIdx.x * kFlat + threadIdx.x;
    const bool active = i < a.pooled;
    uint32_t seg = 0, k[3] = {0, 0, 0};
    if (active) {
        const SphereRec s = a.spheres[order[i]];
        seg = clus[i] / size;
        k[0] = key_of(s.cx); k[1] = key_of(s.cy); k[2] = key_of(s.cz);
    }
    box_add(box, active, seg, k);
}

__global__ void __launch_bounds__(kFlat) regroup_key_kernel(const RegroupArgs a, const uint32_t* order, const uint32_t* clus,
                                                            const uint32_t* box, uint32_t size, uint64_t* keys, uint32_t n_sort) {
    if (gate_shut(a.gate)) return;
    const uint32_t i = blockIdx.x * kFlat + threadIdx.x;
    if (i >= n_sort) return;
    uint64_t key = ~0ull;                                   // the padding sorts last
    if (i < a.pooled) {
        const uint32_t seg = clus[i] / size;
        uint32_t k32 = 0;                                   // a segment that passes through keeps its order
        if (segment_sorted(seg, size, a.n_pool)) {
            const SphereRec s = a.spheres[order[i]];
            const uint32_t q = widest_axis(box + 6 * seg);
            k32 = key_of(q == 0 ? s.cx : q == 1 ? s.cy : s.cz);
        }
        key = composite(seg, k32, i);
    }
    keys[i] = key;
}

// the stages k_first .. k_last of the sort of n_sort keys, the steps below kRegroupChunk: one chunk a workgroup, in LDS
__global__ void __launch_bounds__(kThreads) regroup_sort_local_kernel(uint64_t* keys, uint32_t k_first, uint32_t k_last, const uint32_t* gate) {
    __shared__ uint64_t sh[kRegroupChunk];
    if (gate_shut(gate)) return;
    const uint32_t gbase = blockIdx.x * kRegroupChunk;
    for (uint32_t t = threadIdx.x; t < kRegroupChunk; t += kThreads) sh[t] = keys[gbase + t];
    __syncthreads();
    lds_bitonic(sh, kRegroupChunk, gbase, k_first, k_last);
    for (uint32_t t = threadIdx.x; t < kRegroupChunk; t += kThreads) keys[gbase + t] = sh[t];
}

// step j >= kRegroupChunk of stage k: one compare-exchange a lane
__global__ void __launch_bounds__(kFlat) regroup_sort_step_kernel(uint64_t* keys, uint32_t n_sort, uint32_t k, uint32_t j, const uint32_t* gate) {
    if (gate_shut(gate)) return;
    const uint32_t t = blockIdx.x * kFlat + threadIdx.x;
    if (t >= n_sort / 2) return;
    const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), l = i | j;
    const bool up = (i & k) == 0u;
    const uint64_t x = keys[i], y = keys[l];
    if ((x > y) == up) { keys[i] = y; keys[l] = x; }
}

__global__ void __launch_bounds__(kFlat) regroup_gather_kernel(const uint64_t* keys, const uint32_t* order, uint32_t* order_out, uint32_t pooled,
                                                               const uint32_t* gate) {
    if (gate_shut(gate)) return;
    const uint32_t i = blockIdx.x * kFlat + threadIdx.x;
    if (i >= pooled) return;
    const uint32_t rank = (uint32_t)keys[i] & kRankMask;
    if (rank < pooled) order_out[i] = order[rank];
}

// ---- a block: every remaining depth in LDS, then member_index ----
//
// Workgroup w takes the clusters [a, b) = [w block, min(n_pool, (w + 1) block)) and the ranks [pref[a], pref[b]) of `order`,
// at most kRegroupChunk of them.  The centres stay where they were loaded (by local id, in key form); ord[] is the local id at
// every local rank.  50 KiB of static LDS and 1,024 threads: two workgroups a CU by the waves (32 a CU), three by the 160 KiB of
// LDS -- the waves decide, so 8 waves a SIMD while a block sorts.
__global__ void __launch_bounds__(kThreads) regroup_block_kernel(const RegroupArgs a, const uint32_t* order, const uint32_t* clus,
                                                                 const uint32_t* pref, uint32_t size0) {
    __shared__ uint64_t keys[kRegroupChunk];
    __shared__ uint32_t ck[3][kRegroupChunk];
    __shared__ uint32_t box[6 * (kRegroupBlock / 2)];
    __shared__ uint16_t ord[kRegroupChunk];
    if (gate_shut(a.gate)) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t c0 = blockIdx.x * a.block, c1 = min(a.n_pool, c0 + a.block), nc = c1 - c0;
    const uint32_t r0 = pref[c0], cnt = pref[c1] - r0;
    if (cnt > kRegroupChunk) return;                        // (never: a cluster has at most kClusterK real slots)
    uint32_t n2 = 2;
    while (n2 < cnt) n2 <<= 1;
    uint32_t my_clus[2] = {0, 0};                           // the local cluster of my two ranks: a rank's cluster never changes
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const uint32_t i = tid + e * kThreads;
        if (i < cnt) {
            const SphereRec s = a.spheres[order[r0 + i]];
            ck[0][i] = key_of(s.cx); ck[1][i] = key_of(s.cy); ck[2][i] = key_of(s.cz);
            ord[i] = (uint16_t)i;
            my_clus[e] = clus[r0 + i] - c0;
        }
    }
    __syncthreads();
    for (uint32_t size = min(a.block, size0); size >= 2; size >>= 1) {
        const uint32_t n_seg = (nc + size - 1) / size;
        if (n_seg == 1 && nc <= size / 2) continue;         // the one segment passes through (uniform over the workgroup)
        for (uint32_t x = tid; x < 6 * n_seg; x += kThreads) box[x] = (x % 6u) < 3u ? 0xFFFFFFFFu : 0u;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const uint32_t i = tid + e * kThreads;
            const bool active = i < cnt;
            uint32_t k[3] = {0, 0, 0};
            if (active) { const uint32_t id = ord[i]; k[0] = ck[0][id]; k[1] = ck[1][id]; k[2] = ck[2][id]; }
            box_add(box, active, my_clus[e] / size, k);
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const uint32_t i = tid + e * kThreads;
            if (i >= n2) continue;
            uint64_t key = ~0ull;
            if (i < cnt) {
                const uint32_t seg = my_clus[e] / size;
                uint32_t k32 = 0;
                if (segment_sorted(seg, size, nc)) k32 = ck[widest_axis(box + 6 * seg)][ord[i]];
                key = composite(seg, k32, i);
            }
            keys[i] = key;
        }
        __syncthreads();
        lds_bitonic(keys, n2, 0u, 2u, n2);
        uint32_t moved[2] = {0, 0};
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const uint32_t i = tid + e * kThreads;
            if (i < cnt) moved[e] = ord[((uint32_t)keys[i] & kRankMask) & (kRegroupChunk - 1u)];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const uint32_t i = tid + e * kThreads;
            if (i < cnt) ord[i] = (uint16_t)moved[e];
        }
        __syncthreads();
    }
    // cluster k's spheres, ascending by index, into its real slots: the first of its kClusterK (build_clusters pads behind them)
    for (uint32_t k = tid; k < nc; k += kThreads) {
        const uint32_t lo = pref[c0 + k] - r0, m = min(pref[c0 + k + 1] - r0 - lo, kClusterK);
        uint32_t v[kClusterK];
#pragma unroll
        for (uint32_t q = 0; q < kClusterK; q++) v[q] = q < m ? order[r0 + ord[lo + q]] : 0xFFFFFFFFu;
#define MRT_CSWAP(x, y) { const uint32_t lo_ = min(v[x], v[y]), hi_ = max(v[x], v[y]); v[x] = lo_; v[y] = hi_; }
        MRT_CSWAP(0, 1) MRT_CSWAP(2, 3) MRT_CSWAP(0, 2) MRT_CSWAP(1, 3) MRT_CSWAP(1, 2)
#undef MRT_CSWAP
#pragma unroll
        for (uint32_t q = 0; q < kClusterK; q++)
            if (q < m) a.member_index[(size_t)kClusterK * (c0 + k) + q] = v[q];
    }
}

uint32_t pow2_ceil(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

}  // namespace

void regroup_plan(uint32_t n_pool, uint32_t block, uint32_t out[3]) {
    if (block < 4 || block > kRegroupBlock || (block & (block - 1))) block = kRegroupBlock;
    const uint32_t size0 = pow2_ceil(n_pool ? n_pool : 1);
    while (block < kRegroupBlock && size0 / (2 * block) > kRegroupMaxSegments) block <<= 1;
    uint32_t above = 0, within = 0;
    for (uint32_t size = size0; size >= 2; size >>= 1) (size > block ? above : within)++;
    out[0] = block; out[1] = above; out[2] = within;
}

int launch_regroup(const RegroupArgs& a_in, void* stream) {
    static_assert(kClusterK == 4, "the block kernel's sorting network");
    if (a_in.n_pool < 2 || a_in.pooled < a_in.n_pool || a_in.pooled > (uint64_t)kClusterK * a_in.n_pool || a_in.pooled > kMaxSpheres)
        return (int)hipErrorInvalidValue;
    uint32_t plan[3];
    regroup_plan(a_in.n_pool, a_in.block, plan);
    RegroupArgs a = a_in;
    a.block = plan[0];
    hipStream_t st = (hipStream_t)stream;
    const RegroupLayout L = regroup_layout(a.n_pool, a.pooled);
    const uint32_t* const clus = a.scratch + L.clus;
    const uint32_t* const pref = a.scratch + L.pref;
    uint32_t* const box = a.scratch + L.box;
    uint64_t* const keys = reinterpret_cast<uint64_t*>(a.scratch + L.keys);
    const uint32_t size0 = pow2_ceil(a.n_pool), n_sort = L.n_sort;
    const uint32_t* order = a.scratch + L.pool;
    uint32_t turn = 0;
    auto blocks = [](uint32_t n) { return dim3((n + kFlat - 1) / kFlat); };
    for (uint32_t size = size0; size > a.block; size >>= 1) {
        const uint32_t n_seg = (a.n_pool + size - 1) / size;
        hipLaunchKernelGGL(regroup_box_clear_kernel, blocks(6 * n_seg), dim3(kFlat), 0, st, box, n_seg, a.gate);
        hipLaunchKernelGGL(regroup_box_kernel, blocks(a.pooled), dim3(kFlat), 0, st, a, order, clus, box, size);
        hipLaunchKernelGGL(regroup_key_kernel, blocks(n_sort), dim3(kFlat), 0, st, a, order, clus, (const uint32_t*)box, size, keys, n_sort);
        hipLaunchKernelGGL(regroup_sort_local_kernel, dim3(n_sort / kRegroupChunk), dim3(kThreads), 0, st, keys, 2u, kRegroupChunk, a.gate);
        for (uint32_t k = 2 * kRegroupChunk; k != 0 && k <= n_sort; k <<= 1) {
            for (uint32_t j = k >> 1; j >= kRegroupChunk; j >>= 1)
                hipLaunchKernelGGL(regroup_sort_step_kernel, blocks(n_sort / 2), dim3(kFlat), 0, st, keys, n_sort, k, j, a.gate);
            hipLaunchKernelGGL(regroup_sort_local_kernel, dim3(n_sort / kRegroupChunk), dim3(kThreads), 0, st, keys, k, k, a.gate);
        }
        uint32_t* const out = a.scratch + L.ord[turn];
        hipLaunchKernelGGL(regroup_gather_kernel, blocks(a.pooled), dim3(kFlat), 0, st, (const uint64_t*)keys, order, out, a.pooled, a.gate);
        order = out;
        turn ^= 1u;
    }
    hipLaunchKernelGGL(regroup_block_kernel, dim3((a.n_pool + a.block - 1) / a.block), dim3(kThreads), 0, st, a, order, clus, pref, size0);
    return (int)hipGetLastError();
}

}  // namespace mrt
