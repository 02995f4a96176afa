// The judgement behind mrt_set_auto_regroup (world.cpp; include/myraytracer_amd.h "scene"): has the hierarchy loosened enough for a
// regroup to pay?  The figure is DESIGN.md 7f's, the sum of R^2 over the nodes of each level, read off the records the refit has
// just written -- view independent, a few thousand loads -- and the decision stays on the device: the kernel writes the gate word
// that the kernels of launch_regroup, queued behind it, read (regroup.hip), so the host never waits to learn it.
//   The figure is compared with an earlier value of itself by a ratio and against tests/regroup_policy_ref.py bit for bit, so the
// order of the additions is fixed and the same at every launch: ONE workgroup of kQualityThreads lanes; lane l adds the records
// j = l, l + kQualityThreads, .. of a level in ascending order; lane 0 adds the lanes' partials in lane order; the levels are
// added from level 1 up.  No atomics, no shuffles whose order a compiler could choose, and -ffp-contract=off as everywhere.
#include <hip/hip_runtime.h>
#include "mrt_internal.h"

namespace mrt {
namespace {

constexpr uint32_t kQualityThreads = 256;

__global__ void __launch_bounds__(kQualityThreads) regroup_quality_kernel(const QualityArgs a) {
    __shared__ double part[kQualityThreads];
    RegroupState* const s = a.state;
    // (uniform over the workgroup, and before any barrier)
    if (a.mode == kQualityBaseline && !a.mark && s->pending == 0u) return;
    const uint32_t tid = threadIdx.x;
    double q = 0.0, q_level[kMaxLevels] = {0.0, 0.0, 0.0, 0.0};
    for (uint32_t k = 1; k <= a.levels; k++) {
        const SphereRec* const recs = k == a.levels ? a.clusters : a.nodes + a.level_base[k];
        const uint32_t n_k = k == a.levels ? a.n_padded : (k + 1 < a.levels ? a.level_base[k + 1] : a.n_nodes) - a.level_base[k];
        // the nodes whose span of clusters [j 4^(k-1), ..) begins inside the pool
        const uint32_t span = 1u << (2 * (k - 1));
        const uint32_t n = min(n_k, (a.n_pool + span - 1) / span);
        double sum = 0.0;
        for (uint32_t j = tid; j < n; j += kQualityThreads) {
            const float v = recs[j].neg_r2;
            if (v != INFINITY) sum += (double)(-v);
        }
        part[tid] = sum;
        __syncthreads();
        if (tid == 0) {
            double total = 0.0;
            for (uint32_t l = 0; l < kQualityThreads; l++) total += part[l];
            q_level[k - 1] = total;
            q = k == 1 ? total : q + total;
        }
        __syncthreads();
    }
    if (tid != 0) return;
    for (uint32_t k = 0; k < kMaxLevels; k++) s->q_level[k] = q_level[k];
    s->q_last = q;
    if (a.mode == kQualityBaseline) {
        s->q_ref = q;
        s->pending = 0u;
        return;
    }
    s->checks = s->checks + 1ull;
    if (s->pending != 0u) {
        s->q_ref = q;
        s->pending = 0u;
        s->gate = 0u;
    } else if (q > (double)a.ratio * s->q_ref) {
        s->gate = 1u;
        s->pending = 1u;
        s->regroups = s->regroups + 1ull;
    } else {
        s->gate = 0u;
    }
}

}  // namespace

int launch_regroup_quality(const QualityArgs& a, void* stream) {
    static_assert(kMaxLevels == 4, "q_level's initialiser");
    if (a.levels < 1 || a.levels > kMaxLevels || a.n_pool < 2 || !a.state) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(regroup_quality_kernel, dim3(1), dim3(kQualityThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mrt
