// Budget allocation on the device (mrt_noise_query_budget, include/myraytracer_amd.h): mrt_budget_allocate's definition as one
// total order, selected in parallel.  Candidate (t, j) has the 104-bit key (G, j, t), compared most significant part first:
//   mandatory (n_t + j < 2 and j < min(2, max_frames)): G = 0
//   gain: G = ~bits(g'(t, j)), g' the running minimum from j = m_t of s'_t * (K(n_t + j) - K(n_t + j + 1)) in double, which ends
//         at the first value that is not > 0; only for s'_t > 0, finite, and n_t + m_t >= 2
// A positive finite double orders as its bits, so ascending keys are "mandatory by j then t, then g' descending, j ascending, t
// ascending" (a gain's G has its top bit set: never 0).  Keys are unique; the allocation is the `budget` smallest, k_t = those of
// tile t.  Within a tile the keys ascend with j, so k_t is also the number of the tile's keys <= the budget-th smallest key T.
//
// T by radix select, 8-bit digits: 0..7 = G's bytes from the top, 8 = j, 9..12 = t's bytes from the top.  budget_pass_kernel<p>
// adds to hist[p][.] the digit p of every candidate whose digits 0 .. p-1 are T's; the launches are in stream order, so launch p
// reads the finished histograms 0 .. p-1 and every workgroup replays the selection from them (budget_replay: 256 counts a step,
// one wave): no workgroup waits for another, nothing but integer sums crosses workgroups.  When the step takes a whole bin the
// rest of T is all ones and the later launches return at once -- the usual case after G's digits, gains being distinct.  A tile's
// at most 32 gains are recomputed in every pass, not stored.  budget_count_kernel then writes k_t and the blocks' sums P_b,
// budget_sum_kernel adds those in block order (the header's blocked order).  No float atomics; every loop is bounded by
// max_frames, the tile count or the digit count.
#include <hip/hip_runtime.h>
#include "mrt_internal.h"

namespace mrt {
namespace {

constexpr uint32_t kBudgetBlock = 256;               // threads per workgroup: one tile each, four blocks of 64 tiles
constexpr uint32_t kBudgetMaxGrid = 2048;            // workgroups at most; the tiles beyond are grid-strided
constexpr uint64_t kLoMask = (1ull << 40) - 1;       // (j << 32) | t
static_assert(kBudgetBlock == kBudgetBins && kBudgetBlock % kBudgetSumTiles == 0 && kBudgetSumTiles == 64, "one bin a thread, one wave a block of sums");

// the candidates of tile t in ascending key order: emit(G, (j << 32) | t)
template <typename F>
__device__ __forceinline__ void budget_candidates(const BudgetArgs& a, uint32_t t, F&& emit) {
    const float sf = a.s[t];
    const double st = sf >= 0.0f ? (double)sf : 0.0;                 // (a NaN compares false)
    const uint32_t n = a.n ? a.n[t] : a.n_uniform;
    const uint32_t m = n < 2u ? min(2u - n, a.max_frames) : 0u;
    for (uint32_t j = 0; j < m; j++) emit(0ull, ((uint64_t)j << 32) | t);
    if (!(st > 0.0) || __builtin_isinf(st) || n + m < 2u) return;
    double g = __builtin_inf();
    for (uint32_t j = m; j < a.max_frames; j++) {
        const double x = st * (a.K[n + j] - a.K[n + j + 1]);
        g = x < g ? x : g;
        if (!(g > 0.0)) break;
        emit(~(uint64_t)__double_as_longlong(g), ((uint64_t)j << 32) | t);
    }
}

// lane i's value, i the same in every lane: two scalar lane reads, so a chain of additions over the lanes waits for no LDS round trip
__device__ __forceinline__ double lane_value(double v, uint32_t i) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)b, (int)i), hi = __builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), (int)i);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__device__ __forceinline__ uint32_t budget_digit(uint64_t hi, uint64_t lo, uint32_t d) {
    return (uint32_t)(d < 8u ? hi >> (56u - 8u * d) : lo >> (32u - 8u * (d - 8u))) & 255u;
}

// The selection after `passes` digits.  mode 0: digits 0 .. passes-1 of T are fixed in (hi, lo) and `want` of the candidates that
// share them are to be taken, smallest first; 1: T is (hi, lo) entirely; 2: nothing is taken (budget 0, or no candidate).
struct BudgetSel { uint64_t hi, lo, want; uint32_t mode; };

// one wave; every lane returns the same value
__device__ BudgetSel budget_replay(const uint32_t* __restrict__ hist, uint32_t passes, uint64_t budget) {
    const uint32_t lane = threadIdx.x & 63u;
    BudgetSel r{0ull, 0ull, budget, budget == 0 ? 2u : 0u};
    uint4 counts[kBudgetDigits];                         // every finished histogram at once: the steps below depend on each other, the loads do not
#pragma unroll
    for (uint32_t q = 0; q < kBudgetDigits; q++)
        counts[q] = q < passes ? reinterpret_cast<const uint4*>(hist + q * kBudgetBins)[lane] : make_uint4(0u, 0u, 0u, 0u);   // bins 4 lane .. 4 lane + 3
#pragma unroll
    for (uint32_t q = 0; q < kBudgetDigits; q++) {
        if (q >= passes || r.mode != 0) break;
        const uint4 c = counts[q];
        const uint64_t own = (uint64_t)c.x + c.y + c.z + c.w;
        uint64_t incl = own;
#pragma unroll
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint64_t up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        const uint64_t total = __shfl(incl, 63);
        if (q == 0 && total == 0) { r.mode = 2; break; }
        if (q == 0 && r.want >= total) {                 // fewer candidates than the budget: all of them
            r.hi = ~0ull; r.lo = kLoMask; r.mode = 1;
            break;
        }
        // the bin that holds the want-th of these candidates: 1 <= want <= total, so exactly one lane's range does
        const uint64_t excl = incl - own;
        const uint32_t owner = (uint32_t)__ffsll((unsigned long long)__ballot(excl < r.want && r.want <= incl)) - 1u;
        uint32_t bin = 4u * lane, cnt = c.x;
        uint64_t below = excl;
        if (below + cnt < r.want) { below += cnt; bin++; cnt = c.y; }
        if (bin == 4u * lane + 1u && below + cnt < r.want) { below += cnt; bin++; cnt = c.z; }
        if (bin == 4u * lane + 2u && below + cnt < r.want) { below += cnt; bin++; cnt = c.w; }
        bin = __shfl(bin, owner); cnt = __shfl(cnt, owner); below = __shfl(below, owner);
        if (q < 8u) r.hi |= (uint64_t)bin << (56u - 8u * q);
        else r.lo |= (uint64_t)bin << (32u - 8u * (q - 8u));
        r.want -= below;
        if (r.want == cnt) {                             // the whole bin: every key with these digits
            if (q < 7u) r.hi |= ~0ull >> (8u * (q + 1u));
            if (q < 8u) r.lo = kLoMask;
            else if (q < 12u) r.lo |= kLoMask >> (8u * (q - 7u));
            r.mode = 1;
        }
    }
    if (r.mode == 0 && passes == kBudgetDigits) r.mode = 1;      // (keys are unique: want is 1 here)
    return r;
}

__global__ void __launch_bounds__(kBudgetBlock) budget_init_kernel(uint32_t* __restrict__ hist, mrt_budget_result* __restrict__ res) {
    for (uint32_t i = threadIdx.x; i < kBudgetDigits * kBudgetBins; i += kBudgetBlock) hist[i] = 0u;
    if (threadIdx.x < sizeof(mrt_budget_result) / 4u)
        reinterpret_cast<uint32_t*>(res)[threadIdx.x] = threadIdx.x == 0 ? (uint32_t)sizeof(mrt_budget_result) : 0u;
}

__global__ void __launch_bounds__(kBudgetBlock) budget_pass_kernel(BudgetArgs a, uint32_t p) {
    __shared__ uint32_t bins[kBudgetBins];
    __shared__ BudgetSel sel;
    bins[threadIdx.x] = 0u;
    if (threadIdx.x < 64u) {
        const BudgetSel r = budget_replay(a.hist, p, a.budget);
        if (threadIdx.x == 0) sel = r;
    }
    __syncthreads();
    if (sel.mode != 0) return;                           // T is known (or nothing is taken): the same in every workgroup
    const uint64_t hi = sel.hi, lo = sel.lo;
    const uint64_t mask_hi = p >= 8u ? ~0ull : p == 0 ? 0ull : ~0ull << (64u - 8u * p);
    const uint64_t mask_lo = p <= 8u ? 0ull : kLoMask & (~0ull << (40u - 8u * (p - 8u)));
    for (uint32_t t = blockIdx.x * kBudgetBlock + threadIdx.x; t < a.n_tiles; t += gridDim.x * kBudgetBlock) {
        uint32_t run_digit = 0xFFFFFFFFu, run = 0;       // a tile's keys ascend: equal digits are consecutive
        budget_candidates(a, t, [&](uint64_t G, uint64_t jt) {
            if (((G ^ hi) & mask_hi) != 0 || ((jt ^ lo) & mask_lo) != 0) return;
            const uint32_t d = budget_digit(G, jt, p);
            if (d != run_digit) {
                if (run) atomicAdd(&bins[run_digit], run);
                run_digit = d; run = 0;
            }
            run++;
        });
        if (run) atomicAdd(&bins[run_digit], run);
    }
    __syncthreads();
    const uint32_t mine = bins[threadIdx.x];
    if (mine) atomicAdd(&a.hist[p * kBudgetBins + threadIdx.x], mine);
}

// k_t, the integer fields of the result, and P_b of both variance sums: wave w of a workgroup takes the block of 64 tiles
// 4 (workgroup's chunk) + w, so a lane's tile is 64 b + lane
__global__ void __launch_bounds__(kBudgetBlock) budget_count_kernel(BudgetArgs a) {
    __shared__ BudgetSel sel;
    if (threadIdx.x < 64u) {
        const BudgetSel r = budget_replay(a.hist, kBudgetDigits, a.budget);
        if (threadIdx.x == 0) sel = r;
    }
    __syncthreads();
    const uint64_t hi = sel.hi, lo = sel.lo;
    const bool none = sel.mode == 2u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t chunks = (a.n_tiles + kBudgetBlock - 1) / kBudgetBlock;
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const uint32_t t = chunk * kBudgetBlock + threadIdx.x;
        const uint32_t first = t - lane;                 // of this wave's block of 64
        if (first >= a.n_tiles) continue;                // (wave-uniform)
        uint32_t k = 0;
        double before = 0.0, after = 0.0;
        if (t < a.n_tiles) {
            if (!none)
                budget_candidates(a, t, [&](uint64_t G, uint64_t jt) { k += (G < hi || (G == hi && jt <= lo)) ? 1u : 0u; });
            a.k_out[t] = k;
            const uint32_t n = a.n ? a.n[t] : a.n_uniform;
            if (n >= 2u) {
                const float sf = a.s[t];
                const double st = sf >= 0.0f ? (double)sf : 0.0;
                before = st * a.K[n];
                after = st * a.K[n + k];
            }
        }
        // P_b: the sequential sum from 0.0 over the block's tiles, ascending (every lane adds the same chain)
        const uint32_t count = min(64u, a.n_tiles - first);
        double pb = 0.0, pa = 0.0;
        for (uint32_t i = 0; i < count; i++) {
            pb += lane_value(before, i);
            pa += lane_value(after, i);
        }
        uint32_t sum = k, most = k, used = k ? 1u : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sum += __shfl_xor(sum, off);
            used += __shfl_xor(used, off);
            most = max(most, __shfl_xor(most, off));
        }
        if (lane == 0) {
            const uint32_t b = first / kBudgetSumTiles, blocks = (a.n_tiles + kBudgetSumTiles - 1) / kBudgetSumTiles;
            a.sums[b] = pb;
            a.sums[blocks + b] = pa;
            if (sum) {
                atomicAdd(reinterpret_cast<unsigned long long*>(&a.res->tile_frames), (unsigned long long)sum);
                atomicAdd(&a.res->tiles, used);
                atomicMax(&a.res->frames, most);
            }
        }
    }
}

// var_before / var_after: the sequential sum from 0.0 of P_b over ascending b.  One wave.
__global__ void __launch_bounds__(64) budget_sum_kernel(BudgetArgs a) {
    const uint32_t lane = threadIdx.x, blocks = (a.n_tiles + kBudgetSumTiles - 1) / kBudgetSumTiles;
    double vb = 0.0, va = 0.0;
    for (uint32_t base = 0; base < blocks; base += 64u) {
        const bool in = base + lane < blocks;
        const double b = in ? a.sums[base + lane] : 0.0, f = in ? a.sums[blocks + base + lane] : 0.0;
        const uint32_t count = min(64u, blocks - base);
        for (uint32_t i = 0; i < count; i++) {
            vb += lane_value(b, i);
            va += lane_value(f, i);
        }
    }
    if (lane == 0) {
        a.res->var_before = vb;
        a.res->var_after = va;
    }
}

}  // namespace

int launch_budget_plan(const BudgetArgs& a, void* stream) {
    if (a.n_tiles == 0 || a.max_frames < 1 || a.max_frames > kMaxFrameBatch) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t chunks = (a.n_tiles + kBudgetBlock - 1) / kBudgetBlock, grid = chunks < kBudgetMaxGrid ? chunks : kBudgetMaxGrid;
    hipLaunchKernelGGL(budget_init_kernel, dim3(1), dim3(kBudgetBlock), 0, st, a.hist, a.res);
    for (uint32_t p = 0; p < kBudgetDigits; p++) hipLaunchKernelGGL(budget_pass_kernel, dim3(grid), dim3(kBudgetBlock), 0, st, a, p);
    hipLaunchKernelGGL(budget_count_kernel, dim3(grid), dim3(kBudgetBlock), 0, st, a);
    hipLaunchKernelGGL(budget_sum_kernel, dim3(1), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace mrt
