// m2s_lodbudget.hip — the search behind m2s_lod_select_budget (include/m2s.h): the smallest tau_px, as the bits of a float, at which the
// cut of m2s_lod_select holds at most N records.  No counterpart in the reference.  The pinned comparison is monotone in tau_px, so
// every node is selected on one interval of keys [L, H); the count of a key is #{L <= key} - #{H <= key} over the nodes with L < H, it
// does not increase with the key, and the smallest key that fits is found by a radix descent over the two planes: no sort, no bisection
// on the host.  The cut itself is m2s_lod.hip's sweep at the tau found.
//
//   k_lod_thresholds   one launch per level from the coarsest to the leaves, as the sweep: per node above the leaves d2 and s*s once,
//                      then T = the smallest key whose tau does not refine it, built from its top bit down: T >= c exactly when
//                      key c - 1 refines (31 trips in registers, the very expression of the sweep: tau*tau rounded first, then times d2).  Writes
//                      (L, H) = (leaf ? 0 : T, min(L, H) of the parent; 0xFFFFFFFF on the last level): 8 B.  Reads 16 + 4 B per node
//                      above the leaves, 4 B per leaf (a leaf's own bound never matters: it is drawn whenever its ancestors refine),
//                      and 8 B gathered from the parent, which neighbours share.
//   k_lod_budget_hist  round p = 0..3, digit = bits [24 - 8p, 32 - 8p): the nodes with L < H, grid-stride; an L whose higher digits equal
//                      the prefix found so far goes into 256 LDS bins, an H likewise into 256 more (a wave whose lanes hold one digit
//                      sends one atomicAdd: the leaves' L is 0, and thresholds of one scene share their top digits).  Non-zero bins leave
//                      with one integer atomicAdd each into one of kLodBudgetShards copies.
//   k_lod_budget_pick  one workgroup: inclusive prefix sums of (L bins - H bins) in wrapping 32-bit arithmetic; `below` + sum[b] is the
//                      count at the largest key of digit b, and the first digit at which it fits carries the answer.  Prefix, `below`
//                      (the count just under the prefix's range) and the count at the key in front of the answer stay on the device,
//                      so the four rounds run back to back.
// m2s_lod_select_budget_frustum runs the kVis instances of k_lod_thresholds (a node without a leaf inside the frustum gets L = H: selected
// at no key) and k_lod_budget_pick<true> (the budget raised to the visible nodes of the last level, on the device).
// Atomics on ONE word retire one after the other on MI355X (m2s_budget.hip): few, large workgroups and sharded bins.  Integer atomics
// only: every count is the same from run to run.  Vector stores only.
#include <algorithm>

#include "../../include/m2s.h"
#include "m2s_device.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr uint32_t kLodBudgetGrid = 512;   // workgroups of the two grid-stride kernels at most: two per CU

// nodes [first, first + n) of one level.  kTop: no parents; kLeaf: L = 0, the bound is not read.  kVis (the budget over a frustum): a
// node whose visibility byte is 0 gets L = H, so it is selected at no key, and its children inherit the H it was given (+1 B read per
// node; its 31 trips are skipped).  The kVis = false instances are the plain search's.
template <bool kTop, bool kLeaf, bool kVis>
__global__ void __launch_bounds__(256) k_lod_thresholds(const float4* __restrict__ bounds, const uint32_t* __restrict__ parent, uint32_t first, uint32_t n,
                                                        LodSelectK k, uint2* __restrict__ lh, const uint8_t* __restrict__ vis) {
    const uint32_t stride = gridDim.x * 256u;
    for (unsigned long long t = blockIdx.x * 256u + threadIdx.x; t < n; t += stride) {       // (64 bits: t + stride may pass 2^32)
        const uint32_t i = first + (uint32_t)t;
        uint32_t L = 0u;
        bool seen = true;
        if (kVis) seen = vis[i] != 0;
        if (!kLeaf && seen) {
            const float4 b = bounds[i];
            const float dx = b.x - k.cx, dy = b.y - k.cy, dz = b.z - k.cz;
            const float d2 = fmaxf((dx * dx + dy * dy) + dz * dz, k.near2);
            const float s = b.w * k.focal;
            const float ss = s * s;
            // refine(key) is true on [0, T) and false from T on (false for every key above 0x7F7FFFFF: tau*tau is +inf or NaN), so
            // T >= c exactly when key c - 1 refines: T is built from its top bit down
#pragma unroll 1
            for (uint32_t bit = 0x40000000u; bit; bit >>= 1) {
                const float tau = __uint_as_float((L | bit) - 1u);
                const float tau2 = tau * tau;
                if (ss > tau2 * d2) L |= bit;
            }
        }
        uint32_t H = 0xFFFFFFFFu;
        if (!kTop) {
            const uint2 p = lh[parent[i]];
            H = p.x < p.y ? p.x : p.y;
        }
        if (kVis && !seen) L = H;
        lh[i] = make_uint2(L, H);
    }
}

// one key of a lane into the workgroup's bins; `in`: it takes part in this round.  Called by whole waves.
__device__ __forceinline__ void lod_count_digit(uint32_t* bins, bool in, uint32_t d) {
    const unsigned long long act = __ballot(in);
    if (!act) return;
    const uint32_t first = (uint32_t)__builtin_ctzll(act);
    const uint32_t d0 = (uint32_t)__shfl((int)d, (int)first);
    if (__ballot(in && d != d0) == 0ull) {
        if ((threadIdx.x & 63u) == first) atomicAdd(&bins[d0], (uint32_t)__popcll(act));
    } else if (in) {
        atomicAdd(&bins[d], 1u);
    }
}

__global__ void __launch_bounds__(256) k_lod_budget_hist(const uint2* __restrict__ lh, uint32_t n, uint32_t pass, uint32_t* __restrict__ state) {
    __shared__ uint32_t bins[512];                                      // [0, 256): L, [256, 512): H
    bins[threadIdx.x] = 0;
    bins[256u + threadIdx.x] = 0;
    __syncthreads();
    const uint32_t shift = 24u - 8u * pass;
    const uint32_t high_mask = pass == 0u ? 0u : ~(0xFFFFFFFFu >> (8u * pass));
    const uint32_t want = state[kLodBudgetPrefix] & high_mask;
    const uint32_t stride = gridDim.x * 256u;
    // (every lane of a workgroup makes the same number of trips: lod_count_digit's ballots are over whole waves)
    for (unsigned long long base = blockIdx.x * 256u; base < n; base += stride) {           // (64 bits: base + stride may pass 2^32)
        const unsigned long long i = base + threadIdx.x;
        const bool live = i < n;
        const uint2 v = live ? lh[i] : make_uint2(0u, 0u);
        const bool some = live && v.x < v.y;                            // selected at some key
        lod_count_digit(bins, some && (v.x & high_mask) == want, (v.x >> shift) & 255u);
        lod_count_digit(bins + 256, some && (v.y & high_mask) == want, (v.y >> shift) & 255u);
    }
    __syncthreads();
    uint32_t* const out = state + kLodBudgetHist + 512u * (kLodBudgetShards * pass + (blockIdx.x & (kLodBudgetShards - 1u)));
    const uint32_t a = bins[threadIdx.x], b = bins[256u + threadIdx.x];
    if (a) atomicAdd(&out[threadIdx.x], a);
    if (b) atomicAdd(&out[256u + threadIdx.x], b);
}

// kRaise (the budget over a frustum): the budget is at least count(0x7F7FFFFF), which round 0 reads off its own sums at digit 0x7F (no L
// or H lies in 0x7F800000 .. 0x7FFFFFFF: the count at 0x7FFFFFFF is the one at 0x7F7FFFFF) and the later rounds find in the state.
template <bool kRaise>
__global__ void __launch_bounds__(256) k_lod_budget_pick(uint32_t pass, uint32_t budget, uint32_t* __restrict__ state) {
    __shared__ uint32_t sum[256];
    const uint32_t t = threadIdx.x;
    uint32_t d = 0;
#pragma unroll
    for (uint32_t s = 0; s < kLodBudgetShards; ++s) {
        const uint32_t* const h = state + kLodBudgetHist + 512u * (kLodBudgetShards * pass + s);
        d += h[t] - h[256u + t];                                        // (wraps; the sums below are counts again: in [0, nodes])
    }
    const uint32_t below = state[kLodBudgetBelow];                      // (read by every lane in front of the barriers, written behind them)
    uint32_t v = d;
    sum[t] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t o = 1; o < 256u; o <<= 1) {
        const uint32_t add = t >= o ? sum[t - o] : 0u;
        __syncthreads();
        v += add;
        sum[t] = v;
        __syncthreads();
    }
    // count(largest key of digit t) = below + v, not increasing in t, and it fits at t = 255 (round 0: no node is left there; later
    // rounds: the key the round before chose).  Exactly one digit is the first that fits.
    const uint32_t before = below + (v - d);                            // the count at the key in front of digit t's range
    if (kRaise) {
        if (pass == 0u) {
            const uint32_t last = sum[0x7Fu];                           // (below is 0 in round 0)
            budget = budget > last ? budget : last;
            if (t == 0u) state[kLodBudgetEff] = budget;
        } else {
            budget = state[kLodBudgetEff];
        }
    }
    if (below + v <= budget && (t == 0u || before > budget)) {
        state[kLodBudgetPrefix] |= t << (24u - 8u * pass);
        state[kLodBudgetBelow] = before;
        if (t) state[kLodBudgetFiner] = before;
    }
}

template <bool kVis>
hipError_t lod_thresholds_levels(const LodLevelsK& t, const LodSelectK& k, uint2* lh, const uint8_t* vis, hipStream_t st) {
    for (uint32_t l = t.levels; l-- > 0;) {
        const uint32_t f = (uint32_t)t.first[l], n = (uint32_t)(t.first[l + 1] - t.first[l]);
        if (!n) continue;
        const dim3 grid(std::min((n + 255u) / 256u, 2u * kLodBudgetGrid)), block(256);
        const bool top = l + 1 == t.levels, leaf = l == 0;
        if (top && leaf) hipLaunchKernelGGL((k_lod_thresholds<true, true, kVis>), grid, block, 0, st, t.bounds, t.parent, f, n, k, lh, vis);
        else if (top) hipLaunchKernelGGL((k_lod_thresholds<true, false, kVis>), grid, block, 0, st, t.bounds, t.parent, f, n, k, lh, vis);
        else if (leaf) hipLaunchKernelGGL((k_lod_thresholds<false, true, kVis>), grid, block, 0, st, t.bounds, t.parent, f, n, k, lh, vis);
        else hipLaunchKernelGGL((k_lod_thresholds<false, false, kVis>), grid, block, 0, st, t.bounds, t.parent, f, n, k, lh, vis);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t lod_thresholds(const LodLevelsK& t, const LodSelectK& k, uint2* lh, const uint8_t* vis, hipStream_t st) {
    return vis ? lod_thresholds_levels<true>(t, k, lh, vis, st) : lod_thresholds_levels<false>(t, k, lh, nullptr, st);
}

hipError_t lod_budget_search(const uint2* lh, uint32_t n, uint32_t budget, bool raise_to_last, uint32_t* state, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(state, 0, kLodBudgetStateWords * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    const uint32_t blocks = (uint32_t)(((unsigned long long)n + 1023ull) / 1024ull);       // four trips per lane at least, where there are that many
    const dim3 grid(std::max(1u, std::min(blocks, kLodBudgetGrid))), block(256);
    for (uint32_t pass = 0; pass < 4u; ++pass) {
        hipLaunchKernelGGL(k_lod_budget_hist, grid, block, 0, st, lh, n, pass, state);
        if (raise_to_last) hipLaunchKernelGGL(k_lod_budget_pick<true>, dim3(1), block, 0, st, pass, budget, state);
        else hipLaunchKernelGGL(k_lod_budget_pick<false>, dim3(1), block, 0, st, pass, budget, state);
    }
    return hipGetLastError();
}

}  // namespace m2s
