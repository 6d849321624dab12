// m2s_budget.hip — the selection behind m2s_prune_budget (include/m2s.h): of the candidates, the max_records with the largest 32-bit key,
// ties broken by index.  No counterpart in the reference, whose cap keeps whatever arrives first.  A radix select, not a sort: the 4-byte
// words are read a handful of times and nothing moves until the compaction (m2s_contrib.hip: k_prune_compact).
//
//   k_budget_keys   one lane per record, grid-stride: the key of the pin (the only float arithmetic of the pass), bit 31 set on a record
//                   that is not a candidate — a key is the bits of a non-negative float, so bit 31 of a candidate's word is always clear.
//                   The candidates are counted in a register, then per workgroup, and leave as ONE integer atomicAdd per workgroup.
//   k_budget_hist   pass p = 0..3, digit = bits [24 - 8p, 32 - 8p) of the key: the candidates whose higher digits equal the prefix found
//                   so far, counted into 256 LDS bins per workgroup (a wave whose lanes all hold the same digit sends one atomicAdd, not
//                   64 to one bank: the top digit of weights of one scene takes few values), non-zero bins flushed with one global
//                   integer atomicAdd each.  Four keys (16 bytes) per lane and trip, grid-stride.  Leaves at once when the candidates
//                   fit the budget.
//   k_budget_pick   one workgroup: the suffix sums of the 256 bins from the top, the digit at which they cross the remaining quota;
//                   prefix and quota stay in device memory, so the four rounds run back to back.
//   k_budget_ties   tie[i] = candidate and key == T; the host scans them (rocPRIM) into ranks
//   k_budget_flags  keep[i] = candidate and (key > T or (tie and rank < quota)); every candidate when nothing had to be selected
// Atomics on ONE word retire one after the other, about 11 ns each on MI355X (42 788 waves adding to one counter took 0.49 ms where the
// loads take 0.01): hence few, large workgroups' worth of work per atomic (at most kBudgetGrid workgroups) and kBudgetShards copies of the
// counter and of every bin, chosen by workgroup and summed by their readers.  Integer atomics only: every count is the same from run to
// run.  Vector stores only.
#include <rocprim/device/device_scan.hpp>

#include "m2s_device.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr uint32_t kNotCandidate = 0x80000000u;
constexpr uint32_t kBudgetGrid = 512;      // workgroups of the two grid-stride kernels: two per CU

// the bits of p where p > 0, else 0: a NaN, a zero of either sign and (never produced by the pin's inputs) a negative value give key 0
__device__ __forceinline__ uint32_t key_bits(float p) { return p > 0.0f ? __float_as_uint(p) : 0u; }

__device__ __forceinline__ uint32_t candidates_of(const uint32_t* state) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t s = 0; s < kBudgetShards; ++s) c += state[kBudgetCandidates + s];
    return c;
}

__global__ void __launch_bounds__(256) k_budget_keys(const float4* __restrict__ rec, const uint32_t* __restrict__ wmax,
                                                     const uint32_t* __restrict__ npix, uint32_t n, uint32_t importance, float min_weight,
                                                     uint32_t min_pixels, uint32_t* __restrict__ keys, uint32_t* __restrict__ state) {
    __shared__ uint32_t wave_count[4];
    uint32_t mine = 0;
    const uint32_t stride = gridDim.x * 256u;
    for (unsigned long long i = blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {      // (64 bits: i + stride may pass 2^32)
        uint32_t key;
        bool cand;
        if (importance == 0u) {                                         // M2S_IMPORTANCE_VIEWS
            const float w = __uint_as_float(wmax[i]);
            const uint32_t k = npix[i];
            cand = w > min_weight && k >= min_pixels;                   // m2s_prune's test (k_prune_flags)
            key = key_bits(__uint2float_rn(k) * w);
        } else {                                                        // M2S_IMPORTANCE_AREA
            const float4 color = rec[(size_t)6 * i + 1], scale = rec[(size_t)6 * i + 2];
            const float a = fminf(fmaxf(color.w, 0.0f), 1.0f);
            const float s = fabsf(scale.x) * fabsf(scale.y);
            cand = true;
            key = key_bits(s * a);
        }
        keys[i] = cand ? key : (key | kNotCandidate);
        mine += cand ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o);
    if ((threadIdx.x & 63u) == 0u) wave_count[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t c = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
        if (c) atomicAdd(&state[kBudgetCandidates + (blockIdx.x & (kBudgetShards - 1u))], c);
    }
}

// one key of a lane into the workgroup's bins; `in`: it takes part in this round.  Called by whole waves.
__device__ __forceinline__ void count_digit(uint32_t* bins, bool in, uint32_t d) {
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

__global__ void __launch_bounds__(256) k_budget_hist(const uint32_t* __restrict__ keys, uint32_t n, uint32_t pass, uint32_t budget,
                                                     uint32_t* __restrict__ state) {
    if (candidates_of(state) <= budget) return;                         // nothing to select (uniform over the grid)
    __shared__ uint32_t bins[256];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t shift = 24u - 8u * pass;
    const uint32_t prefix = state[kBudgetPrefix];
    // the digits above this pass's: in front of pass 0 bit 31 alone decides (a candidate's is clear, and so is the prefix's)
    const uint32_t high_mask = pass == 0u ? kNotCandidate : ~(0xFFFFFFFFu >> (8u * pass));
    const uint32_t want = prefix & high_mask;
    const uint32_t n4 = n / 4u;                                         // whole groups of four keys (the buffer is 256-byte aligned)
    const uint4* keys4 = reinterpret_cast<const uint4*>(keys);
    const uint32_t stride = gridDim.x * 256u;
    // (every lane of a workgroup makes the same number of trips: count_digit's ballots are over whole waves)
    for (uint32_t base = blockIdx.x * 256u; base < n4; base += stride) {                    // (n4 < 2^30: no wrap)
        const uint32_t g = base + threadIdx.x;
        const bool live = g < n4;
        const uint4 k = live ? keys4[g] : make_uint4(kNotCandidate, kNotCandidate, kNotCandidate, kNotCandidate);
        count_digit(bins, live && (k.x & high_mask) == want, (k.x >> shift) & 255u);
        count_digit(bins, live && (k.y & high_mask) == want, (k.y >> shift) & 255u);
        count_digit(bins, live && (k.z & high_mask) == want, (k.z >> shift) & 255u);
        count_digit(bins, live && (k.w & high_mask) == want, (k.w >> shift) & 255u);
    }
    if (blockIdx.x == 0u) {                                             // the last n % 4 keys
        const uint32_t i = 4u * n4 + threadIdx.x;
        const bool live = threadIdx.x < n - 4u * n4;
        const uint32_t k = live ? keys[i] : kNotCandidate;
        count_digit(bins, live && (k & high_mask) == want, (k >> shift) & 255u);
    }
    __syncthreads();
    const uint32_t c = bins[threadIdx.x];
    if (c) atomicAdd(&state[kBudgetHist + 256u * (kBudgetShards * pass + (blockIdx.x & (kBudgetShards - 1u))) + threadIdx.x], c);
}

__global__ void __launch_bounds__(256) k_budget_pick(uint32_t pass, uint32_t budget, uint32_t* __restrict__ state) {
    if (candidates_of(state) <= budget) return;
    __shared__ uint32_t suf[256];
    const uint32_t t = threadIdx.x;
    uint32_t h = 0;
#pragma unroll
    for (uint32_t s = 0; s < kBudgetShards; ++s) h += state[kBudgetHist + 256u * (kBudgetShards * pass + s) + t];
    const uint32_t quota = pass == 0u ? budget : state[kBudgetQuota];
    // inclusive suffix sums: suf[t] = the candidates of this round with digit >= t (sums of counts of distinct records: below 2^32)
    uint32_t v = h;
    suf[t] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t o = 1; o < 256u; o <<= 1) {
        const uint32_t add = t + o < 256u ? suf[t + o] : 0u;
        __syncthreads();
        v += add;
        suf[t] = v;
        __syncthreads();
    }
    // exactly one digit: those above it do not fill the quota, those from it upwards do (the round holds at least `quota` candidates)
    const uint32_t above = v - h;
    if (above < quota && quota <= v) {
        const uint32_t shift = 24u - 8u * pass;
        const uint32_t prefix = state[kBudgetPrefix] | (t << shift);
        state[kBudgetPrefix] = prefix;
        state[kBudgetQuota] = quota - above;
        if (pass == 3u) {
            state[kBudgetActive] = 1u;
            state[kBudgetTies] = h;                                     // candidates with key == T; quota - above of them are kept
        }
    }
}

__global__ void __launch_bounds__(256) k_budget_ties(const uint32_t* __restrict__ keys, uint32_t n, const uint32_t* __restrict__ state,
                                                     uint32_t* __restrict__ tie) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    tie[i] = (state[kBudgetActive] && keys[i] == state[kBudgetPrefix]) ? 1u : 0u;     // (a word with bit 31 set equals no T)
}

__global__ void __launch_bounds__(256) k_budget_flags(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ rank, uint32_t n,
                                                      const uint32_t* __restrict__ state, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    bool keep = !(k & kNotCandidate);
    if (keep && state[kBudgetActive]) {
        const uint32_t T = state[kBudgetPrefix];
        keep = k > T || (k == T && rank[i] < state[kBudgetQuota]);
    }
    flags[i] = keep ? 1u : 0u;
}

}  // namespace

hipError_t budget_select(const float4* rec, const uint32_t* wmax, const uint32_t* npix, uint32_t n, uint32_t importance, float min_weight,
                         uint32_t min_pixels, uint32_t budget, uint32_t* keys, uint32_t* state, uint32_t* flags, uint32_t* offsets, void* temp,
                         size_t temp_bytes, const m2s_host::StageMarks& marks, hipStream_t st) {
    const uint32_t blocks = (uint32_t)(((unsigned long long)n + 255ull) / 256ull);
    const dim3 grid(blocks), block(256);
    hipError_t e = hipMemsetAsync(state, 0, kBudgetStateWords * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_budget_keys, dim3(blocks < kBudgetGrid ? blocks : kBudgetGrid), block, 0, st, rec, wmax, npix, n, importance, min_weight,
                       min_pixels, keys, state);
    const uint32_t hist_blocks = (blocks + 3u) / 4u;
    const dim3 hist_grid(hist_blocks < kBudgetGrid ? hist_blocks : kBudgetGrid);
    for (uint32_t pass = 0; pass < 4u; ++pass) {
        hipLaunchKernelGGL(k_budget_hist, hist_grid, block, 0, st, keys, n, pass, budget, state);
        hipLaunchKernelGGL(k_budget_pick, dim3(1), block, 0, st, pass, budget, state);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = marks.mark(0, st)) != hipSuccess) return e;
    // the ties' ranks pass through the two words per record the compaction is about to use: tie in `flags`, rank in `offsets`
    hipLaunchKernelGGL(k_budget_ties, grid, block, 0, st, keys, n, state, flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = rocprim::exclusive_scan(temp, temp_bytes, (const uint32_t*)flags, offsets, 0u, (size_t)n, rocprim::plus<uint32_t>(), st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_budget_flags, grid, block, 0, st, keys, offsets, n, state, flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = rocprim::exclusive_scan(temp, temp_bytes, (const uint32_t*)flags, offsets, 0u, (size_t)n, rocprim::plus<uint32_t>(), st)) != hipSuccess) return e;
    if ((e = marks.mark(1, st)) != hipSuccess) return e;
    return hipSuccess;
}

hipError_t preload_budget() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_budget_keys)); }

}  // namespace m2s
