// m2s_lod.hip — the kernels behind m2s_lod_build and m2s_lod_select (include/m2s.h): the level-of-detail tree is a chain of m2s_merge
// steps kept and linked, the cut is one sweep over its nodes.  No counterpart in the reference, which draws every Gaussian it converted.
//
//   k_lod_link      after every step that merged: parent = first node of the new level + the merge's map, for the level below; the
//                   16-byte bound (position, longer edge of the flat footprint) of every new node.  The last level gets M2S_LOD_NO_PARENT.
//                   k_lod_link_gauss: the same with pin 4g's bound, for a tree built under M2S_MERGE_MODEL_GAUSSIAN.
//   k_lod_select    one launch per level, from the coarsest to the leaves, on one stream: a lane reads its bound (16 B), its parent (4 B)
//                   and the parent's `open` byte (a gather, but the parents of neighbouring nodes are neighbours: every level above the
//                   leaves is in the merge's Morton order), evaluates the pinned comparison, writes its own `open` byte (not for leaves:
//                   nobody reads it) and its selection flag (4 B, what the scan and k_prune_compact take).  26 B per node above the
//                   leaves, 25 B per leaf; the 96-byte records are not touched.  Grid-stride over at most kLodGrid workgroups; the
//                   selected and refining nodes are counted in registers, then per wave, then per workgroup, and leave as at most two
//                   integer atomicAdds per workgroup (one word per level and one for the refining nodes: atomics on ONE word retire
//                   one after the other on MI355X, m2s_budget.hip).  Integer sums: the same from run to run.
//                   The kVis instances (m2s_lod_select_frustum) mask the selection with the visibility byte of m2s_lodfrustum.hip
//                   (+1 B per node) and count the unmasked selection as a third sum.
//   k_lod_ids       ids[offsets[i]] = i for every selected node: which node each output record is
// The scan of the flags is rocPRIM's, as m2s_prune's; the compaction is m2s_prune's own kernel.  Vector stores only.
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "../../include/m2s.h"
#include "m2s_device.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr uint32_t kLodGrid = 1024;        // workgroups of the sweep at most: four per CU

__global__ void __launch_bounds__(256) k_lod_link(const uint32_t* __restrict__ map, uint32_t n_map, uint32_t offset, uint32_t* __restrict__ parent,
                                                  const float4* __restrict__ rec, uint32_t n_rec, float4* __restrict__ bounds) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < n_map) parent[t] = map ? offset + map[t] : M2S_LOD_NO_PARENT;
    if (t < n_rec) {
        const float4 p = rec[(size_t)6 * t], s = rec[(size_t)6 * t + 2];
        bounds[t] = make_float4(p.x, p.y, p.z, fmaxf(fabsf(s.x), fabsf(s.y)));
    }
}

// Pin 4g (a tree built under M2S_MERGE_MODEL_GAUSSIAN): the bound is one standard deviation along the longest of the three axes
__global__ void __launch_bounds__(256) k_lod_link_gauss(const uint32_t* __restrict__ map, uint32_t n_map, uint32_t offset, uint32_t* __restrict__ parent,
                                                        const float4* __restrict__ rec, uint32_t n_rec, float sigma, float4* __restrict__ bounds) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < n_map) parent[t] = map ? offset + map[t] : M2S_LOD_NO_PARENT;
    if (t < n_rec) {
        const float4 p = rec[(size_t)6 * t], s = rec[(size_t)6 * t + 2];
        bounds[t] = make_float4(p.x, p.y, p.z, sigma * fmaxf(fmaxf(fabsf(s.x), fabsf(s.y)), fabsf(s.z)));
    }
}

// the pinned comparison: one rounding per operation, no contraction
__device__ __forceinline__ bool lod_refines(const float4 b, const LodSelectK& k) {
    const float dx = b.x - k.cx, dy = b.y - k.cy, dz = b.z - k.cz;
    const float d2 = fmaxf((dx * dx + dy * dy) + dz * dz, k.near2);
    const float s = b.w * k.focal;
    return s * s > k.tau2 * d2;
}

// nodes [first, first + n) of one level.  kTop: no parents (every node's ancestors refine, vacuously); kLeaf: no `open` byte to write,
// and a leaf that refines is still selected.  kVis (the cuts over a frustum, m2s_lodfrustum.hip builds the plane): a selected node whose
// visibility byte is 0 is dropped (+1 B read per node); what the plain cut selects is counted beside what is left, in the same launch.
// The kVis = false instances are the plain cut's.
template <bool kTop, bool kLeaf, bool kVis>
__global__ void __launch_bounds__(256) k_lod_select(const float4* __restrict__ bounds, const uint32_t* __restrict__ parent, uint32_t first, uint32_t n,
                                                    LodSelectK k, uint8_t* __restrict__ open, uint32_t* __restrict__ flags,
                                                    uint32_t* __restrict__ selected_word, uint32_t* __restrict__ refine_word,
                                                    const uint8_t* __restrict__ vis, uint32_t* __restrict__ plain_word) {
    __shared__ uint32_t wave_sel[4], wave_ref[4];
    uint32_t n_sel = 0, n_ref = 0, n_plain = 0;
    const uint32_t stride = gridDim.x * 256u;
    for (unsigned long long t = blockIdx.x * 256u + threadIdx.x; t < n; t += stride) {       // (64 bits: t + stride may pass 2^32)
        const uint32_t i = first + (uint32_t)t;
        const bool refine = lod_refines(bounds[i], k);
        bool above = true;
        if (!kTop) above = open[parent[i]] != 0;
        bool sel = above && (kLeaf || !refine);
        if (!kLeaf) open[i] = (refine && above) ? 1 : 0;
        if (kVis) {
            n_plain += sel ? 1u : 0u;
            sel = sel && vis[i] != 0;
        }
        flags[i] = sel ? 1u : 0u;
        n_sel += sel ? 1u : 0u;
        n_ref += refine ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        n_sel += (uint32_t)__shfl_xor((int)n_sel, o);
        n_ref += (uint32_t)__shfl_xor((int)n_ref, o);
    }
    if ((threadIdx.x & 63u) == 0u) { wave_sel[threadIdx.x >> 6] = n_sel; wave_ref[threadIdx.x >> 6] = n_ref; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t a = (wave_sel[0] + wave_sel[1]) + (wave_sel[2] + wave_sel[3]);
        const uint32_t b = (wave_ref[0] + wave_ref[1]) + (wave_ref[2] + wave_ref[3]);
        if (a) atomicAdd(selected_word, a);
        if (b) atomicAdd(refine_word, b);
    }
    if (kVis) {                                                         // (a third sum, after the two of the plain cut)
        __shared__ uint32_t wave_plain[4];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) n_plain += (uint32_t)__shfl_xor((int)n_plain, o);
        if ((threadIdx.x & 63u) == 0u) wave_plain[threadIdx.x >> 6] = n_plain;
        __syncthreads();
        if (threadIdx.x == 0u) {
            const uint32_t p = (wave_plain[0] + wave_plain[1]) + (wave_plain[2] + wave_plain[3]);
            if (p) atomicAdd(plain_word, p);
        }
    }
}

__global__ void __launch_bounds__(256) k_lod_ids(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offsets, uint32_t n,
                                                 uint32_t* __restrict__ ids) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && flags[i]) ids[offsets[i]] = i;
}

}  // namespace

hipError_t lod_link(const uint32_t* map, uint32_t n_map, uint32_t offset, uint32_t* parent, const float4* rec, uint32_t n_rec, float4* bounds,
                    bool gauss, float sigma, hipStream_t st) {
    const uint32_t n = n_map > n_rec ? n_map : n_rec;
    if (!n) return hipSuccess;
    if (gauss) hipLaunchKernelGGL(k_lod_link_gauss, dim3((n + 255u) / 256u), dim3(256), 0, st, map, n_map, offset, parent, rec, n_rec, sigma, bounds);
    else hipLaunchKernelGGL(k_lod_link, dim3((n + 255u) / 256u), dim3(256), 0, st, map, n_map, offset, parent, rec, n_rec, bounds);
    return hipGetLastError();
}

namespace {

template <bool kVis>
hipError_t lod_sweep_levels(const LodLevelsK& t, const LodSelectK& k, uint8_t* open, uint32_t* flags, uint32_t* counts, const uint8_t* vis, hipStream_t st) {
    for (uint32_t l = t.levels; l-- > 0;) {
        const uint32_t f = (uint32_t)t.first[l], n = (uint32_t)(t.first[l + 1] - t.first[l]);
        if (!n) continue;
        const dim3 grid(std::min((n + 255u) / 256u, kLodGrid)), block(256);
        const bool top = l + 1 == t.levels, leaf = l == 0;
        uint32_t* const sel = counts + l;
        uint32_t* const ref = counts + kLodRefineWord;
        uint32_t* const pln = counts + kLodPlainWord;
        if (top && leaf) hipLaunchKernelGGL((k_lod_select<true, true, kVis>), grid, block, 0, st, t.bounds, t.parent, f, n, k, open, flags, sel, ref, vis, pln);
        else if (top) hipLaunchKernelGGL((k_lod_select<true, false, kVis>), grid, block, 0, st, t.bounds, t.parent, f, n, k, open, flags, sel, ref, vis, pln);
        else if (leaf) hipLaunchKernelGGL((k_lod_select<false, true, kVis>), grid, block, 0, st, t.bounds, t.parent, f, n, k, open, flags, sel, ref, vis, pln);
        else hipLaunchKernelGGL((k_lod_select<false, false, kVis>), grid, block, 0, st, t.bounds, t.parent, f, n, k, open, flags, sel, ref, vis, pln);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t lod_sweep(const LodLevelsK& t, const LodSelectK& k, uint8_t* open, uint32_t* flags, uint32_t* counts, const uint8_t* vis, hipStream_t st) {
    return vis ? lod_sweep_levels<true>(t, k, open, flags, counts, vis, st) : lod_sweep_levels<false>(t, k, open, flags, counts, nullptr, st);
}

hipError_t lod_node_ids(const uint32_t* flags, const uint32_t* offsets, uint32_t n, uint32_t* ids, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_lod_ids, dim3((n + 255u) / 256u), dim3(256), 0, st, flags, offsets, n, ids);
    return hipGetLastError();
}

hipError_t lod_scan(const uint32_t* flags, uint32_t* offsets, uint32_t n, void* temp, size_t temp_bytes, hipStream_t st) {
    return rocprim::exclusive_scan(temp, temp_bytes, flags, offsets, 0u, (size_t)n, rocprim::plus<uint32_t>(), st);
}

}  // namespace m2s
