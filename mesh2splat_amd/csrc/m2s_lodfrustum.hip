// m2s_lodfrustum.hip — the visibility plane behind m2s_lod_select_frustum and m2s_lod_select_budget_frustum (include/m2s.h): a node of
// the level-of-detail tree is visible iff at least one leaf below it passes the prepass's frustum test (m2s_viewmath.h, the one
// definition).  No counterpart in the reference.  The two cuts that read the plane are the kVis instances of k_lod_select (m2s_lod.hip)
// and k_lod_thresholds (m2s_lodbudget.hip).
//
//   k_lod_visible   one launch per level from the leaves up to the level below the last, on one stream, over a plane zeroed by a
//                   stream-ordered memset in front of them.  A leaf reads its bound (16 B) and its parent word (4 B), evaluates the
//                   test with the caller's guard band and, where it passes, writes its own byte and its parent's; a node above the
//                   leaves reads its own byte (1 B) and, where it is set, its parent word (4 B) and writes the parent's byte.  Every
//                   store writes the value 1 into a byte that is 0 or 1 and that nobody reads before the next launch: the plane does not
//                   depend on the order of the lanes.  Plain vector byte stores, not atomicOr on words: a byte store touches no
//                   neighbouring byte, so there is nothing to merge, and the children of one parent are neighbours, whose stores of one
//                   value to one address an atomic would only serialise.  The leaves that pass are counted in registers, then per wave,
//                   then per workgroup, and leave as one integer atomicAdd per workgroup.  Grid-stride over at most kLodVisGrid workgroups.
//                   The occluded leaf instance (kOcc, behind m2s_lod_select_occluded and m2s_lod_select_budget_occluded) reads, per
//                   leaf that passes the frustum test, one texel of a depth image (4 B, a gather) through the prepass's own depth
//                   test (m2s_viewmath.h, the one definition) and, only where the leaf lies behind it, the alpha of its node record
//                   (4 B at a 96 B stride): a leaf behind the image whose alpha is above .95 is not inside.  Its three counts (inside
//                   the frustum, occluded, behind but kept) go the way of the one above: registers, wave, workgroup, one atomicAdd each.
// No floating-point atomics.  Vector stores only.
#include <algorithm>

#include "../../include/m2s.h"
#include "m2s_device.h"
#include "m2s_viewmath.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr uint32_t kLodVisGrid = 1024;     // workgroups at most: four per CU, as the sweep

// What the leaf test takes beside the bounds: the frustum alone, or the frustum and the occluder behind it.  The plain form IS
// LodFrustumK, so that the instances without an occluder keep their kernel arguments byte for byte.
template <bool kOcc> struct LodVisArgs : LodFrustumK {};
template <> struct LodVisArgs<true> : LodFrustumK { LodOccluderK occ; };

// nodes [first, first + n) of one level.  A node of the last level has M2S_LOD_NO_PARENT and marks nobody.
// kOcc (leaves only): inside_word then points at three words: leaves inside the frustum, of those occluded, of those behind the image and kept.
template <bool kLeaf, bool kOcc = false>
__global__ void __launch_bounds__(256) k_lod_visible(const float4* __restrict__ bounds, const uint32_t* __restrict__ parent, uint32_t first, uint32_t n,
                                                     LodVisArgs<kOcc> f, uint8_t* __restrict__ vis, uint32_t* __restrict__ inside_word) {
    static_assert(kLeaf || !kOcc, "only leaves are tested against the depth image");
    uint32_t n_in = 0, n_occ = 0, n_kept = 0;
    const uint32_t stride = gridDim.x * 256u;
    for (unsigned long long t = blockIdx.x * 256u + threadIdx.x; t < n; t += stride) {       // (64 bits: t + stride may pass 2^32)
        const uint32_t i = first + (uint32_t)t;
        bool seen;
        if (kLeaf) {
            const float4 b = bounds[i];
            const float4 ws = m4_mul(f.M, b.x, b.y, b.z, 1.0f);
            const float4 vs = m4_mul(f.V, ws.x, ws.y, ws.z, 1.0f);
            const float4 c = m4_mul(f.P, vs.x, vs.y, vs.z, vs.w);
            seen = clip_inside(c, f.guard);
            n_in += seen ? 1u : 0u;
            if constexpr (kOcc) {
                if (seen && depth_behind(c, f.occ.depth, f.occ.depth_w, f.occ.depth_h, f.occ.bias)) {
                    const float alpha = f.occ.nodes[(size_t)i * 24u + 7u];           // color[3] of the leaf's node record
                    seen = !(alpha > .95f);                                          // (a NaN alpha keeps the leaf, as in the shader)
                    n_occ += seen ? 0u : 1u;
                    n_kept += seen ? 1u : 0u;
                }
            }
            if (seen) vis[i] = 1;
        } else {
            seen = vis[i] != 0;
        }
        if (seen) {
            const uint32_t p = parent[i];
            if (p != M2S_LOD_NO_PARENT) vis[p] = 1;
        }
    }
    if (kLeaf) {
        __shared__ uint32_t wave_in[4];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) n_in += (uint32_t)__shfl_xor((int)n_in, o);
        if ((threadIdx.x & 63u) == 0u) wave_in[threadIdx.x >> 6] = n_in;
        __syncthreads();
        if (threadIdx.x == 0u) {
            const uint32_t a = (wave_in[0] + wave_in[1]) + (wave_in[2] + wave_in[3]);
            if (a) atomicAdd(inside_word, a);
        }
        if constexpr (kOcc) {
            __shared__ uint32_t wave_occ[4], wave_kept[4];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                n_occ += (uint32_t)__shfl_xor((int)n_occ, o);
                n_kept += (uint32_t)__shfl_xor((int)n_kept, o);
            }
            if ((threadIdx.x & 63u) == 0u) { wave_occ[threadIdx.x >> 6] = n_occ; wave_kept[threadIdx.x >> 6] = n_kept; }
            __syncthreads();
            if (threadIdx.x == 0u) {
                const uint32_t a = (wave_occ[0] + wave_occ[1]) + (wave_occ[2] + wave_occ[3]);
                const uint32_t b = (wave_kept[0] + wave_kept[1]) + (wave_kept[2] + wave_kept[3]);
                if (a) atomicAdd(inside_word + 1, a);
                if (b) atomicAdd(inside_word + 2, b);
            }
        }
    }
}

}  // namespace

hipError_t lod_visibility(const LodLevelsK& t, const LodFrustumK& f, const LodOccluderK* occ, uint8_t* vis, uint32_t* inside_word, hipStream_t st) {
    hipError_t e = hipMemsetAsync(vis, 0, (size_t)t.first[t.levels], st);
    if (e != hipSuccess) return e;
    for (uint32_t l = 0; l < t.levels && (l == 0 || l + 1 < t.levels); ++l) {
        const uint32_t fl = (uint32_t)t.first[l], n = (uint32_t)(t.first[l + 1] - t.first[l]);
        if (!n) continue;
        const dim3 grid(std::min((n + 255u) / 256u, kLodVisGrid)), block(256);
        if (l == 0 && occ) {
            LodVisArgs<true> fo;
            static_cast<LodFrustumK&>(fo) = f;
            fo.occ = *occ;
            hipLaunchKernelGGL((k_lod_visible<true, true>), grid, block, 0, st, t.bounds, t.parent, fl, n, fo, vis, inside_word);
        } else {
            LodVisArgs<false> fp;
            static_cast<LodFrustumK&>(fp) = f;
            if (l == 0) hipLaunchKernelGGL((k_lod_visible<true, false>), grid, block, 0, st, t.bounds, t.parent, fl, n, fp, vis, inside_word);
            else hipLaunchKernelGGL((k_lod_visible<false, false>), grid, block, 0, st, t.bounds, t.parent, fl, n, fp, vis, inside_word);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace m2s
