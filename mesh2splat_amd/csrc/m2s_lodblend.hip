// m2s_lodblend.hip — the kernels behind m2s_lod_blend (include/m2s.h): every record of a cut is rewritten as "its node at weight 1 - t,
// its node's parent at weight t", out of the TREE into the context's pool.  No counterpart in the reference.
//
//   k_lod_blend_t    one lane per record of the cut: ids[j] (4 B), the parent word (4 B, a gather in node order: the cut's output is
//                    sorted by node index, so neighbours read neighbours), the node's bound and — where it has a parent — the parent's
//                    (16 B each); writes t[j] (4 B).  44 B per record.  The records with t > 0 and with t == 1 are counted in registers,
//                    then per wave, then per workgroup, and leave as at most one integer atomicAdd per word per workgroup
//                    (k_lod_select's scheme).
//   k_lod_blend      the gather-blend of the 96-byte records, k_prune_compact's shape: one lane per 16-byte word, consecutive lanes on
//                    consecutive words, so a wave stores 1 KiB without a gap and reads whole 96-byte records.  A lane reads t[j] and
//                    ids[j] (8 B, shared by the six lanes of a record), its word of the node (16 B) and, ONLY where t > 0, the parent
//                    word (4 B) and its word of the parent (16 B).  The scale lane and the rotation lane both read the two rotation words
//                    and evaluate the frame rule (pin 5) on their own, so that they agree on k without talking: the scale lane pays 32 B
//                    more.  At t == 0 the lane copies.  Per record: 96 B written, 104 B read at t == 0, 232 B at t > 0.  The records
//                    with t > 0 and k != 0 are counted by the rotation lane, the same way as above.
//   k_lod_blend_sh   one lane per (record, float4 column) of the SH plane, as k_merge_reduce_sh: 192 B written per record, 192 B read at
//                    t == 0, 384 B at t > 0.
// All three: grid-stride over at most kBlendGrid workgroups, 64-bit lane indices, no LDS beyond the count reduction, vector stores only.
// fp32, one rounding per operation, the compiler's IEEE division.
#include <algorithm>

#include "../../include/m2s.h"
#include "m2s_device.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr uint32_t kBlendGrid = 2048;       // workgroups at most: eight per CU
constexpr float kC = 0.70710678118654752f;

// pin 2: (s * s) / d2 of one bound
__device__ __forceinline__ float blend_q(const float4 b, const LodBlendK& k) {
    const float dx = b.x - k.cx, dy = b.y - k.cy, dz = b.z - k.cz;
    const float d2 = fmaxf((dx * dx + dy * dy) + dz * dz, k.near2);
    const float s = b.w * k.focal;
    return (s * s) / d2;
}

__device__ __forceinline__ float lerp1(float u, float t, float a, float b) { return u * a + t * b; }

// the sum of n over the workgroup's four waves, added to *word by one lane (nothing for a sum of 0); `part`: four words of LDS
__device__ __forceinline__ void blend_count(uint32_t n, uint32_t* part, uint32_t* __restrict__ word) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t a = (part[0] + part[1]) + (part[2] + part[3]);
        if (a) atomicAdd(word, a);
    }
}

__global__ void __launch_bounds__(256) k_lod_blend_t(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ parent,
                                                     const float4* __restrict__ bounds, uint32_t n, LodBlendK k, float* __restrict__ t,
                                                     uint32_t* __restrict__ counts) {
    __shared__ uint32_t part_blend[4], part_sat[4];
    uint32_t n_blend = 0, n_sat = 0;
    const uint32_t stride = gridDim.x * 256u;
    for (unsigned long long j = blockIdx.x * 256u + threadIdx.x; j < n; j += stride) {      // (64 bits: j + stride may pass 2^32)
        const uint32_t i = ids[j], p = parent[i];
        float tv = 0.0f;
        if (p != M2S_LOD_NO_PARENT) {
            const float qi = blend_q(bounds[i], k), qp = blend_q(bounds[p], k);
            const float den = qp - qi, num = k.tau2 - qi;
            const float t_raw = num / den;
            tv = fminf(fmaxf((t_raw - (1.0f - k.band)) / k.band, 0.0f), 1.0f);
            if (!(den > 0.0f) || !(tv > 0.0f)) tv = 0.0f;      // (the second test: a zero is +0, whichever zero fmaxf returned)
        }
        t[j] = tv;
        n_blend += tv > 0.0f ? 1u : 0u;
        n_sat += tv == 1.0f ? 1u : 0u;
    }
    blend_count(n_blend, part_blend, counts + kLodBlendBlended);
    blend_count(n_sat, part_sat, counts + kLodBlendSaturated);
}

// Pin 5.  c, r: the stored rotation words (w, x, y, z) = (.x, .y, .z, .w) of the child and of the parent.  -> k; *cand = the parent's
// frame turned to the child's, kC and the sign applied.
__device__ __forceinline__ uint32_t blend_frame(const float4 c, const float4 r, float4* cand) {
    const float W = r.x, X = r.y, Y = r.z, Z = r.w;
    const float wmz = W - Z, wpz = W + Z, xpy = X + Y, xmy = X - Y, ymx = Y - X, zmw = Z - W;
    const bool unit = fabsf(((W * W + X * X) + (Y * Y + Z * Z)) - 1.0f) <= 0x1p-10f;
    float4 best = r;
    float best_d = (c.x * r.x + c.y * r.y) + (c.z * r.z + c.w * r.w);
    float best_score = best_d * best_d;
    uint32_t best_k = 0;
#define M2S_CAND(K, A, B, C, D)                                                     \
    {                                                                               \
        const float d = (c.x * (A) + c.y * (B)) + (c.z * (C) + c.w * (D));          \
        const float score = ((K) & 1) ? (d * d) * 0.5f : d * d;                     \
        if (unit && score > best_score) {                                           \
            best_score = score; best_d = d; best_k = (K);                           \
            best = ((K) & 1) ? make_float4((A) * kC, (B) * kC, (C) * kC, (D) * kC) : make_float4((A), (B), (C), (D)); \
        }                                                                           \
    }
    M2S_CAND(1, wmz, xpy, ymx, wpz)
    M2S_CAND(2, -Z, Y, -X, W)
    M2S_CAND(3, wpz, xmy, xpy, zmw)
    M2S_CAND(4, -X, W, Z, -Y)
    M2S_CAND(5, -xpy, wmz, wpz, xmy)
    M2S_CAND(6, -Y, -Z, W, X)
    M2S_CAND(7, ymx, wpz, zmw, -xpy)
#undef M2S_CAND
    if (best_d < 0.0f) best = make_float4(-best.x, -best.y, -best.z, -best.w);
    *cand = best;
    return best_k;
}

__global__ void __launch_bounds__(256) k_lod_blend(const float4* __restrict__ nodes, const uint32_t* __restrict__ ids,
                                                   const uint32_t* __restrict__ parent, const float* __restrict__ t,
                                                   unsigned long long n_f4, float4* __restrict__ out, uint32_t* __restrict__ counts) {
    __shared__ uint32_t part_turn[4];
    uint32_t n_turn = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long g = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; g < n_f4; g += stride) {
        const uint32_t j = (uint32_t)(g / 6ull), w = (uint32_t)(g - (unsigned long long)j * 6ull);
        const float tv = t[j];
        const uint32_t i = ids[j];
        const float4 a = nodes[(size_t)6 * i + w];
        float4 o = a;
        if (tv != 0.0f) {                                                  // (t > 0: the weights hold no NaN and no negative value)
            const uint32_t p = parent[i];
            const float4 b = nodes[(size_t)6 * p + w];
            const float u = 1.0f - tv;
            if (w == 1u) {                                                 // colour and alpha
                o = make_float4(lerp1(u, tv, a.x, b.x), lerp1(u, tv, a.y, b.y), lerp1(u, tv, a.z, b.z), lerp1(u, tv, a.w, b.w));
            } else if (w == 0u || w == 3u) {                               // position, normal: the fourth word is the child's
                o = make_float4(lerp1(u, tv, a.x, b.x), lerp1(u, tv, a.y, b.y), lerp1(u, tv, a.z, b.z), a.w);
            } else if (w == 5u) {                                          // pbr[0..1]
                o = make_float4(lerp1(u, tv, a.x, b.x), lerp1(u, tv, a.y, b.y), a.z, a.w);
            } else {                                                       // scale (w == 2) and rotation (w == 4): one frame rule
                const float4 c = w == 4u ? a : nodes[(size_t)6 * i + 4];
                const float4 r = w == 4u ? b : nodes[(size_t)6 * p + 4];
                float4 cand;
                const uint32_t k = blend_frame(c, r, &cand);
                if (w == 4u) {
                    o = make_float4(lerp1(u, tv, a.x, cand.x), lerp1(u, tv, a.y, cand.y), lerp1(u, tv, a.z, cand.z), lerp1(u, tv, a.w, cand.w));
                    n_turn += k != 0u ? 1u : 0u;
                } else {
                    const bool swap = (k & 1u) != 0u;
                    o = make_float4(lerp1(u, tv, a.x, swap ? b.y : b.x), lerp1(u, tv, a.y, swap ? b.x : b.y), lerp1(u, tv, a.z, b.z), a.w);
                }
            }
        }
        out[g] = o;
    }
    blend_count(n_turn, part_turn, counts + kLodBlendTurned);
}

__global__ void __launch_bounds__(256) k_lod_blend_sh(const float4* __restrict__ sh, const uint32_t* __restrict__ ids,
                                                      const uint32_t* __restrict__ parent, const float* __restrict__ t,
                                                      unsigned long long n_f4, float4* __restrict__ out) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long g = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; g < n_f4; g += stride) {
        const uint32_t j = (uint32_t)(g / kMergeShLanes), q = (uint32_t)(g - (unsigned long long)j * kMergeShLanes);
        const float tv = t[j];
        const uint32_t i = ids[j];
        float4 o = sh[(size_t)kMergeShLanes * i + q];
        if (tv != 0.0f) {
            const float4 b = sh[(size_t)kMergeShLanes * parent[i] + q];
            const float u = 1.0f - tv;
            o = make_float4(lerp1(u, tv, o.x, b.x), lerp1(u, tv, o.y, b.y), lerp1(u, tv, o.z, b.z), lerp1(u, tv, o.w, b.w));
        }
        out[g] = o;
    }
}

dim3 blend_grid(unsigned long long lanes) { return dim3((uint32_t)std::min<unsigned long long>((lanes + 255ull) / 256ull, kBlendGrid)); }

}  // namespace

hipError_t lod_blend_weights(const uint32_t* ids, const uint32_t* parent, const float4* bounds, uint32_t n, const LodBlendK& k, float* t,
                             uint32_t* counts, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_lod_blend_t, blend_grid(n), dim3(256), 0, st, ids, parent, bounds, n, k, t, counts);
    return hipGetLastError();
}

hipError_t lod_blend_records(const float4* nodes, const uint32_t* ids, const uint32_t* parent, const float* t, uint32_t n, float4* out,
                             uint32_t* counts, hipStream_t st) {
    if (!n) return hipSuccess;
    const unsigned long long n_f4 = (unsigned long long)n * 6ull;
    hipLaunchKernelGGL(k_lod_blend, blend_grid(n_f4), dim3(256), 0, st, nodes, ids, parent, t, n_f4, out, counts);
    return hipGetLastError();
}

hipError_t lod_blend_sh(const float4* sh, const uint32_t* ids, const uint32_t* parent, const float* t, uint32_t n, float4* out, hipStream_t st) {
    if (!n) return hipSuccess;
    const unsigned long long n_f4 = (unsigned long long)n * kMergeShLanes;
    hipLaunchKernelGGL(k_lod_blend_sh, blend_grid(n_f4), dim3(256), 0, st, sh, ids, parent, t, n_f4, out);
    return hipGetLastError();
}

}  // namespace m2s
