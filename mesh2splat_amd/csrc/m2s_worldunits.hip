// m2s_worldunits.hip — the kernels behind m2s_records_to_world_units (include/m2s.h): scale[0..2] of every record divided by its
// resolutionTarget, so that the records carry what the viewer draws (m2s_covmath.h: std / R times the stored scale) and the merge pass
// and the level-of-detail cut, which read scale[0..1] as world lengths, see conversions as they see every other record.  No counterpart
// in the reference, which keeps R beside its records for as long as they live.
//
//   k_world_units_copy     out of place (records adopted through m2s_set_records, uploaded ones, a second lane's: the pool gets them),
//                          built as k_prune_compact: one lane per 16-byte word, consecutive lanes on consecutive words, so a wave reads
//                          and writes 1 KiB in one instruction each way.  Word 2 of every record is divided on its way, the other five
//                          pass with their bits.  96 B in, 96 B out per record.
//   k_world_units_inplace  the records live in the pool already: one lane per record, only its scale word is loaded and stored — 16 of
//                          its 96 bytes each way.  A wave touches 64 words 96 B apart, i.e. a 16-byte piece of every 128-byte line or
//                          so; the fabric moves whole 64-byte requests, so the traffic is nearer 2 x 64 B per record than 2 x 16 B, still
//                          under the 2 x 96 B of moving everything (k_refit_apply has the same shape and runs at 0.6 - 0.7 ms on 2.74 M).
// Both are grid-stride over at most kWorldUnitsGrid workgroups: no LDS, no atomics, nothing read twice.  The quotient is the compiler's
// IEEE expansion of `/` (no fast-math, denormals kept): m2s_exact.h's div_rn is proven for |a|, b in [2^-60, 2^60] only, and this pass
// must be right for zeros, infinities, NaN and subnormal quotients too, on a path where the division hides behind the memory traffic.
#include <algorithm>

#include "m2s_device.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr uint32_t kWorldUnitsGrid = 2048;     // workgroups at most: eight per CU

__device__ __forceinline__ float4 world_units_scale(float4 s, float Rf) {
    s.x = s.x / Rf;
    s.y = s.y / Rf;
    s.z = s.z / Rf;
    return s;                                   // (s.w: the bits it was read with)
}

__global__ void __launch_bounds__(256) k_world_units_copy(const float4* __restrict__ src, unsigned long long n_f4, float Rf,
                                                          float4* __restrict__ dst) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; t < n_f4; t += stride) {
        float4 v = src[t];
        if (t % 6ull == 2ull) v = world_units_scale(v, Rf);
        dst[t] = v;
    }
}

__global__ void __launch_bounds__(256) k_world_units_inplace(float4* __restrict__ records, uint32_t n, float Rf) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) {     // (64 bits: i + stride may pass 2^32)
        float4* slot = records + 6ull * i + 2;                          // scale[4] of the 96-byte record
        *slot = world_units_scale(*slot, Rf);
    }
}

}  // namespace

hipError_t world_units(const float4* src, float4* dst, uint32_t n, uint32_t R, hipStream_t st) {
    if (!n) return hipSuccess;
    const float Rf = (float)R;
    if (src == dst) {
        const uint32_t grid = (uint32_t)std::min<unsigned long long>(((unsigned long long)n + 255ull) / 256ull, kWorldUnitsGrid);
        hipLaunchKernelGGL(k_world_units_inplace, dim3(grid), dim3(256), 0, st, dst, n, Rf);
    } else {
        const unsigned long long n_f4 = 6ull * n;
        const uint32_t grid = (uint32_t)std::min<unsigned long long>((n_f4 + 255ull) / 256ull, kWorldUnitsGrid);
        hipLaunchKernelGGL(k_world_units_copy, dim3(grid), dim3(256), 0, st, src, n_f4, Rf, dst);
    }
    return hipGetLastError();
}

}  // namespace m2s
