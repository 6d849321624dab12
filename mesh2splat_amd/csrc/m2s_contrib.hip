// m2s_contrib.hip — the contribution pass and the compaction behind it (include/m2s.h: m2s_contrib_accumulate, m2s_prune).  No
// counterpart in the reference, which shows every Gaussian it keeps.
//
//   k_splat_contrib   a lean sibling of k_splat_blend (m2s_splat.hip) over the SAME records, pairs, ranges and tile order — the host
//                     runs the splat pass's own setup / bin / grouping stages first —: one 256-lane workgroup per 16 x 16 tile, one
//                     lane per pixel, the tile's quads staged through LDS in batches of 256 with the same per-tile edge thresholds
//                     (stage_triangle).  A lane carries ONE destination value, the albedo attachment's alpha A3, instead of seventeen,
//                     and records per fragment the weight w = sA3 * tA of the pinned update A3 <- unorm8(sA3 * tA + A3).
//                     Reduction: lanes -> the staged quad's two LDS words (integer max of the bits of w, integer sum of the fragments
//                     with w > count_weight), through a wave-level reduction when many lanes of the wave contribute; after the batch
//                     the staging thread sends at most one atomicMax and one atomicAdd per (tile, quad) pair to the record the quad
//                     was made from, and none for a zero.  Integer atomics only: the result does not depend on the order.
//   Early exit        unconditional here (k_splat_blend needs `tame` sources): once A3 == 1.0 — 255 / 255, exactly representable —
//                     tA = 1 - 1 = 0, sA3 = clamp01(x) lies in [0, 1] for EVERY x (fmin / fmax drop a NaN, so clamp01(NaN) = 0) and
//                     w = sA3 * 0 = +0 exactly, whatever the quad; unorm8(0 + 1) = 1 keeps A3 there.  A saturated lane therefore skips
//                     every later quad, and a workgroup whose lanes are all saturated (or outside the viewport) leaves its list.
//   k_prune_flags / rocPRIM exclusive scan / k_prune_compact: the stable compaction of m2s_prune, 16 bytes per lane.
#include <rocprim/device/device_scan.hpp>

#include "m2s_devfn.h"
#include "m2s_quadraster.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr int kTile = kSplatTile;
constexpr int kBatch = 256;
constexpr uint32_t kFlagTri0 = kQuadTri0, kFlagTri1 = kQuadTri1;
constexpr int kWaveShift = 8;              // as k_splat_blend: bits 8..11 = the waves of the tile whose rows the quad's box reaches
constexpr int kRecF4 = 8;                  // the 128-byte record of k_splat_setup
constexpr int kDirectLanes = 6;            // up to this many contributing lanes of a wave send their own LDS atomics

struct __align__(16) StagedContrib {
    int4 e0, e1, e2, e3;   // as StagedQuad (m2s_splat.hip)
    int4 e4;               // T[2] of tri 0, T[2] of tri 1, flags (this tile), bits of the opacity
    float4 f;              // record word [3]: screen.x, screen.y, -0.5 conic.x, -0.5 conic.z
    float cy;              // record word [4].x: -conic.y
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float unorm8(float r) {   // == m2s_splat.hip
    const float q = rintf(clamp01(r) * 255.0f);
    return (float)((double)q * (1.0 / 255.0));
}

__global__ void __launch_bounds__(256) k_splat_contrib(const float4* __restrict__ rec, const uint32_t* __restrict__ vals,
                                                       const uint2* __restrict__ ranges, const uint32_t* __restrict__ order, int W, int H,
                                                       int tiles_x, const uint32_t* __restrict__ sources, float count_weight,
                                                       uint32_t* __restrict__ g_wmax, uint32_t* __restrict__ g_npix) {
    __shared__ StagedContrib sq[kBatch];
    __shared__ uint32_t acc_w[kBatch], acc_n[kBatch];
    const int tid = threadIdx.x;
    const uint32_t tile = order[blockIdx.x];
    const int px0 = (int)(tile % (uint32_t)tiles_x) * kTile, py0 = (int)(tile / (uint32_t)tiles_x) * kTile;
    const int lx = tid & (kTile - 1), ly = tid / kTile;
    const int x = px0 + lx, y = py0 + ly;
    const bool in_view = x < W && y < H;
    const uint32_t wave_bit = 1u << (kWaveShift + tid / 64);
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
    const uint2 rg = ranges[tile];
    const uint32_t begin = rg.x, end = rg.y;

    float A3 = 0.0f;
    for (uint32_t base = begin; base < end; base += kBatch) {
        const uint32_t m = min((uint32_t)kBatch, end - base);
        uint32_t record = 0;
        // (thread t alone writes slot t between the barriers below, and it flushed the slot's previous contents itself)
        if ((uint32_t)tid < m) {
            const uint32_t qi = vals[base + tid];
            record = sources[qi];
            const float4* r = rec + (size_t)kRecF4 * qi;
            const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
            const int X[4] = { __float_as_int(r0.x), __float_as_int(r0.y), __float_as_int(r0.z), __float_as_int(r0.w) };
            const int Y[4] = { __float_as_int(r1.x), __float_as_int(r1.y), __float_as_int(r1.z), __float_as_int(r1.w) };
            const uint32_t qf = __float_as_uint(r2.x);
            uint32_t fl = 0;
            StagedContrib s;
            s.e0 = s.e1 = s.e2 = s.e3 = make_int4(0, 0, 0, kTMax);
            int t20 = kTMax, t21 = kTMax;
            const int X0[3] = { X[0], X[1], X[2] }, Y0[3] = { Y[0], Y[1], Y[2] };
            const int X1[3] = { X[0], X[2], X[3] }, Y1[3] = { Y[0], Y[2], Y[3] };
            uint32_t waves = 0;
            if ((qf & kFlagTri0) && box_meets_tile(X0, Y0, W, H, px0, py0, &waves)) { stage_triangle(X0, Y0, px0, py0, s.e0, s.e1, t20); fl |= kFlagTri0; }
            if ((qf & kFlagTri1) && box_meets_tile(X1, Y1, W, H, px0, py0, &waves)) { stage_triangle(X1, Y1, px0, py0, s.e2, s.e3, t21); fl |= kFlagTri1; }
            fl |= waves << kWaveShift;
            s.e4 = make_int4(t20, t21, (int)fl, __float_as_int(r4.z));
            s.f = r3;
            s.cy = r4.x;
            sq[tid] = s;
            acc_w[tid] = 0;
            acc_n[tid] = 0;
        }
        // the early exit of the header: nothing behind a saturated pixel has a weight other than +0
        if (__syncthreads_and(!in_view || A3 == 1.0f)) break;          // (also the barrier behind the staging)
        for (uint32_t e = 0; e < m; ++e) {
            const int4 e4 = sq[e].e4;
            const uint32_t fl = (uint32_t)e4.z;
            if (!(fl & wave_bit)) continue;                             // (wave-uniform)
            int cov = 0;
            if (in_view && A3 != 1.0f) {
                if (fl & kFlagTri0) {
                    const int4 a = sq[e].e0, b = sq[e].e1;
                    cov += (a.x * lx + b.x * ly > a.w) & (a.y * lx + b.y * ly > b.w) & (a.z * lx + b.z * ly > e4.x);
                }
                if (fl & kFlagTri1) {
                    const int4 a = sq[e].e2, b = sq[e].e3;
                    cov += (a.x * lx + b.x * ly > a.w) & (a.y * lx + b.y * ly > b.w) & (a.z * lx + b.z * ly > e4.y);
                }
            }
            if (!__any(cov)) continue;                                  // (wave-uniform)
            uint32_t wbits = 0, cnt = 0;
            if (cov) {
                const float4 f3 = sq[e].f;
                const float dx = f3.x - fx, dy = f3.y - fy;
                const float alpha = (f3.z * (dx * dx) + f3.w * (dy * dy)) + sq[e].cy * (dx * dy);
                const float g = __expf(alpha);
                const float sA3 = clamp01(__int_as_float(e4.w) * g);
                for (int k = 0; k < cov; ++k) {
                    const float tA = 1.0f - A3;
                    const float w = sA3 * tA;                           // the weight: the product of the pinned update itself
                    wbits = max(wbits, __float_as_uint(w));             // (0 <= w <= 1: the bits order as the values)
                    cnt += w > count_weight ? 1u : 0u;
                    A3 = unorm8(w + A3);
                }
                if (wbits == 0x80000000u) wbits = 0;                    // (cannot happen — both factors are >= +0 —; kept out of the maximum anyway)
            }
            const unsigned long long nz = __ballot(wbits != 0u);
            if (!nz) continue;
            if (__popcll(nz) <= kDirectLanes) {
                if (wbits) {
                    atomicMax(&acc_w[e], wbits);
                    if (cnt) atomicAdd(&acc_n[e], cnt);
                }
            } else {
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    wbits = max(wbits, (uint32_t)__shfl_xor((int)wbits, o));
                    cnt += (uint32_t)__shfl_xor((int)cnt, o);
                }
                if ((tid & 63) == 0) {
                    atomicMax(&acc_w[e], wbits);
                    if (cnt) atomicAdd(&acc_n[e], cnt);
                }
            }
        }
        __syncthreads();                                                // every lane's contribution to this batch has arrived
        if ((uint32_t)tid < m) {
            const uint32_t w = acc_w[tid], n = acc_n[tid];
            if (w) atomicMax(&g_wmax[record], w);
            if (n) atomicAdd(&g_npix[record], n);
        }
    }
}

// ---- compaction ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_prune_flags(const uint32_t* __restrict__ wmax, const uint32_t* __restrict__ npix, uint32_t n,
                                                     float min_weight, uint32_t min_pixels, uint32_t* __restrict__ flags,
                                                     unsigned long long* __restrict__ counters) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool by_w = false, by_p = false;
    if (i < n) {
        by_w = !(__uint_as_float(wmax[i]) > min_weight);
        by_p = !by_w && npix[i] < min_pixels;
        flags[i] = (by_w || by_p) ? 0u : 1u;
    }
    const unsigned long long bw = __ballot(by_w), bp = __ballot(by_p);
    if ((threadIdx.x & 63) == 0) {
        if (bw) atomicAdd(&counters[0], (unsigned long long)__popcll(bw));
        if (bp) atomicAdd(&counters[1], (unsigned long long)__popcll(bp));
    }
}

// one lane per 16 bytes: lane t moves float4 (t % f4_per_row) of row (t / f4_per_row)
__global__ void __launch_bounds__(256) k_prune_compact(const float4* __restrict__ src, const uint32_t* __restrict__ flags,
                                                       const uint32_t* __restrict__ offsets, unsigned long long n_f4, uint32_t f4_per_row,
                                                       float4* __restrict__ dst) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (t >= n_f4) return;
    const uint32_t row = (uint32_t)(t / f4_per_row), j = (uint32_t)(t - (unsigned long long)row * f4_per_row);
    if (flags[row]) dst[(size_t)offsets[row] * f4_per_row + j] = src[t];
}

}  // namespace

hipError_t contrib_blend(const float4* rec, const uint32_t* vals, const uint2* ranges, const uint32_t* order, int W, int H,
                         const uint32_t* sources, float count_weight, uint32_t* wmax, uint32_t* npix, hipStream_t st) {
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_splat_contrib, dim3((uint32_t)(tiles_x * tiles_y)), dim3(256), 0, st, rec, vals, ranges, order, W, H, tiles_x, sources,
                       count_weight, wmax, npix);
    return hipGetLastError();
}

size_t prune_scan_temp_bytes(uint32_t n) {
    size_t b = 0;
    (void)rocprim::exclusive_scan(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(), (hipStream_t)0);
    return b;
}

hipError_t prune_flags_scan(const uint32_t* wmax, const uint32_t* npix, uint32_t n, float min_weight, uint32_t min_pixels, uint32_t* flags,
                            uint32_t* offsets, unsigned long long* counters, void* temp, size_t temp_bytes, hipStream_t st) {
    hipLaunchKernelGGL(k_prune_flags, dim3((n + 255u) / 256u), dim3(256), 0, st, wmax, npix, n, min_weight, min_pixels, flags, counters);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return rocprim::exclusive_scan(temp, temp_bytes, (const uint32_t*)flags, offsets, 0u, (size_t)n, rocprim::plus<uint32_t>(), st);
}

hipError_t prune_compact(const float4* src, const uint32_t* flags, const uint32_t* offsets, uint32_t n, uint32_t f4_per_row, float4* dst,
                         hipStream_t st) {
    const unsigned long long n_f4 = (unsigned long long)n * f4_per_row;
    if (!n_f4) return hipSuccess;
    hipLaunchKernelGGL(k_prune_compact, dim3((uint32_t)((n_f4 + 255ull) / 256ull)), dim3(256), 0, st, src, flags, offsets, n_f4, f4_per_row, dst);
    return hipGetLastError();
}

}  // namespace m2s
