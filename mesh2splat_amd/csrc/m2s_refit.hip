// m2s_refit.hip — the colour refit (include/m2s.h: m2s_refit_accumulate, m2s_refit_apply).  No counterpart in the reference, whose
// Gaussians keep the one texture sample the conversion gave them.
//
//   k_splat_refit     a sibling of k_splat_contrib (m2s_contrib.hip) over the SAME records, pairs, ranges and tile order — the host runs
//                     the splat pass's own setup / bin / grouping stages first —: one 256-lane workgroup per 16 x 16 tile, one lane per
//                     pixel, the tile's quads staged through LDS in batches of 256 (stage_triangle / box_meets_tile).  A lane reads its
//                     pixel's two uchar4 once and keeps its three errors eq_k, its participation bit and the albedo alpha A3; a lane
//                     that does not take part is treated as outside the viewport (its A3 matters to no other pixel).  Per fragment the
//                     weight w = sA3 * tA of the pinned update becomes wq = rint(w * 65536); eq_k is the lane's own, so a lane's share
//                     of a quad is (sum of its wq) and that sum times eq_k (<= 2^17 and 2^29: 32-bit products).
//                     Reduction: lanes -> the staged quad's four 64-bit LDS words, by LDS atomics of the few lanes that contribute or
//                     through a wave reduction first when many do; after the batch the staging thread sends at most four 64-bit
//                     integer atomics per (tile, quad) pair to the record the quad was made from, and none for a zero den.  Integer
//                     atomics only: the result does not depend on the order.
//   Early exit        that of k_splat_contrib: once A3 == 1.0 every later w is +0 and wq = 0, so a saturated lane skips every later
//                     quad and a workgroup whose lanes are all saturated (or take no part) leaves its list.
//   k_refit_apply     one lane per record: 32 bytes of accumulators in, 16 bytes of colour out, the update in fp64.
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
constexpr int kDirectLanes = 4;            // up to this many contributing lanes of a wave send their own LDS atomics (four each)
constexpr int kEqOne = 4096;               // an error of 1.0

struct __align__(16) StagedRefit {         // == StagedContrib (m2s_contrib.hip)
    int4 e0, e1, e2, e3;
    int4 e4;               // T[2] of tri 0, T[2] of tri 1, flags (this tile), bits of the opacity
    float4 f;              // record word [3]: screen.x, screen.y, -0.5 conic.x, -0.5 conic.z
    float cy;              // record word [4].x: -conic.y
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float unorm8(float r) {   // == m2s_splat.hip
    const float q = rintf(clamp01(r) * 255.0f);
    return (float)((double)q * (1.0 / 255.0));
}

// eq = floor((2 n + d) / (2 d)) clamped to +-4096, n = 4096 (m sa - 255 s), d = 255 sa: m / 255 - s / sa rounded to 1 / 4096 (sa >= 1)
__device__ __forceinline__ int refit_error(int m, int s, int sa) {
    const int n = kEqOne * (m * sa - 255 * s), d = 255 * sa;
    const int a = 2 * n + d, b = 2 * d;
    int q = a / b;
    if (a % b < 0) --q;                               // (C division truncates; b > 0)
    return min(max(q, -kEqOne), kEqOne);
}

__global__ void __launch_bounds__(256) k_splat_refit(const float4* __restrict__ rec, const uint32_t* __restrict__ vals,
                                                     const uint2* __restrict__ ranges, const uint32_t* __restrict__ order, int W, int H,
                                                     int tiles_x, const uint32_t* __restrict__ sources, const uint32_t* __restrict__ target,
                                                     const uint32_t* __restrict__ render, uint32_t min_cover,
                                                     unsigned long long* __restrict__ g_num, unsigned long long* __restrict__ g_den,
                                                     unsigned long long* __restrict__ g_pixels) {
    __shared__ StagedRefit sq[kBatch];
    __shared__ unsigned long long acc[kBatch][4];     // num[0..2] (two's complement), den
    const int tid = threadIdx.x;
    const uint32_t tile = order ? order[blockIdx.x] : blockIdx.x;
    const int px0 = (int)(tile % (uint32_t)tiles_x) * kTile, py0 = (int)(tile / (uint32_t)tiles_x) * kTile;
    const int lx = tid & (kTile - 1), ly = tid / kTile;
    const int x = px0 + lx, y = py0 + ly;
    const uint32_t wave_bit = 1u << (kWaveShift + tid / 64);
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;
    uint32_t begin = 0, end = 0;
    if (ranges) { const uint2 rg = ranges[tile]; begin = rg.x; end = rg.y; }

    // the lane's pixel: does it take part, and its error per channel
    bool active = false;
    int eq0 = 0, eq1 = 0, eq2 = 0;
    if (x < W && y < H) {
        const size_t p = (size_t)y * (size_t)W + (size_t)x;
        const uint32_t t = target[p], r = render[p];
        const int sa = (int)(r >> 24);
        active = (t >> 24) != 0u && (uint32_t)sa >= min_cover;                 // (min_cover >= 1: sa >= 1)
        if (active) {
            eq0 = refit_error((int)(t & 255u), (int)(r & 255u), sa);
            eq1 = refit_error((int)((t >> 8) & 255u), (int)((r >> 8) & 255u), sa);
            eq2 = refit_error((int)((t >> 16) & 255u), (int)((r >> 16) & 255u), sa);
        }
    }
    {
        const unsigned long long pb = __ballot(active);
        if ((tid & 63) == 0 && pb) atomicAdd(g_pixels, (unsigned long long)__popcll(pb));
    }

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
            StagedRefit s;
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
            acc[tid][0] = 0; acc[tid][1] = 0; acc[tid][2] = 0; acc[tid][3] = 0;
        }
        // the early exit of the header: nothing behind a saturated pixel has a weight other than +0
        if (__syncthreads_and(!active || A3 == 1.0f)) break;           // (also the barrier behind the staging)
        for (uint32_t e = 0; e < m; ++e) {
            const int4 e4 = sq[e].e4;
            const uint32_t fl = (uint32_t)e4.z;
            if (!(fl & wave_bit)) continue;                             // (wave-uniform)
            int cov = 0;
            if (active && A3 != 1.0f) {
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
            uint32_t dw = 0;                                            // the lane's wq over its (one or two) fragments: <= 2^17
            if (cov) {
                const float4 f3 = sq[e].f;
                const float dx = f3.x - fx, dy = f3.y - fy;
                const float alpha = (f3.z * (dx * dx) + f3.w * (dy * dy)) + sq[e].cy * (dx * dy);
                const float g = __expf(alpha);
                const float sA3 = clamp01(__int_as_float(e4.w) * g);
                for (int k = 0; k < cov; ++k) {
                    const float tA = 1.0f - A3;
                    const float w = sA3 * tA;                           // the weight of k_splat_contrib: 0 <= w <= 1, never NaN
                    dw += (uint32_t)rintf(w * 65536.0f);
                    A3 = unorm8(w + A3);
                }
            }
            const unsigned long long nz = __ballot(dw != 0u);
            if (!nz) continue;
            // the lane's products: |dw * eq| <= 2^17 * 2^12
            long long n0 = (long long)((int)dw * eq0), n1 = (long long)((int)dw * eq1), n2 = (long long)((int)dw * eq2);
            if (__popcll(nz) <= kDirectLanes) {
                if (dw) {
                    atomicAdd(&acc[e][3], (unsigned long long)dw);
                    if (n0) atomicAdd(&acc[e][0], (unsigned long long)n0);
                    if (n1) atomicAdd(&acc[e][1], (unsigned long long)n1);
                    if (n2) atomicAdd(&acc[e][2], (unsigned long long)n2);
                }
            } else {
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {                     // (64 lanes: den <= 2^23 in 32 bits, a num up to 2^35 in 64)
                    dw += (uint32_t)__shfl_xor((int)dw, o);
                    n0 += __shfl_xor(n0, o);
                    n1 += __shfl_xor(n1, o);
                    n2 += __shfl_xor(n2, o);
                }
                if ((tid & 63) == 0) {
                    atomicAdd(&acc[e][3], (unsigned long long)dw);
                    if (n0) atomicAdd(&acc[e][0], (unsigned long long)n0);
                    if (n1) atomicAdd(&acc[e][1], (unsigned long long)n1);
                    if (n2) atomicAdd(&acc[e][2], (unsigned long long)n2);
                }
            }
        }
        __syncthreads();                                                // every lane's contribution to this batch has arrived
        if ((uint32_t)tid < m) {
            const unsigned long long d = acc[tid][3];
            if (d) {                                                    // (a zero den: every wq was 0, so every num is 0 too)
                const unsigned long long a0 = acc[tid][0], a1 = acc[tid][1], a2 = acc[tid][2];
                atomicAdd(&g_den[record], d);
                if (a0) atomicAdd(&g_num[3 * (size_t)record + 0], a0);
                if (a1) atomicAdd(&g_num[3 * (size_t)record + 1], a1);
                if (a2) atomicAdd(&g_num[3 * (size_t)record + 2], a2);
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_refit_apply(float4* __restrict__ records, const long long* __restrict__ num,
                                                     const unsigned long long* __restrict__ den, uint32_t n, double step, unsigned long long D,
                                                     unsigned long long* __restrict__ counters) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool updated = false, clamped = false, starved = false;
    if (i < n) {
        const unsigned long long d = den[i];
        starved = d == 0ull || d < D;
        if (!starved) {
            float4* slot = records + 6 * (size_t)i + 1;                 // color[4] of the 96-byte record
            float4 c = *slot;
            const double scale = (double)d * 4096.0;                    // (exact: a power of two)
            auto channel = [&](float v0, long long nk) {
                if (!isfinite(v0)) return v0;
                const double dlt = (double)nk / scale;
                const double v = (double)v0 + step * dlt;
                const double cl = fmin(fmax(v, 0.0), 1.0);
                clamped = clamped || cl != v;
                return (float)cl;
            };
            const long long* nm = num + 3 * (size_t)i;
            c.x = channel(c.x, nm[0]);
            c.y = channel(c.y, nm[1]);
            c.z = channel(c.z, nm[2]);
            *slot = c;                                                  // (c.w: the bits it was read with)
            updated = true;
        }
    }
    const unsigned long long bu = __ballot(updated), bc = __ballot(clamped), bs = __ballot(starved);
    if ((threadIdx.x & 63) == 0) {
        if (bu) atomicAdd(&counters[0], (unsigned long long)__popcll(bu));
        if (bc) atomicAdd(&counters[1], (unsigned long long)__popcll(bc));
        if (bs) atomicAdd(&counters[2], (unsigned long long)__popcll(bs));
    }
}

}  // namespace

hipError_t refit_blend(const float4* rec, const uint32_t* vals, const uint2* ranges, const uint32_t* order, int W, int H,
                       const uint32_t* sources, const uint32_t* target, const uint32_t* render, uint32_t min_cover, long long* num,
                       unsigned long long* den, unsigned long long* pixels, hipStream_t st) {
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_splat_refit, dim3((uint32_t)(tiles_x * tiles_y)), dim3(256), 0, st, rec, vals, ranges, order, W, H, tiles_x, sources,
                       target, render, min_cover, reinterpret_cast<unsigned long long*>(num), den, pixels);
    return hipGetLastError();
}

hipError_t refit_apply(float4* records, const long long* num, const unsigned long long* den, uint32_t n, double step, unsigned long long D,
                       unsigned long long* counters, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_refit_apply, dim3((n + 255u) / 256u), dim3(256), 0, st, records, num, den, n, step, D, counters);
    return hipGetLastError();
}

}  // namespace m2s
