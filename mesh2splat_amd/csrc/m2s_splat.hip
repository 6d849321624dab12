// m2s_splat.hip — the splat pass: GaussianSplattingPass::execute (GaussianSplattingPass.cpp:50-95) draws one instanced quad per
// sorted Gaussian (gaussianSplattingVS.glsl:31-40) and blends gaussianSplattingPS.glsl:29-45 front to back into a five-target
// G-buffer (renderer.cpp:325-380).  Here as a tile-based compute pass; the semantics it follows operation for operation are the
// ones include/m2s.h pins (m2s_splat), and tests/splat_ref.py restates them in numpy.
//
//   1. setup / bin   k_splat_setup: one thread per quad — the four vertices, the W x H viewport transform, the 24.8 snap, the two
//                    triangles' raster setup (raster_setup_wh, m2s_devfn.h), the guard band and the finiteness test (skipped quads
//                    are counted), the 16 x 16 tile range, and a compact 128-byte record of what the fragments need.  An exclusive
//                    scan of the per-quad tile counts gives the exact number of (tile, quad) pairs (read back once: the pair buffers
//                    are sized from it), and k_splat_pairs writes them in quad order.
//   2. grouping      rocPRIM's LSD radix sort of the pairs over the tile-id bits only — stable, so array order survives inside a
//                    tile —, the start / end of every tile's list, and the tiles ordered by the length of their list, longest first.
//   3. blend         k_splat_blend: one workgroup per tile (in that order), one lane per pixel.  The tile's quads stream through LDS
//                    in batches of 256; the staging thread turns each into per-tile edge thresholds (exact int64 arithmetic once
//                    per (quad, tile); the lanes then test coverage with 32-bit products), then every lane runs exp and the 20
//                    channels of the blend with the per-fragment quantisation of the pin.  A pixel whose five alphas are exactly
//                    1.0 (and whose float planes hold no -0) no longer changes under a finite source: it skips quads whose sources
//                    are provably finite, and a batch is skipped by the whole workgroup when every pixel and every quad qualifies.
//                    A wave (four rows of the tile) skips the quads whose pixel box does not reach its rows without testing them.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "m2s_devfn.h"
#include "m2s_quadraster.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr int kTile = kSplatTile;          // 16 x 16 pixels = 256 lanes
constexpr int kBatch = 256;                // quads staged in LDS per round (one per staging thread)
constexpr uint32_t kFlagTri0 = kQuadTri0, kFlagTri1 = kQuadTri1, kFlagTame = 4u;
constexpr int kWaveShift = 8;              // bits 8..11 of a staged quad's flags: the waves of the tile whose rows its box reaches

// The 128-byte record of one quad (8 x float4):
//   [0] X[4]  [1] Y[4]  snapped window coordinates (24.8) of the four vertices
//   [2] flags, tile box (tx0 | ty0 << 16), (tx1 | ty1 << 16), unused
//   [3] screen.x, screen.y, -0.5 conic.x, -0.5 conic.z
//   [4] -conic.y, conic.w (depth), colour.a, normal.w (metallic)
//   [5] colour.rgb * colour.a, ws.w (roughness)
//   [6] ws.xyz, normal.x
//   [7] normal.yz, 0, 0
constexpr int kRecF4 = 8;

// Sources provably finite for every fragment of the quad (what lets a saturated pixel skip it): a positive definite conic with a
// margin far above the rounding of the fp32 alpha (so alpha <= 0 and 0 <= g <= 1 wherever it is evaluated), magnitudes that keep
// every product finite, and a finite premultiplied colour.
__device__ __forceinline__ bool quad_tame(float4 m, float4 co, float3 pre) {
    if (!(fabsf(m.x) <= 64.0f && fabsf(m.y) <= 64.0f)) return false;                        // |d| < 2^19 px
    if (!(co.x > 0.0f && co.z > 0.0f && fabsf(co.x) <= 1e20f && fabsf(co.y) <= 1e20f && fabsf(co.z) <= 1e20f)) return false;
    const double cx = co.x, cy = co.y, cz = co.z;
    const double h = 0.5 * (cx - cz);
    const double lmin = 0.5 * (cx + cz) - sqrt(h * h + cy * cy);
    if (!(lmin > 1e-4 * (cx + cz))) return false;
    return isfinite(pre.x) && isfinite(pre.y) && isfinite(pre.z);
}

__global__ void __launch_bounds__(256) k_splat_setup(const float4* __restrict__ q, uint32_t n, int W, int H, float4* __restrict__ rec,
                                                     uint32_t* __restrict__ cnt, unsigned long long* __restrict__ skipped) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool skip = false;
    if (i < n) {
        const float4 m = q[6ull * i + 0], s = q[6ull * i + 1], col = q[6ull * i + 2], co = q[6ull * i + 3], nr = q[6ull * i + 4],
                     ws = q[6ull * i + 5];
        const bool fin = isfinite(m.x) && isfinite(m.y) && finite4(s) && finite4(col) && finite4(co) && finite4(nr) && finite4(ws);
        QuadBox qb;
        quad_snap_box(m, s, fin, W, H, qb);
        skip = qb.skip;
        uint32_t flags = qb.flags, c = 0;
        const int* X = qb.X;
        const int* Y = qb.Y;
        const float3 pre = make_float3(col.x * col.w, col.y * col.w, col.z * col.w);
        if (!skip && quad_tame(m, co, pre)) flags |= kFlagTame;
        uint32_t tb0 = 0, tb1 = 0;
        if (flags & (kFlagTri0 | kFlagTri1)) c = quad_tile_box(qb, 0, tb0, tb1);
        cnt[i] = c;
        float4* o = rec + (size_t)kRecF4 * i;
        o[0] = make_float4(__int_as_float(X[0]), __int_as_float(X[1]), __int_as_float(X[2]), __int_as_float(X[3]));
        o[1] = make_float4(__int_as_float(Y[0]), __int_as_float(Y[1]), __int_as_float(Y[2]), __int_as_float(Y[3]));
        o[2] = make_float4(__uint_as_float(flags), __uint_as_float(tb0), __uint_as_float(tb1), 0.0f);
        // gaussianSplattingVS.glsl:34-40: out_screen = ((mean.xy + 1) * 0.5) * u_resolution, out_conic = (-0.5 cx, -cy, -0.5 cz)
        const float sx = ((m.x + 1.0f) * 0.5f) * (float)W, sy = ((m.y + 1.0f) * 0.5f) * (float)H;
        o[3] = make_float4(sx, sy, -0.5f * co.x, -0.5f * co.z);
        o[4] = make_float4(-co.y, co.w, col.w, nr.w);
        o[5] = make_float4(pre.x, pre.y, pre.z, ws.w);
        o[6] = make_float4(ws.x, ws.y, ws.z, nr.x);
        o[7] = make_float4(nr.y, nr.z, 0.0f, 0.0f);
    }
    const unsigned long long b = __ballot(skip);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(skipped, (unsigned long long)__popcll(b));
}

// totals[0] = (tile, quad) pairs = off[n-1] + cnt[n-1]
__global__ void k_splat_total(const unsigned long long* __restrict__ off, const uint32_t* __restrict__ cnt, uint32_t n,
                              unsigned long long* __restrict__ totals) {
    if (threadIdx.x == 0 && blockIdx.x == 0) totals[0] = off[n - 1] + cnt[n - 1];
}

__global__ void __launch_bounds__(256) k_splat_pairs(const float4* __restrict__ rec, const uint32_t* __restrict__ cnt,
                                                     const unsigned long long* __restrict__ off, uint32_t n, int tiles_x,
                                                     uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || cnt[i] == 0) return;
    const float4 r2 = rec[(size_t)kRecF4 * i + 2];
    const uint32_t tb0 = __float_as_uint(r2.y), tb1 = __float_as_uint(r2.z);
    emit_tile_pairs(tb0, tb1, tiles_x, (size_t)off[i], i, keys, vals);
}

// start / end of every tile's run in the sorted pairs (ranges zeroed beforehand), and the run lengths for the tile order
__global__ void __launch_bounds__(256) k_splat_ranges(const uint32_t* __restrict__ keys, uint32_t p, uint2* __restrict__ ranges) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p) return;
    const uint32_t k = keys[i];
    if (i == 0 || keys[i - 1] != k) ranges[k].x = i;
    if (i == p - 1 || keys[i + 1] != k) ranges[k].y = i + 1;
}
__global__ void __launch_bounds__(256) k_splat_lengths(const uint2* __restrict__ ranges, uint32_t n_tiles, uint32_t* __restrict__ len) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < n_tiles) len[t] = ranges[t].y - ranges[t].x;
}

// ---- blend ---------------------------------------------------------------------------------------------------------------
struct __align__(16) StagedQuad {
    int4 e0;   // tri 0: a[0..2], T[0]
    int4 e1;   // tri 0: b[0..2], T[1]
    int4 e2;   // tri 1: a[0..2], T[0]
    int4 e3;   // tri 1: b[0..2], T[1]
    int4 e4;   // T[2] of tri 0, T[2] of tri 1, flags (this tile), unused
    float4 f[5];   // record words [3..7]
};

__device__ __forceinline__ float h16(float v) { return (float)(_Float16)v; }        // RNE to half and back (subnormals kept)
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
// the RGBA8 value read back: q / 255.0f, correctly rounded — (float)(q * (1/255.0)) in double equals it for every q in 0..255
__device__ __forceinline__ float unorm8(float r) {
    const float q = rintf(clamp01(r) * 255.0f);
    return (float)((double)q * (1.0 / 255.0));
}

template <bool kOverdraw>
__global__ void __launch_bounds__(256) k_splat_blend(const float4* __restrict__ rec, const uint32_t* __restrict__ vals,
                                                     const uint2* __restrict__ ranges, const uint32_t* __restrict__ order, int W, int H,
                                                     int tiles_x, uint2* __restrict__ g_pos, uint2* __restrict__ g_nrm,
                                                     uint32_t* __restrict__ g_alb, uint2* __restrict__ g_dep, uint32_t* __restrict__ g_mr,
                                                     unsigned long long* __restrict__ frag_count) {
    __shared__ StagedQuad sq[kBatch];
    __shared__ uint32_t wg_frags;
    const int tid = threadIdx.x;
    const uint32_t tile = order ? order[blockIdx.x] : blockIdx.x;
    const int px0 = (int)(tile % (uint32_t)tiles_x) * kTile, py0 = (int)(tile / (uint32_t)tiles_x) * kTile;
    const int lx = tid & (kTile - 1), ly = tid / kTile;
    const int x = px0 + lx, y = py0 + ly;
    const bool in_view = x < W && y < H;
    const uint32_t wave_bit = 1u << (kWaveShift + tid / 64);
    const float fx = (float)x + 0.5f, fy = (float)y + 0.5f;            // gl_FragCoord.xy
    uint32_t begin = 0, end = 0;
    if (ranges) { const uint2 rg = ranges[tile]; begin = rg.x; end = rg.y; }
    if (tid == 0) wg_frags = 0;
    __syncthreads();

    // destination values as read back (half-exact / q / 255): position, normal, depth (its three colour channels are equal), albedo, MR
    float P0 = 0, P1 = 0, P2 = 0, P3 = 0, N0 = 0, N1 = 0, N2 = 0, N3 = 0, D0 = 0, D3 = 0;
    float A0 = 0, A1 = 0, A2 = 0, A3 = 0, M0 = 0, M1 = 0, M3 = 0;
    uint32_t frags = 0;

    for (uint32_t base = begin; base < end; base += kBatch) {
        const uint32_t m = min((uint32_t)kBatch, end - base);
        bool tame_or_absent = true;
        __syncthreads();                                              // the previous batch has been consumed
        if ((uint32_t)tid < m) {
            const uint32_t qi = vals[base + tid];
            const float4* r = rec + (size_t)kRecF4 * qi;
            const float4 r0 = r[0], r1 = r[1], r2 = r[2];
            const int X[4] = { __float_as_int(r0.x), __float_as_int(r0.y), __float_as_int(r0.z), __float_as_int(r0.w) };
            const int Y[4] = { __float_as_int(r1.x), __float_as_int(r1.y), __float_as_int(r1.z), __float_as_int(r1.w) };
            const uint32_t qf = __float_as_uint(r2.x);
            uint32_t fl = qf & kFlagTame;
            StagedQuad s;
            s.e0 = s.e1 = s.e2 = s.e3 = make_int4(0, 0, 0, kTMax);
            int t20 = kTMax, t21 = kTMax;
            const int X0[3] = { X[0], X[1], X[2] }, Y0[3] = { Y[0], Y[1], Y[2] };
            const int X1[3] = { X[0], X[2], X[3] }, Y1[3] = { Y[0], Y[2], Y[3] };
            uint32_t waves = 0;
            if ((qf & kFlagTri0) && box_meets_tile(X0, Y0, W, H, px0, py0, &waves)) { stage_triangle(X0, Y0, px0, py0, s.e0, s.e1, t20); fl |= kFlagTri0; }
            if ((qf & kFlagTri1) && box_meets_tile(X1, Y1, W, H, px0, py0, &waves)) { stage_triangle(X1, Y1, px0, py0, s.e2, s.e3, t21); fl |= kFlagTri1; }
            fl |= waves << kWaveShift;
            s.e4 = make_int4(t20, t21, (int)fl, 0);
#pragma unroll
            for (int k = 0; k < 5; ++k) s.f[k] = r[3 + k];
            sq[tid] = s;
            tame_or_absent = (fl & kFlagTame) || !(fl & (kFlagTri0 | kFlagTri1));
        }
        // A pixel is saturated when its five alphas are exactly 1.0 and no colour channel of the float planes holds -0: then
        // t = 1 - 1 = 0 and a finite source adds +-0, which leaves every stored value as it is.
        bool sat = !in_view;
        if (!kOverdraw && in_view) {
            const bool negz = __float_as_uint(P0) == 0x80000000u || __float_as_uint(P1) == 0x80000000u || __float_as_uint(P2) == 0x80000000u ||
                              __float_as_uint(N0) == 0x80000000u || __float_as_uint(N1) == 0x80000000u || __float_as_uint(N2) == 0x80000000u ||
                              __float_as_uint(D0) == 0x80000000u;
            sat = P3 == 1.0f && N3 == 1.0f && D3 == 1.0f && A3 == 1.0f && M3 == 1.0f && !negz;
        }
        const bool skip_batch = __syncthreads_and(sat && tame_or_absent);  // (also the barrier behind the staging)
        if (!kOverdraw && skip_batch) continue;
        for (uint32_t e = 0; e < m; ++e) {
            const int4 e4 = sq[e].e4;
            const uint32_t fl = (uint32_t)e4.z;
            if (!(fl & wave_bit)) continue;                             // (wave-uniform: no row of this wave is in the quad's box)
            if (!kOverdraw && sat && (fl & kFlagTame)) continue;
            int cov = 0;
            if (fl & kFlagTri0) {
                const int4 a = sq[e].e0, b = sq[e].e1;
                cov += (a.x * lx + b.x * ly > a.w) & (a.y * lx + b.y * ly > b.w) & (a.z * lx + b.z * ly > e4.x);
            }
            if (fl & kFlagTri1) {
                const int4 a = sq[e].e2, b = sq[e].e3;
                cov += (a.x * lx + b.x * ly > a.w) & (a.y * lx + b.y * ly > b.w) & (a.z * lx + b.z * ly > e4.y);
            }
            if (!cov) continue;
            const float4 f3 = sq[e].f[0], f4 = sq[e].f[1], f5 = sq[e].f[2], f6 = sq[e].f[3], f7 = sq[e].f[4];
            // gaussianSplattingPS.glsl:30-32: d = out_screen - gl_FragCoord.xy; alpha = dot(conic.xzy, (d*d, d.x*d.y)); g = exp(alpha)
            const float dx = f3.x - fx, dy = f3.y - fy;
            const float alpha = (f3.z * (dx * dx) + f3.w * (dy * dy)) + f4.x * (dx * dy);
            const float g = __expf(alpha);
            // the five sources (PS:34-45)
            const float op = f4.z, opg = op * g;
            const float sP0 = f6.x * g, sP1 = f6.y * g, sP2 = f6.z * g, sP3 = g;
            const float sN0 = f6.w * g, sN1 = f7.x * g, sN2 = f7.y * g;
            const float sD = f4.y * g;
            float sA0, sA1, sA2, sA3;
            if (kOverdraw) { sA0 = 0.01f; sA1 = 0.005f; sA2 = 0.0f; sA3 = 0.01f; }
            else { sA0 = f5.x * g; sA1 = f5.y * g; sA2 = f5.z * g; sA3 = opg; }
            const float sM0 = clamp01(f4.w * g), sM1 = clamp01(f5.w * g), sM3 = clamp01(g);
            sA0 = clamp01(sA0); sA1 = clamp01(sA1); sA2 = clamp01(sA2); sA3 = clamp01(sA3);
            for (int k = 0; k < cov; ++k) {
                frags++;
                if (kOverdraw) {                                        // glBlendFunc(GL_ONE, GL_ONE)
                    P0 = h16(sP0 + P0); P1 = h16(sP1 + P1); P2 = h16(sP2 + P2); P3 = h16(sP3 + P3);
                    N0 = h16(sN0 + N0); N1 = h16(sN1 + N1); N2 = h16(sN2 + N2); N3 = h16(opg + N3);
                    D0 = h16(sD + D0); D3 = h16(opg + D3);
                    A0 = unorm8(sA0 + A0); A1 = unorm8(sA1 + A1); A2 = unorm8(sA2 + A2); A3 = unorm8(sA3 + A3);
                    M0 = unorm8(sM0 + M0); M1 = unorm8(sM1 + M1); M3 = unorm8(sM3 + M3);
                } else {                                                // glBlendFunc(GL_ONE_MINUS_DST_ALPHA, GL_ONE), per attachment
                    const float tP = 1.0f - P3, tN = 1.0f - N3, tD = 1.0f - D3, tA = 1.0f - A3, tM = 1.0f - M3;
                    P0 = h16(sP0 * tP + P0); P1 = h16(sP1 * tP + P1); P2 = h16(sP2 * tP + P2); P3 = h16(sP3 * tP + P3);
                    N0 = h16(sN0 * tN + N0); N1 = h16(sN1 * tN + N1); N2 = h16(sN2 * tN + N2); N3 = h16(opg * tN + N3);
                    D0 = h16(sD * tD + D0); D3 = h16(opg * tD + D3);
                    A0 = unorm8(sA0 * tA + A0); A1 = unorm8(sA1 * tA + A1); A2 = unorm8(sA2 * tA + A2); A3 = unorm8(sA3 * tA + A3);
                    M0 = unorm8(sM0 * tM + M0); M1 = unorm8(sM1 * tM + M1); M3 = unorm8(sM3 * tM + M3);
                }
            }
        }
    }
    if (in_view) {
        const size_t px = (size_t)y * (size_t)W + (size_t)x;
        auto pack_h = [](float a, float b, float c, float d) {
            const uint32_t ha = __builtin_bit_cast(uint16_t, (_Float16)a), hb = __builtin_bit_cast(uint16_t, (_Float16)b);
            const uint32_t hc = __builtin_bit_cast(uint16_t, (_Float16)c), hd = __builtin_bit_cast(uint16_t, (_Float16)d);
            return make_uint2(ha | (hb << 16), hc | (hd << 16));
        };
        auto pack_8 = [](float a, float b, float c, float d) {
            return (uint32_t)rintf(a * 255.0f) | ((uint32_t)rintf(b * 255.0f) << 8) | ((uint32_t)rintf(c * 255.0f) << 16) |
                   ((uint32_t)rintf(d * 255.0f) << 24);
        };
        g_pos[px] = pack_h(P0, P1, P2, P3);
        g_nrm[px] = pack_h(N0, N1, N2, N3);
        g_dep[px] = pack_h(D0, D0, D0, D3);
        g_alb[px] = pack_8(A0, A1, A2, A3);
        g_mr[px] = pack_8(M0, M1, 0.0f, M3);
    }
    if (frag_count) {
        __syncthreads();
        atomicAdd(&wg_frags, frags);
        __syncthreads();
        if (tid == 0 && wg_frags) atomicAdd(frag_count, (unsigned long long)wg_frags);
    }
}

}  // namespace

// ---- host side --------------------------------------------------------------------------------------------------------------
size_t splat_scan_temp_bytes(uint32_t n) {
    size_t b = 0;
    (void)rocprim::exclusive_scan(nullptr, b, (const uint32_t*)nullptr, (unsigned long long*)nullptr, 0ull, (size_t)n,
                                  rocprim::plus<unsigned long long>(), (hipStream_t)0);
    return b;
}
size_t splat_sort_temp_bytes(uint32_t pairs, uint32_t n_tiles) {
    size_t b = 0, bt = 0;
    (void)rocprim::radix_sort_pairs(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, pairs, 0, 32,
                                    (hipStream_t)0);
    (void)rocprim::radix_sort_pairs_desc(nullptr, bt, (uint32_t*)nullptr, (uint32_t*)nullptr, rocprim::counting_iterator<uint32_t>(0),
                                         (uint32_t*)nullptr, n_tiles, 0, 32, (hipStream_t)0);
    return std::max(b, bt);
}

hipError_t splat_setup(const float4* quads, uint32_t n, int W, int H, float4* rec, uint32_t* cnt, unsigned long long* off, void* temp,
                       size_t temp_bytes, unsigned long long* totals, hipStream_t st) {
    const uint32_t blocks = (n + 255u) / 256u;
    hipLaunchKernelGGL(k_splat_setup, dim3(blocks), dim3(256), 0, st, quads, n, W, H, rec, cnt, totals + 1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(temp, temp_bytes, (const uint32_t*)cnt, off, 0ull, (size_t)n, rocprim::plus<unsigned long long>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_splat_total, dim3(1), dim3(64), 0, st, (const unsigned long long*)off, (const uint32_t*)cnt, n, totals);
    return hipGetLastError();
}

hipError_t splat_pairs(const float4* rec, const uint32_t* cnt, const unsigned long long* off, uint32_t n, int tiles_x, uint32_t* keys,
                       uint32_t* vals, hipStream_t st) {
    hipLaunchKernelGGL(k_splat_pairs, dim3((n + 255u) / 256u), dim3(256), 0, st, rec, cnt, off, n, tiles_x, keys, vals);
    return hipGetLastError();
}

hipError_t splat_group(uint32_t* keys_in, uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out, uint32_t pairs, uint32_t n_tiles,
                       uint2* ranges, uint32_t* len, uint32_t* len_sorted, uint32_t* order, void* temp, size_t temp_bytes, hipStream_t st) {
    int bits = 1;
    while ((1u << bits) < n_tiles) ++bits;
    hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, pairs, 0, bits, st);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(ranges, 0, (size_t)n_tiles * sizeof(uint2), st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_splat_ranges, dim3((pairs + 255u) / 256u), dim3(256), 0, st, (const uint32_t*)keys_out, pairs, ranges);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_splat_lengths, dim3((n_tiles + 255u) / 256u), dim3(256), 0, st, (const uint2*)ranges, n_tiles, len);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // longest list first: the dispatcher hands out workgroups in index order, so the heavy tiles start before the light ones
    return rocprim::radix_sort_pairs_desc(temp, temp_bytes, len, len_sorted, rocprim::counting_iterator<uint32_t>(0), order, n_tiles, 0, 32, st);
}

hipError_t splat_blend(const float4* rec, const uint32_t* vals, const uint2* ranges, const uint32_t* order, int W, int H, int render_mode,
                       void* const planes[5], unsigned long long* frag_count, hipStream_t st) {
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
    const dim3 grid((uint32_t)(tiles_x * tiles_y));
    auto k = render_mode == 4 ? k_splat_blend<true> : k_splat_blend<false>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, st, rec, vals, ranges, order, W, H, tiles_x, (uint2*)planes[0], (uint2*)planes[1],
                       (uint32_t*)planes[2], (uint2*)planes[3], (uint32_t*)planes[4], frag_count);
    return hipGetLastError();
}

hipError_t preload_splat() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_splat_setup)); }

}  // namespace m2s
