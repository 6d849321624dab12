// m2s_light.hip — the last two passes of the viewer's frame: the Gaussian shadow pass (GaussianShadowPass.cpp:83-236,
// gaussianPointShadowMappingCS.glsl, gaussianPointLightCubeMapShadow{VS,PS}.glsl) and the deferred relighting pass
// (GaussianRelightingPass.cpp:136-143, gaussianSplattingDeferredPS.glsl).  The semantics are the ones include/m2s.h pins (m2s_shadow,
// m2s_relight); tests/light_ref.py restates them in numpy.
//
// Shadow pass, stage A (every record of the scene, every frame): the viewer prepass seen from the six 90-degree cameras of the light.
//   k_shadow_quads<false>  one lane per record: world position, cube face, that face's camera, the 1.05 w cull, the covariance
//                          projection (m2s_covmath.h: the prepass's own functions) and the lambda2 cull; per workgroup the number of
//                          survivors of each face.  An exclusive scan over the face-major table gives where every (face, workgroup)
//                          starts in ONE buffer that holds the six lists back to back, and the six list lengths (read back once:
//                          the buffer is exact-size).
//   k_shadow_quads<true>   the same arithmetic again, survivors written at table base + rank inside the workgroup (ballot +
//                          popcount): every list in INPUT order, no atomics.  Recomputing costs a second read of the records
//                          (96 B) and saves writing, re-reading and compacting 48 B per record.
// Shadow pass, stage B (the six instanced draws with depth test and gl_FragDepth = |ws - light| / far, constant per quad): a texel
// ends as min(1, min over covering quads of d) — order-independent and idempotent, so:
//   k_shadow_setup         one lane per quad: vertices, S x S viewport, 24.8 snap, guard band, the two triangles' raster setup, d, the
//                          box of 16 x 16 tiles on the 6-face atlas (tile row = face * tiles_y + row); skipped quads are counted.
//   scan + k_shadow_pairs  exact number of (tile, quad) pairs, the pairs in quad order; rocPRIM radix sort over the tile-id bits.
//   k_shadow_tiles         the SORTED PAIR ARRAY is cut into chunks of 256, one workgroup each, whatever tiles they belong to — a
//                          tile with a long list is spread over many workgroups (min is associative), a chunk with many short
//                          lists handles them one after the other.  Staging: one thread per pair, exact int64 edge thresholds for
//                          its tile (m2s_quadraster.h, the splat pass's).  Then one lane per texel of the current tile: coverage
//                          with 32-bit products, running min in a register; when the tile changes (and at the end) the lanes
//                          whose min is below the texel's current value (a plain read) send one atomicMin on the depth bits
//                          (non-negative floats order as unsigned integers).  A quad that spans hundreds of texels is therefore
//                          256 lanes wide per tile and one tile per pair: no lane loops over a quad's texels.
// Relighting pass:
//   k_relight              one lane per pixel: texel fetch of the four G-buffer planes it reads, the 20-tap shadow count (decision
//                          arithmetic: IEEE fp32 operation by operation), the shader's PBR arithmetic (value arithmetic: fp32 with
//                          the device's fast log2 / exp2 / rsq), RGBA8 out.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "m2s_devfn.h"
#include "m2s_quadraster.h"
#include "m2s_viewmath.h"
#include "m2s_covmath.h"
#include "m2s_lightmath.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr int kTile = kSplatTile;
constexpr uint32_t kOne = 0x3F800000u;      // 1.0f: the cube's clear value

// gaussianPointShadowMappingCS.glsl:58-207 for one record.  -> the cube face 0..5 of a survivor (q: its QuadNdcTransformation), -1 culled.
__device__ __forceinline__ int shadow_one(const PrepassK& k, const float* __restrict__ views, float lx, float ly, float lz, float4 gpos, float4 gscl,
                                          float4 grot, float4 (&q)[3]) {
    const float4 ws = m4_mul(k.M, gpos.x, gpos.y, gpos.z, 1.0f);                  // :80
    // :58-69 determineFaceIndex; normalize pinned as v / sqrt((x x + y y) + z z) (0/0 = NaN at the light: every test below is false -> face 5)
    const float dx = ws.x - lx, dy = ws.y - ly, dz = ws.z - lz;
    const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
    const float nx = dx / len, ny = dy / len, nz = dz / len;
    const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
    int face;
    if (ax >= ay && ax >= az) face = nx > 0.0f ? 0 : 1;
    else if (ay >= ax && ay >= az) face = ny > 0.0f ? 2 : 3;
    else face = nz > 0.0f ? 4 : 5;
    float V[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) V[i] = views[face * 16 + i];
    const float4 vs = m4_mul(V, ws.x, ws.y, ws.z, 1.0f);                          // :85
    float4 pos2d = m4_mul(k.P, vs.x, vs.y, vs.z, vs.w);                           // :87
    if (!clip_inside(pos2d)) return -1;                                           // :89-94
    M3 rot;
    const M3 cov3d = gaussian_cov3d(k, gscl, grot, rot);                          // :96-112
    pos2d.x = pos2d.x / pos2d.w; pos2d.y = pos2d.y / pos2d.w; pos2d.z = pos2d.z / pos2d.w;   // :153
    Cov2D cv;
    project_cov(V, k.P, k.res, k.near_far, vs, cov3d, cv);                        // :160-196 (u_resolution: the RENDERER's)
    if (cv.lambda2 < 0.0f) return -1;                                             // :189
    q[0] = pos2d;                                                                 // :204-206
    q[1] = cv.quad_scale;
    q[2] = ws;
    return face;
}

// cnt / off: [face][workgroup] (+ one trailing word): survivors of the face in the workgroup / where they start in the buffer
template <bool kEmit>
__global__ void __launch_bounds__(256) k_shadow_quads(const PrepassK k, const float* __restrict__ views, float lx, float ly, float lz,
                                                      const float4* __restrict__ rec, uint32_t n, uint32_t nb, uint32_t* __restrict__ cnt,
                                                      const uint32_t* __restrict__ off, float4* __restrict__ quads) {
    __shared__ uint32_t s_cnt[4][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    int face = -1;
    float4 q[3];
    if (i < n) {
        const float4* g = rec + (size_t)i * 6;
        face = shadow_one(k, views, lx, ly, lz, g[0], g[2], g[4], q);
    }
    uint32_t rank = 0;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const unsigned long long mask = __ballot(face == f);
        if (lane == 0) s_cnt[wave][f] = (uint32_t)__popcll(mask);
        if (face == f) rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (!kEmit) {
        if (threadIdx.x < 6) cnt[(size_t)threadIdx.x * nb + blockIdx.x] = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
    } else if (face >= 0) {
        uint32_t base = off[(size_t)face * nb + blockIdx.x] + rank;
        for (int w = 0; w < wave; ++w) base += s_cnt[w][face];
        float4* o = quads + (size_t)base * 3;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
    }
}

// bases[f] = first quad of face f in the buffer, bases[6] = all quads
__global__ void k_shadow_bases(const uint32_t* __restrict__ off, uint32_t nb, uint32_t* __restrict__ bases) {
    if (threadIdx.x < 7) bases[threadIdx.x] = off[(size_t)threadIdx.x * nb];
}

// The 48-byte record of one quad (3 x float4): [0] X[4], [1] Y[4] snapped window coordinates (24.8) on its face,
// [2] flags, tile box (tx0 | ty0 << 16), (tx1 | ty1 << 16) with atlas rows (face * tiles_y + row), d
constexpr uint32_t kFlagTri0 = kQuadTri0, kFlagTri1 = kQuadTri1;

__global__ void __launch_bounds__(256) k_shadow_setup(const float4* __restrict__ q, uint32_t n, ShadowBases fb, int S, int tiles_y, float lx, float ly,
                                                      float lz, float far_plane, float4* __restrict__ rec, uint32_t* __restrict__ cnt,
                                                      unsigned long long* __restrict__ skipped) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool skip = false;
    if (i < n) {
        const int face = (int)(i >= fb.b[1]) + (int)(i >= fb.b[2]) + (int)(i >= fb.b[3]) + (int)(i >= fb.b[4]) + (int)(i >= fb.b[5]);
        const float4 m = q[3ull * i + 0], s = q[3ull * i + 1], ws = q[3ull * i + 2];
        const bool fin = isfinite(m.x) && isfinite(m.y) && finite4(s) && finite4(ws);
        QuadBox qb;
        quad_snap_box(m, s, fin, S, S, qb);
        skip = qb.skip;
        uint32_t flags = qb.flags, c = 0;
        const int* X = qb.X;
        const int* Y = qb.Y;
        // gaussianPointLightCubeMapShadowPS.glsl: gl_FragDepth = length(out_pos - u_lightPos) / u_farPlane, stored clamped to [0, 1]
        const float dx = ws.x - lx, dy = ws.y - ly, dz = ws.z - lz;
        float d = sqrtf((dx * dx + dy * dy) + dz * dz) / far_plane;
        d = d > 0.0f ? fminf(d, 1.0f) : (d == d ? 0.0f : 1.0f);           // (NaN: never passes GL_LESS)
        if (!(d < 1.0f)) flags = 0;                                       // cannot pass GL_LESS against the clear value: no pairs
        uint32_t tb0 = 0, tb1 = 0;
        if (flags) c = quad_tile_box(qb, face * tiles_y, tb0, tb1);
        cnt[i] = c;
        float4* o = rec + 3ull * i;
        o[0] = make_float4(__int_as_float(X[0]), __int_as_float(X[1]), __int_as_float(X[2]), __int_as_float(X[3]));
        o[1] = make_float4(__int_as_float(Y[0]), __int_as_float(Y[1]), __int_as_float(Y[2]), __int_as_float(Y[3]));
        o[2] = make_float4(__uint_as_float(flags), __uint_as_float(tb0), __uint_as_float(tb1), d);
    }
    const unsigned long long b = __ballot(skip);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(skipped, (unsigned long long)__popcll(b));
}

__global__ void k_shadow_total(const unsigned long long* __restrict__ off, const uint32_t* __restrict__ cnt, uint32_t n,
                               unsigned long long* __restrict__ totals) {
    if (threadIdx.x == 0 && blockIdx.x == 0) totals[0] = off[n - 1] + cnt[n - 1];
}

__global__ void __launch_bounds__(256) k_shadow_pairs(const float4* __restrict__ rec, const uint32_t* __restrict__ cnt,
                                                      const unsigned long long* __restrict__ off, uint32_t n, int tiles_x,
                                                      uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || cnt[i] == 0) return;
    const float4 r2 = rec[3ull * i + 2];
    const uint32_t tb0 = __float_as_uint(r2.y), tb1 = __float_as_uint(r2.z);
    emit_tile_pairs(tb0, tb1, tiles_x, (size_t)off[i], i, keys, vals);
}

struct __align__(16) StagedShadow {
    int4 e0, e1;   // tri 0: a[0..2], T[0];  b[0..2], T[1]
    int4 e2, e3;   // tri 1
    int4 e4;       // T[2] of tri 0, T[2] of tri 1, flags (this tile), tile key
};

__global__ void __launch_bounds__(256) k_shadow_tiles(const float4* __restrict__ rec, const uint32_t* __restrict__ keys,
                                                      const uint32_t* __restrict__ vals, uint32_t pairs, int S, int tiles_x, int tiles_y,
                                                      uint32_t* __restrict__ cube, unsigned long long* __restrict__ writes) {
    __shared__ StagedShadow sq[256];
    __shared__ float sd[256];
    __shared__ uint32_t wg_writes;
    const int tid = threadIdx.x;
    const int lx = tid & (kTile - 1), ly = tid / kTile;
    const uint32_t base = blockIdx.x * 256u;
    const uint32_t m = min(256u, pairs - base);
    if (tid == 0) wg_writes = 0;
    if ((uint32_t)tid < m) {
        const uint32_t key = keys[base + tid], qi = vals[base + tid];
        const float4* r = rec + 3ull * qi;
        const float4 r0 = r[0], r1 = r[1], r2 = r[2];
        const int X[4] = { __float_as_int(r0.x), __float_as_int(r0.y), __float_as_int(r0.z), __float_as_int(r0.w) };
        const int Y[4] = { __float_as_int(r1.x), __float_as_int(r1.y), __float_as_int(r1.z), __float_as_int(r1.w) };
        const uint32_t qf = __float_as_uint(r2.x);
        const int px0 = (int)(key % (uint32_t)tiles_x) * kTile, py0 = (int)((key / (uint32_t)tiles_x) % (uint32_t)tiles_y) * kTile;
        StagedShadow s;
        s.e0 = s.e1 = s.e2 = s.e3 = make_int4(0, 0, 0, kTMax);
        int t20 = kTMax, t21 = kTMax;
        const int X0[3] = { X[0], X[1], X[2] }, Y0[3] = { Y[0], Y[1], Y[2] };
        const int X1[3] = { X[0], X[2], X[3] }, Y1[3] = { Y[0], Y[2], Y[3] };
        uint32_t fl = 0, waves = 0;
        if ((qf & kFlagTri0) && box_meets_tile(X0, Y0, S, S, px0, py0, &waves)) { stage_triangle(X0, Y0, px0, py0, s.e0, s.e1, t20); fl |= kFlagTri0; }
        if ((qf & kFlagTri1) && box_meets_tile(X1, Y1, S, S, px0, py0, &waves)) { stage_triangle(X1, Y1, px0, py0, s.e2, s.e3, t21); fl |= kFlagTri1; }
        s.e4 = make_int4(t20, t21, (int)fl, (int)key);
        sq[tid] = s;
        sd[tid] = r2.w;
    }
    __syncthreads();
    uint32_t sent = 0;
    auto flush = [&](uint32_t key, float dmin) {
        const int x = (int)(key % (uint32_t)tiles_x) * kTile + lx;
        const uint32_t row = key / (uint32_t)tiles_x;                      // atlas row of tiles: face * tiles_y + tile row
        const int y = (int)(row % (uint32_t)tiles_y) * kTile + ly, face = (int)(row / (uint32_t)tiles_y);
        if (x < S && y < S && dmin < 1.0f) {
            uint32_t* p = cube + ((size_t)face * (size_t)S + (size_t)y) * (size_t)S + (size_t)x;
            const uint32_t bits = __float_as_uint(dmin);
            // (the plain read races with other workgroups' atomicMin on this texel; a texel only ever decreases, so a stale value is
            //  at least the current one: it can cause a redundant atomic, never a missed one)
            if (bits < *p) { atomicMin(p, bits); ++sent; }
        }
    };
    uint32_t cur = (uint32_t)sq[0].e4.w;
    float dmin = 1.0f;
    for (uint32_t e = 0; e < m; ++e) {
        const int4 e4 = sq[e].e4;
        if ((uint32_t)e4.w != cur) { flush(cur, dmin); cur = (uint32_t)e4.w; dmin = 1.0f; }     // (workgroup-uniform)
        const uint32_t fl = (uint32_t)e4.z;
        int cov = 0;
        if (fl & kFlagTri0) {
            const int4 a = sq[e].e0, b = sq[e].e1;
            cov |= (a.x * lx + b.x * ly > a.w) & (a.y * lx + b.y * ly > b.w) & (a.z * lx + b.z * ly > e4.x);
        }
        if (fl & kFlagTri1) {
            const int4 a = sq[e].e2, b = sq[e].e3;
            cov |= (a.x * lx + b.x * ly > a.w) & (a.y * lx + b.y * ly > b.w) & (a.z * lx + b.z * ly > e4.y);
        }
        if (cov) dmin = fminf(dmin, sd[e]);
    }
    flush(cur, dmin);
    if (writes) {
        if (sent) atomicAdd(&wg_writes, sent);
        __syncthreads();
        if (tid == 0 && wg_writes) atomicAdd(writes, (unsigned long long)wg_writes);
    }
}

// ---- relighting --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float half_lo(uint32_t v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v & 0xFFFFu)); }
__device__ __forceinline__ float half_hi(uint32_t v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v >> 16)); }
// kSplit (GaussianRelightingPass.cpp:90-135): pixels left of split_x are lit from the second set of planes (the mesh G-buffer), the
// two divider columns from div_x on are white; everything else is the one shader.
struct RelightPlanes { const uint2* pos; const uint2* nrm; const uint32_t* alb; const uint32_t* mr; };
template <bool kSplit>
__global__ void __launch_bounds__(256) k_relight(const RelightK k, const uint2* __restrict__ g_pos, const uint2* __restrict__ g_nrm,
                                                 const uint32_t* __restrict__ g_alb, const uint32_t* __restrict__ g_mr,
                                                 const float* __restrict__ cube, uint32_t* __restrict__ frame, uint8_t* __restrict__ counts,
                                                 const RelightPlanes left, int split_x, int div_x) {
    const size_t px = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (px >= (size_t)k.W * (size_t)k.H) return;
    if constexpr (kSplit) {
        const int x = (int)(px % (size_t)k.W);
        if (x >= div_x && x < div_x + 2) {                  // the scissored clear to white, drawn last
            frame[px] = 0xFFFFFFFFu;
            if (counts) counts[px] = 0;
            return;
        }
        if (x < split_x) { g_pos = left.pos; g_nrm = left.nrm; g_alb = left.alb; g_mr = left.mr; }
    }
    const uint32_t alb = g_alb[px];
    if (k.mode != 6) {                                   // :105-117: byte copies
        const uint32_t src = k.mode == 5 ? (g_mr[px] & 0x0000FFFFu) : (alb & 0x00FFFFFFu);
        frame[px] = src | 0xFF000000u;
        return;
    }
    const uint32_t mr = g_mr[px];
    const uint2 pp = g_pos[px], nn = g_nrm[px];
    const float inv255 = 255.0f;
    float a0 = (float)(alb & 255u) / inv255, a1 = (float)((alb >> 8) & 255u) / inv255, a2 = (float)((alb >> 16) & 255u) / inv255;
    const float roughness = (float)((mr >> 8) & 255u) / inv255, metallic = (float)((mr >> 16) & 255u) / inv255;   // :121-122 (pbr.b)
    const float p0 = half_lo(pp.x), p1 = half_hi(pp.x), p2 = half_lo(pp.y);
    float N0 = half_lo(nn.x) * 2.0f - 1.0f, N1 = half_hi(nn.x) * 2.0f - 1.0f, N2 = half_lo(nn.y) * 2.0f - 1.0f;   // :126
    normalize3(N0, N1, N2);
    // ---- computeShadowFactor (:70-99): decision arithmetic, IEEE fp32 operation by operation
    const uint32_t count = shadow_taps(cube, k.S, p0, p1, p2, k.light[0], k.light[1], k.light[2], k.far_plane);
    if (counts) counts[px] = (uint8_t)count;
    const float shadow = (float)count / 20.0f;
    // ---- the rest of main() (:130-164): value arithmetic
    a0 = pow_fast(a0, 2.2f); a1 = pow_fast(a1, 2.2f); a2 = pow_fast(a2, 2.2f);
    float L0 = k.light[0] - p0, L1 = k.light[1] - p1, L2 = k.light[2] - p2;
    const float d2 = dot3(L0, L1, L2, L0, L1, L2);
    const float d = __builtin_amdgcn_sqrtf(d2);
    normalize3(L0, L1, L2);
    float V0 = k.cam[0] - p0, V1 = k.cam[1] - p1, V2 = k.cam[2] - p2;
    normalize3(V0, V1, V2);
    float H0 = V0 + L0, H1 = V1 + L1, H2 = V2 + L2;
    normalize3(H0, H1, H2);
    const float attenuation = 1.0f / (d * d);
    const float r0 = (k.color[0] * k.intensity) * attenuation, r1 = (k.color[1] * k.intensity) * attenuation, r2 = (k.color[2] * k.intensity) * attenuation;
    const float im = 1.0f - metallic;
    const float F00 = 0.04f * im + a0 * metallic, F01 = 0.04f * im + a1 * metallic, F02 = 0.04f * im + a2 * metallic;   // mix
    const float hv = max0(dot3(H0, H1, H2, V0, V1, V2));
    const float fc = fminf(fmaxf(1.0f - hv, 0.0f), 1.0f);
    const float f5 = pow_fast(fc, 5.0f);
    const float F0 = F00 + (1.0f - F00) * f5, F1 = F01 + (1.0f - F01) * f5, F2 = F02 + (1.0f - F02) * f5;
    // DistributionGGX; `PI * denom * denom` with PI the macro 22.0f/7.0f: ((22/7) denom) denom
    const float a = roughness * roughness, aa = a * a;
    const float nh = max0(dot3(N0, N1, N2, H0, H1, H2));
    float den = (nh * nh) * (aa - 1.0f) + 1.0f;
    den = ((22.0f / 7.0f) * den) * den;
    const float NDF = aa / den;
    // GeometrySmith
    const float nv = max0(dot3(N0, N1, N2, V0, V1, V2)), nl = max0(dot3(N0, N1, N2, L0, L1, L2));
    const float rr = roughness + 1.0f, kk = (rr * rr) / 8.0f;
    const float G = (nl / (nl * (1.0f - kk) + kk)) * (nv / (nv * (1.0f - kk) + kk));
    const float ng = NDF * G;
    const float denominator = (4.0f * nv) * nl + 0.0001f;
    const float s0 = (ng * F0) / denominator, s1 = (ng * F1) / denominator, s2 = (ng * F2) / denominator;
    const float kD0 = (1.0f - F0) * im, kD1 = (1.0f - F1) * im, kD2 = (1.0f - F2) * im;
    const float lit = 1.0f - shadow;
    // `kD * albedo / PI` with the macro: ((kD albedo) / 22) / 7
    const float Lo0 = ((((kD0 * a0) / 22.0f) / 7.0f + s0) * r0) * nl * lit;
    const float Lo1 = ((((kD1 * a1) / 22.0f) / 7.0f + s1) * r1) * nl * lit;
    const float Lo2 = ((((kD2 * a2) / 22.0f) / 7.0f + s2) * r2) * nl * lit;
    float c0 = 0.3f * a0 + Lo0, c1 = 0.3f * a1 + Lo1, c2 = 0.3f * a2 + Lo2;
    const float ig = 1.0f / 2.2f;
    c0 = pow_fast(c0 / (c0 + 1.0f), ig); c1 = pow_fast(c1 / (c1 + 1.0f), ig); c2 = pow_fast(c2 / (c2 + 1.0f), ig);
    auto q8 = [](float c) { return c == c ? (uint32_t)rintf(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f) : 0u; };
    frame[px] = q8(c0) | (q8(c1) << 8) | (q8(c2) << 16) | 0xFF000000u;
}

}  // namespace

// ---- host side ---------------------------------------------------------------------------------------------------------------
size_t shadow_temp_bytes(uint32_t n_words, uint32_t n_quads, uint32_t pairs) {
    size_t a = 0, b = 0, c = 0;
    (void)rocprim::exclusive_scan(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n_words, rocprim::plus<uint32_t>(), (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, b, (const uint32_t*)nullptr, (unsigned long long*)nullptr, 0ull, (size_t)n_quads,
                                  rocprim::plus<unsigned long long>(), (hipStream_t)0);
    (void)rocprim::radix_sort_pairs(nullptr, c, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, pairs, 0, 32,
                                    (hipStream_t)0);
    return std::max(a, std::max(b, c));
}

hipError_t shadow_count(const PrepassK& k, const float* views, const float light[3], const float4* rec, uint32_t n, uint32_t* cnt, uint32_t* off,
                        void* temp, size_t temp_bytes, uint32_t* bases, hipStream_t st) {
    const uint32_t nb = shadow_blocks(n);
    hipError_t e = hipMemsetAsync(cnt + 6ull * nb, 0, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_shadow_quads<false>, dim3(nb), dim3(256), 0, st, k, views, light[0], light[1], light[2], rec, n, nb, cnt, (const uint32_t*)nullptr,
                       (float4*)nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = rocprim::exclusive_scan(temp, temp_bytes, (const uint32_t*)cnt, off, 0u, (size_t)(6ull * nb + 1), rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_shadow_bases, dim3(1), dim3(64), 0, st, (const uint32_t*)off, nb, bases);
    return hipGetLastError();
}

hipError_t shadow_emit(const PrepassK& k, const float* views, const float light[3], const float4* rec, uint32_t n, const uint32_t* off, float4* quads,
                       hipStream_t st) {
    const uint32_t nb = shadow_blocks(n);
    hipLaunchKernelGGL(k_shadow_quads<true>, dim3(nb), dim3(256), 0, st, k, views, light[0], light[1], light[2], rec, n, nb, (uint32_t*)nullptr, off, quads);
    return hipGetLastError();
}

hipError_t shadow_setup(const float4* quads, uint32_t n, const ShadowBases& fb, int S, const float light[3], float far_plane, float4* rec, uint32_t* cnt,
                        unsigned long long* off, void* temp, size_t temp_bytes, unsigned long long* totals, hipStream_t st) {
    const int tiles_y = (S + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_shadow_setup, dim3((n + 255u) / 256u), dim3(256), 0, st, quads, n, fb, S, tiles_y, light[0], light[1], light[2], far_plane, rec, cnt,
                       totals + 1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(temp, temp_bytes, (const uint32_t*)cnt, off, 0ull, (size_t)n, rocprim::plus<unsigned long long>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_shadow_total, dim3(1), dim3(64), 0, st, (const unsigned long long*)off, (const uint32_t*)cnt, n, totals);
    return hipGetLastError();
}

hipError_t shadow_bin(const float4* rec, const uint32_t* cnt, const unsigned long long* off, uint32_t n, int S, uint32_t* keys_in, uint32_t* vals_in,
                      uint32_t* keys_out, uint32_t* vals_out, uint32_t pairs, void* temp, size_t temp_bytes, hipStream_t st) {
    const int tiles = (S + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_shadow_pairs, dim3((n + 255u) / 256u), dim3(256), 0, st, rec, cnt, off, n, tiles, keys_in, vals_in);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t n_tiles = 6u * (uint32_t)tiles * (uint32_t)tiles;
    int bits = 1;
    while ((1u << bits) < n_tiles) ++bits;
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, pairs, 0, bits, st);
}

hipError_t shadow_clear(float* cube, int S, hipStream_t st) {
    return hipMemsetD32Async((hipDeviceptr_t)cube, (int)kOne, 6ull * (size_t)S * (size_t)S, st);
}

hipError_t shadow_raster(const float4* rec, const uint32_t* keys, const uint32_t* vals, uint32_t pairs, int S, float* cube, unsigned long long* writes,
                         hipStream_t st) {
    const int tiles = (S + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_shadow_tiles, dim3((pairs + 255u) / 256u), dim3(256), 0, st, rec, keys, vals, pairs, S, tiles, tiles, (uint32_t*)cube, writes);
    return hipGetLastError();
}

hipError_t launch_relight(const RelightK& k, const void* const planes[5], const float* cube, uint32_t* frame, uint8_t* counts, hipStream_t st,
                          const void* const left_planes[5], int split_x, int div_x) {
    const size_t px = (size_t)k.W * (size_t)k.H;
    if (left_planes) {
        const RelightPlanes lp = { (const uint2*)left_planes[0], (const uint2*)left_planes[1], (const uint32_t*)left_planes[2], (const uint32_t*)left_planes[4] };
        hipLaunchKernelGGL(k_relight<true>, dim3((uint32_t)((px + 255u) / 256u)), dim3(256), 0, st, k, (const uint2*)planes[0], (const uint2*)planes[1],
                           (const uint32_t*)planes[2], (const uint32_t*)planes[4], cube, frame, counts, lp, split_x, div_x);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_relight<false>, dim3((uint32_t)((px + 255u) / 256u)), dim3(256), 0, st, k, (const uint2*)planes[0], (const uint2*)planes[1],
                       (const uint32_t*)planes[2], (const uint32_t*)planes[4], cube, frame, counts, RelightPlanes{ nullptr, nullptr, nullptr, nullptr }, 0, 0);
    return hipGetLastError();
}

hipError_t preload_light() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_relight<false>)); }

}  // namespace m2s
