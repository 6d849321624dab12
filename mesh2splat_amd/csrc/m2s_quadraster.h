// m2s_quadraster.h — what the passes that rasterise per 16 x 16 tile share (m2s_splat.hip: the splat pass into the G-buffer;
// m2s_light.hip: the shadow pass into the depth cube; m2s_meshdepth.hip: the mesh depth prepass, triangles instead of quads): the quad's four vertices in the pinned order and rounding, and the per-tile
// form of the pinned rasteriser (raster_setup_wh, m2s_devfn.h) — exact int64 edge arithmetic once per (triangle, 16 x 16 tile), after
// which the 256 lanes of the tile test coverage with 32-bit products.  One definition, so that both passes cover the same pixels.
#pragma once
#include "m2s_device.h"
#include "m2s_devfn.h"

#pragma clang fp contract(off)

namespace m2s {

constexpr int kTMax = 1 << 30;             // edge thresholds are clamped to +-2^30 (|a lx + b ly| < 2^28)

__device__ __forceinline__ bool finite4(float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w); }

// Quad vertex v of the pinned order (vx, vy) in {(-1,-1), (-1,1), (1,1), (1,-1)}: mean.xy + (vx * scale.xy + vy * scale.zw)
// (gaussianSplattingVS.glsl:33); multiplying by +-1 is exact, so the sum of the two axis terms and the mean's addition round.
__device__ __forceinline__ void quad_vertex(float4 m, float4 s, int v, float& x, float& y) {
    const float vx = (v == 0 || v == 1) ? -1.0f : 1.0f, vy = (v == 0 || v == 3) ? -1.0f : 1.0f;
    x = m.x + (vx * s.x + vy * s.z);
    y = m.y + (vx * s.y + vy * s.w);
}

constexpr uint32_t kQuadTri0 = 1u, kQuadTri1 = 2u;     // bits of QuadBox::flags (and of a quad's record): the triangle has pixels to cover

// What the setup kernel of either pass derives from one quad's mean and axes on a W x H viewport: the four snapped vertices (24.8), the
// skip decision (a non-finite field — `fin` is the caller's test of the fields its pass reads — or a vertex beyond the guard band),
// which of the two triangles (0,1,2), (0,2,3) has a non-empty raster setup, and the union of their pixel boxes.
struct QuadBox {
    int X[4], Y[4];
    bool skip;
    uint32_t flags;
    int x0, x1, y0, y1;     // inclusive pixel box, clamped to the viewport (x0 > x1: empty)
};
__device__ __forceinline__ void quad_snap_box(float4 m, float4 s, bool fin, int W, int H, QuadBox& b) {
    float vx[4], vy[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) quad_vertex(m, s, v, vx[v], vy[v]);
    const float hw = (float)W * 0.5f, hh = (float)H * 0.5f;
    bool guard = true;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const float xw = hw * vx[v] + hw, yw = hh * vy[v] + hh;
        guard = guard && (fabsf(xw) < kGuardPx) && (fabsf(yw) < kGuardPx);
        b.X[v] = (int)rintf(xw * 256.0f);
        b.Y[v] = (int)rintf(yw * 256.0f);
    }
    b.skip = !(fin && guard);
    b.flags = 0;
    b.x0 = W; b.x1 = -1; b.y0 = H; b.y1 = -1;
    if (!b.skip) {
        const float tx0[3] = { vx[0], vx[1], vx[2] }, ty0[3] = { vy[0], vy[1], vy[2] };
        const float tx1[3] = { vx[0], vx[2], vx[3] }, ty1[3] = { vy[0], vy[2], vy[3] };
        Raster r;
        if (raster_setup_wh(tx0, ty0, W, H, r)) { b.flags |= kQuadTri0; b.x0 = min(b.x0, r.x0); b.x1 = max(b.x1, r.x1); b.y0 = min(b.y0, r.y0); b.y1 = max(b.y1, r.y1); }
        if (raster_setup_wh(tx1, ty1, W, H, r)) { b.flags |= kQuadTri1; b.x0 = min(b.x0, r.x0); b.x1 = max(b.x1, r.x1); b.y0 = min(b.y0, r.y0); b.y1 = max(b.y1, r.y1); }
    }
}
// The box in 16 x 16 tiles, packed (tx | ty << 16) for the first and the last tile, tile rows shifted by row_base (the shadow pass's atlas
// of six faces); -> the number of tiles = (tile, quad) pairs of the quad
__device__ __forceinline__ uint32_t quad_tile_box(const QuadBox& b, int row_base, uint32_t& tb0, uint32_t& tb1) {
    const int t0x = b.x0 / kSplatTile, t1x = b.x1 / kSplatTile, t0y = b.y0 / kSplatTile + row_base, t1y = b.y1 / kSplatTile + row_base;
    tb0 = (uint32_t)t0x | ((uint32_t)t0y << 16);
    tb1 = (uint32_t)t1x | ((uint32_t)t1y << 16);
    return (uint32_t)(t1x - t0x + 1) * (uint32_t)(t1y - t0y + 1);
}
// The pairs of quad i, row-major over its tile box, from position k on: key = tile id (row * tiles_x + column), value = the quad
__device__ __forceinline__ void emit_tile_pairs(uint32_t tb0, uint32_t tb1, int tiles_x, size_t k, uint32_t i, uint32_t* __restrict__ keys,
                                                uint32_t* __restrict__ vals) {
    const int t0x = tb0 & 0xFFFF, t0y = tb0 >> 16, t1x = tb1 & 0xFFFF, t1y = tb1 >> 16;
    for (int ty = t0y; ty <= t1y; ++ty)
        for (int tx = t0x; tx <= t1x; ++tx) {
            keys[k] = (uint32_t)(ty * tiles_x + tx);
            vals[k] = i;
            ++k;
        }
}

// The same pairs written by the 64 lanes of one wave, 64 consecutive pairs per step: `count` = tiles of the box
__device__ __forceinline__ void emit_tile_pairs_wave(uint32_t tb0, uint32_t tb1, int tiles_x, uint32_t count, size_t k, uint32_t i, int lane,
                                                     uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t t0x = tb0 & 0xFFFF, t0y = tb0 >> 16, bw = (tb1 & 0xFFFF) - t0x + 1u;
    for (uint32_t j = (uint32_t)lane; j < count; j += 64u) {
        const uint32_t ry = j / bw, rx = j - ry * bw;
        keys[k + j] = (t0y + ry) * (uint32_t)tiles_x + t0x + rx;
        vals[k + j] = i;
    }
}

// Edge i (opposite vertex i) of the triangle with doubled signed area `area2`, oriented so that the interior is positive: its
// coefficients a, b (E_i(P) = a Px + b Py + c), its value e at the centre of pixel (px0, py0) — P = 256 (x, y) + 128 — and the
// top-left rule's bias (1: the edge's own boundary is inside).  int64, exact: raster_setup_wh's integers.
__device__ __forceinline__ void tile_edge(const int X[3], const int Y[3], int i, int sgn, int px0, int py0, int& a, int& b, long long& e, int& bias) {
    const int ia = (i + 1) % 3, ib = (i + 2) % 3;
    const int dy = Y[ib] - Y[ia], dx = X[ib] - X[ia];
    a = -dy * sgn;
    b = dx * sgn;
    const long long c = ((long long)dy * X[ia] - (long long)dx * Y[ia]) * sgn;
    bias = (a > 0 || (a == 0 && b > 0)) ? 1 : 0;
    e = (long long)a * (256ll * px0 + 128) + (long long)b * (256ll * py0 + 128) + c;
}
__device__ __forceinline__ long long tri_area2(const int X[3], const int Y[3]) {
    return (long long)(X[1] - X[0]) * (Y[2] - Y[0]) - (long long)(Y[1] - Y[0]) * (X[2] - X[0]);
}

// One triangle's edge thresholds for the tile whose first pixel is (px0, py0): pixel (px0 + lx, py0 + ly) is inside edge i iff
// a_i lx + b_i ly > T_i, with E_i(P) = a_i Px + b_i Py + c_i at the pixel centre P = 256 (x, y) + 128 and the top-left rule's bias:
// E + bias > 0  <=>  256 (a lx + b ly) > -(E_org + bias)  <=>  a lx + b ly > floor(-(E_org + bias) / 256).
// E_org (or nullptr): the three edge values at the centre of the tile's first pixel, without the bias — what a pass that interpolates
// over the triangle (the mesh depth pass) builds its barycentrics from: E_i(lx, ly) = E_org[i] + 256 (a_i lx + b_i ly).
__device__ __forceinline__ void stage_triangle(const int X[3], const int Y[3], int px0, int py0, int4& ea, int4& eb, int& t2, long long* E_org = nullptr) {
    const long long area2 = tri_area2(X, Y);
    const int sgn = area2 < 0 ? -1 : 1;
    int a[3], b[3], T[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        int bias;
        long long e0;
        tile_edge(X, Y, i, sgn, px0, py0, a[i], b[i], e0, bias);
        if (E_org) E_org[i] = e0;
        const long long e = e0 + bias;
        long long t = (-e) >> 8;                      // floor(-e / 256)
        t = t < -(long long)kTMax ? -(long long)kTMax : t > (long long)kTMax ? (long long)kTMax : t;
        T[i] = (int)t;
    }
    ea = make_int4(a[0], a[1], a[2], T[0]);
    eb = make_int4(b[0], b[1], b[2], T[1]);
    t2 = T[2];
}

// Does the triangle's pixel box (as raster_head_wh clamps it) meet the tile [px0, px0 + 15] x [py0, py0 + 15]?  If so, the waves
// whose rows it reaches (wave w holds rows 4w .. 4w + 3 of the tile) as bits 0..3 of *waves.
__device__ __forceinline__ bool box_meets_tile(const int X[3], const int Y[3], int W, int H, int px0, int py0, uint32_t* waves) {
    const int xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
    const int ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
    const int x0 = max((xmin - 128 + 255) >> 8, 0), x1 = min((xmax - 128) >> 8, W - 1);
    const int y0 = max((ymin - 128 + 255) >> 8, 0), y1 = min((ymax - 128) >> 8, H - 1);
    if (!(x0 <= x1 && y0 <= y1 && x0 <= px0 + kSplatTile - 1 && x1 >= px0 && y0 <= py0 + kSplatTile - 1 && y1 >= py0)) return false;
    const int w0 = (max(y0, py0) - py0) >> 2, w1 = (min(y1, py0 + kSplatTile - 1) - py0) >> 2;
    *waves |= ((2u << w1) - 1u) & ~((1u << w0) - 1u);
    return true;
}

}  // namespace m2s
