// m2s_meshdepth.hip — the mesh depth prepass (DepthPrepass.cpp:8-50, depthPrepass{VS,PS}.glsl): the opaque meshes of the uploaded scene
// drawn depth-only, GL_LESS, through the frame's camera into the image the viewer prepass tests its Gaussians against
// (m2s_prepass_params.depth).  The semantics are the ones include/m2s.h pins (m2s_mesh_depth); tests/meshdepth_ref.py restates them in
// numpy.  A texel ends as min(1, min over covering fragments of z_w): order-independent and idempotent, so every kernel below may
// send its fragments in any order, as atomicMin on the depth bits (non-negative floats order as unsigned integers).
//
//   k_md_setup     one lane per triangle, reading the 36 B of position planes the upload left behind: mesh (opaque?), three clip
//                  positions, the finite test, trivial rejection, the clip decision.  An unclipped triangle is divided, snapped and boxed
//                  (raster_head_wh); one whose pixel box is at most kMdInplace x kMdInplace (4 x 4) pixels is covered IN PLACE by its
//                  lane — at most 16 centres, incremental int64 edges — and sends an atomic only where it is below a plain read.  Every
//                  other triangle that is still alive (larger box, or in need of the clipper) is appended to the deferred list.
//   k_md_deferred  one lane per deferred triangle: the same transform again (a few thousand triangles at most in any real view),
//                  Sutherland-Hodgman in LDS (two polygons of 8 vertices per lane; no scratch), the fan, and per piece a 48-byte record
//                  (snapped vertices, z_w, tile box) in one of the triangle's six slots, with its number of 16 x 16 tiles.
//   scan + k_md_pairs   exact number of (tile, piece) pairs; ONE WAVE per piece writes its pairs, 64 at a time (a floor that fills
//                  an 8192 x 8192 window has 262 144 of them: 4096 coalesced stores per lane, not one lane's loop — the limit DESIGN
//                  5.9 records for k_shadow_pairs).  rocPRIM radix sort over the tile-id bits.
//   k_md_tiles     k_shadow_tiles for triangles with a depth gradient: the sorted pair array cut into chunks of 256 whatever tiles they
//                  belong to, one thread stages one pair (exact int64 edge values at the tile's first pixel, m2s_quadraster.h), then one
//                  lane per texel: coverage with 32-bit products, barycentrics from the exact edge values, running min in a register,
//                  atomics only when the tile changes and only where the min is below a plain read.
//
// Every kernel that touches the image is a template over kVis.  false: the depth pass above, unchanged.  true: the visibility stage of
// the mesh render pass (m2s_mesh_render, m2s_meshrender.hip shades its result): every mesh, back faces culled, and the payload of a
// texel is the 64-bit key (bits of z) << 32 | global triangle index, so that the minimum is GL_LESS in draw order.
#include <type_traits>
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "m2s_devfn.h"
#include "m2s_quadraster.h"
#include "m2s_viewmath.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr int kTile = kSplatTile;
constexpr uint32_t kOne = 0x3F800000u;      // 1.0f: the clear value
constexpr unsigned long long kVisEmpty = ((unsigned long long)kOne << 32) | 0xFFFFFFFFull;     // the clear value of the visibility image

template <bool kVis> using Texel = std::conditional_t<kVis, unsigned long long, uint32_t>;

enum { kMdDead = 0, kMdUnclipped = 1, kMdClip = 2, kMdNonFinite = 3 };

// the five clip planes in the pinned order near, +x, -x, +y, -y: d >= 0 is inside (2 w is exact)
__device__ __forceinline__ float plane_d(int p, float4 c) {
    const float w2 = c.w + c.w;
    return p == 0 ? c.z + c.w : p == 1 ? w2 - c.x : p == 2 ? w2 + c.x : p == 3 ? w2 - c.y : w2 + c.y;
}

// The three clip positions of triangle t (gl_Position = PVM * (p, 1), one mat4 x vec4 per vertex) and what becomes of it.
__device__ __forceinline__ int md_classify(const MeshDepthK& k, const TriPlanes& tp, uint32_t t, float4 (&c)[3]) {
    float p[9];
    load_positions(tp, t, p);
#pragma unroll
    for (int v = 0; v < 3; ++v) c[v] = m4_mul(k.PVM, p[3 * v], p[3 * v + 1], p[3 * v + 2], 1.0f);
    if (!(finite4(c[0]) && finite4(c[1]) && finite4(c[2]))) return kMdNonFinite;
    bool any_out = false, dead = false;
#pragma unroll
    for (int pl = 0; pl < 5; ++pl) {
        const bool o0 = !(plane_d(pl, c[0]) >= 0.0f), o1 = !(plane_d(pl, c[1]) >= 0.0f), o2 = !(plane_d(pl, c[2]) >= 0.0f);
        any_out = any_out || o0 || o1 || o2;
        dead = dead || (o0 && o1 && o2);          // wholly outside one plane: the clipper would return nothing
    }
    return dead ? kMdDead : any_out ? kMdClip : kMdUnclipped;
}

// One triangle after clipping: perspective division, z_w, the far rejection, viewport + snap + box.  false: nothing to draw.
// kCull (GL_CULL_FACE, front = CCW): a piece whose snapped vertices in their STORED order have a doubled area <= 0 (window with y up)
// is not drawn; *back = it was rejected for a negative one.
template <bool kCull>
__device__ __forceinline__ bool md_piece(const MeshDepthK& k, float4 c0, float4 c1, float4 c2, RasterHead& h, float (&zw)[3], bool* back = nullptr) {
    const float4 c[3] = { c0, c1, c2 };
    float nx[3], ny[3];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        nx[v] = c[v].x / c[v].w;
        ny[v] = c[v].y / c[v].w;
        zw[v] = (c[v].z / c[v].w) * 0.5f + 0.5f;
    }
    if (!(zw[0] < 1.0f || zw[1] < 1.0f || zw[2] < 1.0f)) return false;     // cannot pass GL_LESS against the clear value (or NaN)
    if (!raster_head_wh(nx, ny, k.W, k.H, h)) return false;
    if constexpr (kCull) {
        const long long stored = tri_area2(h.X, h.Y);
        if (stored <= 0) { if (stored < 0) *back = true; return false; }
    }
    // canonical vertex order — ascending (Y, X) of the snapped coordinates — so that neither the winding nor the order in which a
    // triangle's vertices are stored changes a bit of the interpolated depth (coverage never depended on it)
    auto cswap = [&](int i, int j) {
        const long long ki = (long long)h.Y[i] * (1ll << 32) + h.X[i], kj = (long long)h.Y[j] * (1ll << 32) + h.X[j];
        if (kj < ki) {
            const int tx = h.X[i], ty = h.Y[i];
            const float tz = zw[i];
            h.X[i] = h.X[j]; h.Y[i] = h.Y[j]; zw[i] = zw[j];
            h.X[j] = tx; h.Y[j] = ty; zw[j] = tz;
        }
    };
    cswap(0, 1); cswap(1, 2); cswap(0, 1);
    return tri_area2(h.X, h.Y) != 0;
}

__device__ __forceinline__ float md_clamp(float z) { return z < 0.0f ? 0.0f : z > 1.0f ? 1.0f : z; }    // (NaN stays NaN: never passes)

__device__ __forceinline__ uint64_t wave_count(bool b) { return (uint64_t)__popcll(__ballot(b)); }

template <bool kVis>
__global__ void __launch_bounds__(256) k_md_setup(const MeshDepthK k, const SceneDev sc, Texel<kVis>* __restrict__ image, uint32_t* __restrict__ deferred,
                                                  unsigned long long* __restrict__ totals) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int cls = kMdDead;
    bool defer = false, drawn = false, back = false;
    uint32_t sent = 0;
    if (t < sc.n_tri) {
        bool draw = true;                                       // (the mesh render pass draws every mesh)
        if constexpr (!kVis) {
            const uint2 mo = sc.mesh_of8[t >> 3];
            const uint32_t mesh = t < mo.y ? mo.x : find_mesh(sc, sc.tri_first + t);
            draw = sc.meshes[mesh].color[3] == 1.0f;            // DepthPrepass.cpp:33
        }
        if (draw) {
            float4 c[3];
            cls = md_classify(k, sc.tri, t, c);
            if (cls == kMdClip) defer = true;
            else if (cls == kMdUnclipped) {
                RasterHead h;
                float zw[3];
                if (md_piece<kVis>(k, c[0], c[1], c[2], h, zw, &back)) {
                    if (h.x1 - h.x0 < k.inplace && h.y1 - h.y0 < k.inplace) {
                        drawn = true;
                        const long long area2 = tri_area2(h.X, h.Y);
                        const int sgn = area2 < 0 ? -1 : 1;
                        const float inva = 1.0f / i64_to_f32(area2 < 0 ? -area2 : area2);
                        int a[3], b[3], bias[3];
                        long long e[3];
#pragma unroll
                        for (int i = 0; i < 3; ++i) tile_edge(h.X, h.Y, i, sgn, h.x0, h.y0, a[i], b[i], e[i], bias[i]);
                        for (int y = h.y0; y <= h.y1; ++y) {
                            long long r0 = e[0], r1 = e[1], r2 = e[2];
                            for (int x = h.x0; x <= h.x1; ++x) {
                                if (r0 + bias[0] > 0 && r1 + bias[1] > 0 && r2 + bias[2] > 0) {
                                    const float b0 = i64_to_f32(r0) * inva, b1 = i64_to_f32(r1) * inva, b2 = i64_to_f32(r2) * inva;
                                    const float z = md_clamp((b0 * zw[0] + b1 * zw[1]) + b2 * zw[2]);
                                    if (z < 1.0f) {
                                        Texel<kVis>* px = image + (size_t)y * (size_t)k.W + (size_t)x;
                                        Texel<kVis> bits = __float_as_uint(z);
                                        if constexpr (kVis) bits = (bits << 32) | (unsigned long long)(sc.tri_first + t);
                                        if (bits < *px) { atomicMin(px, bits); ++sent; }
                                    }
                                }
                                r0 += 256ll * a[0]; r1 += 256ll * a[1]; r2 += 256ll * a[2];
                            }
                            e[0] += 256ll * b[0]; e[1] += 256ll * b[1]; e[2] += 256ll * b[2];
                        }
                    } else defer = true;
                }
            }
        }
    }
    const unsigned long long dm = __ballot(defer);
    if (dm) {
        uint32_t base = 0;
        const int leader = __ffsll((long long)dm) - 1;
        if (lane == leader) base = (uint32_t)atomicAdd(totals + 5, (unsigned long long)__popcll(dm));
        base = __shfl(base, leader);
        if (defer) deferred[base + (uint32_t)__popcll(dm & ((1ull << lane) - 1ull))] = t;
    }
    const uint64_t n_drawn = wave_count(drawn), n_bad = wave_count(cls == kMdNonFinite);
    uint32_t s = sent;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
        if (n_drawn) atomicAdd(totals + 0, (unsigned long long)n_drawn);
        if (n_bad) atomicAdd(totals + 2, (unsigned long long)n_bad);
        if (s) atomicAdd(totals + 4, (unsigned long long)s);
    }
    if constexpr (kVis) {
        const uint64_t n_back = wave_count(back);
        if (lane == 0 && n_back) atomicAdd(totals + 6, (unsigned long long)n_back);
    }
}

// The 48-byte record of one piece (3 x float4): [0] X[3], Y[0]; [1] Y[1], Y[2], z_w[0], z_w[1]; [2] z_w[2], tile box (tx0 | ty0 << 16),
// (tx1 | ty1 << 16), the triangle's global index (visibility stage only).  Slot 6 j + i holds piece i of deferred triangle j; cnt = its tiles (0: no piece).
constexpr int kMdSlots = 6;      // a triangle clipped by five planes has at most 8 vertices: a fan of 6

template <bool kVis>
__global__ void __launch_bounds__(64) k_md_deferred(const MeshDepthK k, const SceneDev sc, const uint32_t* __restrict__ deferred, uint32_t nd,
                                                    float4* __restrict__ rec, uint32_t* __restrict__ cnt, unsigned long long* __restrict__ totals) {
    __shared__ float4 poly[2][8][64];
    const int lane = threadIdx.x;
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    bool clipped = false, drawn = false, back = false;
    if (j < nd) {
        const uint32_t t = deferred[j];
        float4 c[3];
        const int cls = md_classify(k, sc.tri, t, c);
        int n = 3, cur = 0;
        poly[0][0][lane] = c[0]; poly[0][1][lane] = c[1]; poly[0][2][lane] = c[2];
        if (cls == kMdClip) {
            clipped = true;
            for (int pl = 0; pl < 5 && n >= 3; ++pl) {
                int m = 0;
                float4 a = poly[cur][0][lane];
                float da = plane_d(pl, a);
                for (int i = 0; i < n; ++i) {
                    const float4 b = poly[cur][i + 1 == n ? 0 : i + 1][lane];
                    const float db = plane_d(pl, b);
                    const bool ain = da >= 0.0f, bin = db >= 0.0f;
                    if (ain && m < 8) poly[cur ^ 1][m++][lane] = a;
                    if (ain != bin && m < 8) {        // (a convex polygon never gets there; rounding must not be able to overrun the array)
                        const float4 vi = ain ? a : b, vo = ain ? b : a;          // from the inside vertex: the same point from either side of a shared edge
                        const float di = ain ? da : db, dout = ain ? db : da;
                        const float tt = di / (di - dout);
                        poly[cur ^ 1][m++][lane] = make_float4(vi.x + tt * (vo.x - vi.x), vi.y + tt * (vo.y - vi.y), vi.z + tt * (vo.z - vi.z), vi.w + tt * (vo.w - vi.w));
                    }
                    a = b; da = db;
                }
                n = m;
                cur ^= 1;
            }
            if (n < 3) n = 0;
        }
        const float4 v0 = poly[cur][0][lane];
        for (int i = 0; i < kMdSlots; ++i) {
            uint32_t tiles = 0;
            if (i + 2 < n) {
                RasterHead h;
                float zw[3];
                if (md_piece<kVis>(k, v0, poly[cur][i + 1][lane], poly[cur][i + 2][lane], h, zw, &back)) {
                    drawn = true;
                    const int t0x = h.x0 / kTile, t1x = h.x1 / kTile, t0y = h.y0 / kTile, t1y = h.y1 / kTile;
                    tiles = (uint32_t)(t1x - t0x + 1) * (uint32_t)(t1y - t0y + 1);
                    float4* o = rec + 3ull * ((size_t)j * kMdSlots + i);
                    o[0] = make_float4(__int_as_float(h.X[0]), __int_as_float(h.X[1]), __int_as_float(h.X[2]), __int_as_float(h.Y[0]));
                    o[1] = make_float4(__int_as_float(h.Y[1]), __int_as_float(h.Y[2]), zw[0], zw[1]);
                    o[2] = make_float4(zw[2], __uint_as_float((uint32_t)t0x | ((uint32_t)t0y << 16)), __uint_as_float((uint32_t)t1x | ((uint32_t)t1y << 16)),
                                       kVis ? __uint_as_float(sc.tri_first + t) : 0.0f);
                }
            }
            cnt[(size_t)j * kMdSlots + i] = tiles;
        }
    }
    const uint64_t n_drawn = wave_count(drawn), n_clip = wave_count(clipped);
    if (lane == 0) {
        if (n_drawn) atomicAdd(totals + 0, (unsigned long long)n_drawn);
        if (n_clip) atomicAdd(totals + 1, (unsigned long long)n_clip);
    }
    if constexpr (kVis) {        // culled: a piece was back-facing and none was drawn
        const uint64_t n_back = wave_count(back && !drawn);
        if (lane == 0 && n_back) atomicAdd(totals + 6, (unsigned long long)n_back);
    }
}

__global__ void k_md_total(const unsigned long long* __restrict__ off, const uint32_t* __restrict__ cnt, uint32_t n, unsigned long long* __restrict__ totals) {
    if (threadIdx.x == 0 && blockIdx.x == 0) totals[3] = off[n - 1] + cnt[n - 1];
}

// one wave per slot
__global__ void __launch_bounds__(256) k_md_pairs(const float4* __restrict__ rec, const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ off,
                                                  uint32_t n_slots, int tiles_x, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (s >= n_slots) return;
    const uint32_t c = cnt[s];
    if (c == 0) return;
    const float4 r2 = rec[3ull * s + 2];
    emit_tile_pairs_wave(__float_as_uint(r2.y), __float_as_uint(r2.z), tiles_x, c, (size_t)off[s], s, threadIdx.x & 63, keys, vals);
}

struct __align__(16) StagedTri {
    int4 ea, eb;            // a[0..2], T[0];  b[0..2], T[1]
    int4 m;                 // T[2], covered by the tile's box (0 / 1), tile key, bits of 1 / area2
    float4 z;               // z_w[0..2]
    long long E[3];         // edge values at the centre of the tile's first pixel
    long long tri;          // visibility stage: the triangle's global index
};

template <bool kVis>
__global__ void __launch_bounds__(256) k_md_tiles(const float4* __restrict__ rec, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                  uint32_t pairs, int W, int H, int tiles_x, Texel<kVis>* __restrict__ image,
                                                  unsigned long long* __restrict__ totals) {
    __shared__ StagedTri sq[256];
    __shared__ uint32_t wg_writes;
    const int tid = threadIdx.x;
    const int lx = tid & (kTile - 1), ly = tid / kTile;
    const uint32_t base = blockIdx.x * 256u;
    const uint32_t m = min(256u, pairs - base);
    if (tid == 0) wg_writes = 0;
    if ((uint32_t)tid < m) {
        const uint32_t key = keys[base + tid], slot = vals[base + tid];
        const float4* r = rec + 3ull * slot;
        const float4 r0 = r[0], r1 = r[1], r2 = r[2];
        const int X[3] = { __float_as_int(r0.x), __float_as_int(r0.y), __float_as_int(r0.z) };
        const int Y[3] = { __float_as_int(r0.w), __float_as_int(r1.x), __float_as_int(r1.y) };
        const int px0 = (int)(key % (uint32_t)tiles_x) * kTile, py0 = (int)(key / (uint32_t)tiles_x) * kTile;
        StagedTri s;
        s.ea = s.eb = make_int4(0, 0, 0, kTMax);
        s.E[0] = s.E[1] = s.E[2] = 0;
        s.tri = kVis ? (long long)__float_as_uint(r2.w) : 0;
        int t2 = kTMax;
        uint32_t waves = 0;
        const bool meets = box_meets_tile(X, Y, W, H, px0, py0, &waves);
        if (meets) stage_triangle(X, Y, px0, py0, s.ea, s.eb, t2, s.E);
        const long long area2 = tri_area2(X, Y);
        const float inva = 1.0f / i64_to_f32(area2 < 0 ? -area2 : area2);
        s.m = make_int4(t2, meets ? 1 : 0, (int)key, __float_as_int(inva));
        s.z = make_float4(r1.z, r1.w, r2.x, 0.0f);
        sq[tid] = s;
    }
    __syncthreads();
    uint32_t sent = 0;
    // the running minimum of a texel: the depth, or (visibility stage) the whole 64-bit key; both start at the clear value
    using Min = std::conditional_t<kVis, unsigned long long, float>;
    constexpr Min kClear = kVis ? (Min)kVisEmpty : (Min)1.0f;
    auto flush = [&](uint32_t key, Min zmin) {
        const int x = (int)(key % (uint32_t)tiles_x) * kTile + lx, y = (int)(key / (uint32_t)tiles_x) * kTile + ly;
        if (x < W && y < H && zmin < kClear) {
            Texel<kVis>* p = image + (size_t)y * (size_t)W + (size_t)x;
            Texel<kVis> bits;
            if constexpr (kVis) bits = zmin; else bits = __float_as_uint(zmin);
            // (the plain read races with other workgroups' atomicMin on this texel; a texel only ever decreases, so a stale value is
            //  at least the current one: it can cause a redundant atomic, never a missed one)
            if (bits < *p) { atomicMin(p, bits); ++sent; }
        }
    };
    uint32_t cur = (uint32_t)sq[0].m.z;
    Min zmin = kClear;
    for (uint32_t e = 0; e < m; ++e) {
        const int4 mm = sq[e].m;
        if ((uint32_t)mm.z != cur) { flush(cur, zmin); cur = (uint32_t)mm.z; zmin = kClear; }     // (workgroup-uniform)
        if (!mm.y) continue;
        const int4 a = sq[e].ea, b = sq[e].eb;
        const int s0 = a.x * lx + b.x * ly, s1 = a.y * lx + b.y * ly, s2 = a.z * lx + b.z * ly;
        if ((s0 > a.w) & (s1 > b.w) & (s2 > mm.x)) {
            const float inva = __int_as_float(mm.w);
            const float4 z = sq[e].z;
            const float b0 = i64_to_f32(sq[e].E[0] + 256ll * s0) * inva, b1 = i64_to_f32(sq[e].E[1] + 256ll * s1) * inva,
                        b2 = i64_to_f32(sq[e].E[2] + 256ll * s2) * inva;
            const float zz = md_clamp((b0 * z.x + b1 * z.y) + b2 * z.z);
            if constexpr (kVis) {
                const unsigned long long kk = ((unsigned long long)__float_as_uint(zz) << 32) | (unsigned long long)sq[e].tri;
                if (zz < 1.0f && kk < zmin) zmin = kk;
            } else if (zz < zmin) zmin = zz;
        }
    }
    flush(cur, zmin);
    if (sent) atomicAdd(&wg_writes, sent);
    __syncthreads();
    if (tid == 0 && wg_writes) atomicAdd(totals + 4, (unsigned long long)wg_writes);
}

__global__ void __launch_bounds__(256) k_mv_clear(unsigned long long* __restrict__ image, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) image[i] = kVisEmpty;
}

}  // namespace

// ---- host side ---------------------------------------------------------------------------------------------------------------
size_t meshdepth_temp_bytes(uint32_t n_slots, uint32_t pairs) {
    size_t a = 0, b = 0;
    (void)rocprim::exclusive_scan(nullptr, a, (const uint32_t*)nullptr, (unsigned long long*)nullptr, 0ull, (size_t)n_slots,
                                  rocprim::plus<unsigned long long>(), (hipStream_t)0);
    (void)rocprim::radix_sort_pairs(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, pairs, 0, 32,
                                    (hipStream_t)0);
    return std::max(a, b);
}

hipError_t meshdepth_clear(float* image, int W, int H, hipStream_t st) {
    return hipMemsetD32Async((hipDeviceptr_t)image, (int)kOne, (size_t)W * (size_t)H, st);
}

hipError_t meshdepth_setup(const MeshDepthK& k, const SceneDev& sc, float* image, uint32_t* deferred, unsigned long long* totals, hipStream_t st) {
    hipLaunchKernelGGL(k_md_setup<false>, dim3((sc.n_tri + 255u) / 256u), dim3(256), 0, st, k, sc, (uint32_t*)image, deferred, totals);
    return hipGetLastError();
}

hipError_t meshvis_clear(unsigned long long* image, int W, int H, hipStream_t st) {
    const size_t n = (size_t)W * (size_t)H;
    hipLaunchKernelGGL(k_mv_clear, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, st, image, n);
    return hipGetLastError();
}

hipError_t meshvis_setup(const MeshDepthK& k, const SceneDev& sc, unsigned long long* image, uint32_t* deferred, unsigned long long* totals, hipStream_t st) {
    hipLaunchKernelGGL(k_md_setup<true>, dim3((sc.n_tri + 255u) / 256u), dim3(256), 0, st, k, sc, image, deferred, totals);
    return hipGetLastError();
}

hipError_t meshdepth_deferred(const MeshDepthK& k, const SceneDev& sc, const uint32_t* deferred, uint32_t nd, float4* rec, uint32_t* cnt,
                              unsigned long long* off, void* temp, size_t temp_bytes, unsigned long long* totals, hipStream_t st, bool vis) {
    if (vis) hipLaunchKernelGGL(k_md_deferred<true>, dim3((nd + 63u) / 64u), dim3(64), 0, st, k, sc, deferred, nd, rec, cnt, totals);
    else hipLaunchKernelGGL(k_md_deferred<false>, dim3((nd + 63u) / 64u), dim3(64), 0, st, k, sc, deferred, nd, rec, cnt, totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t slots = nd * (uint32_t)kMdSlots;
    e = rocprim::exclusive_scan(temp, temp_bytes, (const uint32_t*)cnt, off, 0ull, (size_t)slots, rocprim::plus<unsigned long long>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_md_total, dim3(1), dim3(64), 0, st, (const unsigned long long*)off, (const uint32_t*)cnt, slots, totals);
    return hipGetLastError();
}

hipError_t meshdepth_bin(const MeshDepthK& k, const float4* rec, const uint32_t* cnt, const unsigned long long* off, uint32_t nd, uint32_t* keys_in,
                         uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out, uint32_t pairs, void* temp, size_t temp_bytes, hipStream_t st) {
    const int tiles_x = (k.W + kTile - 1) / kTile, tiles_y = (k.H + kTile - 1) / kTile;
    const uint32_t slots = nd * (uint32_t)kMdSlots;
    hipLaunchKernelGGL(k_md_pairs, dim3((slots + 3u) / 4u), dim3(256), 0, st, rec, cnt, off, slots, tiles_x, keys_in, vals_in);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t n_tiles = (uint32_t)tiles_x * (uint32_t)tiles_y;
    int bits = 1;
    while ((1u << bits) < n_tiles) ++bits;
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, pairs, 0, bits, st);
}

hipError_t meshdepth_raster(const MeshDepthK& k, const float4* rec, const uint32_t* keys, const uint32_t* vals, uint32_t pairs, float* image,
                            unsigned long long* totals, hipStream_t st) {
    const int tiles_x = (k.W + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_md_tiles<false>, dim3((pairs + 255u) / 256u), dim3(256), 0, st, rec, keys, vals, pairs, k.W, k.H, tiles_x, (uint32_t*)image, totals);
    return hipGetLastError();
}

hipError_t meshvis_raster(const MeshDepthK& k, const float4* rec, const uint32_t* keys, const uint32_t* vals, uint32_t pairs, unsigned long long* image,
                          unsigned long long* totals, hipStream_t st) {
    const int tiles_x = (k.W + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_md_tiles<true>, dim3((pairs + 255u) / 256u), dim3(256), 0, st, rec, keys, vals, pairs, k.W, k.H, tiles_x, image, totals);
    return hipGetLastError();
}

hipError_t preload_meshdepth() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_md_setup<false>)); }

}  // namespace m2s
