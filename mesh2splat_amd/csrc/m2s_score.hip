// m2s_score.hip — the fidelity score (m2s_score_frames): image B (the splats) against image A (the mesh) in ONE pass over the frames
// and their coverage planes.  The pin is in include/m2s.h; tests/score_ref.py restates it.  Everything is integer arithmetic except one
// fp64 division per SSIM window, so every output is a sum / count / maximum of integers and does not depend on the reduction's order.
//
//   k_score   one workgroup per tile of 16 x 16 cells (64 x 64 pixels), one lane per 4 x 4 CELL of the tile's 17 x 17 grid (the extra
//             column and row are the halo: the cells to the right of and above the tile, which the windows starting in the tile's last
//             column / row need; a halo cell is some neighbour's own cell, so its 64 pixels are loaded twice — by two workgroups that
//             are usually resident together; 289 / 256 = 1.13 loads per byte, one of them expected from L2).
//             Per cell: four 16-byte row loads per image (four uchar4 = one uint4) -> the cell's five sums: sum Ya, sum Yb,
//             sum Ya^2 + Yb^2, sum Ya Yb, pixels that pass the mask.  Own cells also gather the colour figures and the coverage counts
//             and write the error map.  The five sums go through LDS; the lane of an own cell then adds 2 x 2 cells to one 8 x 8 window.
//             Reduction: wave (shuffles) -> workgroup (LDS integer atomics, one per wave and counter) -> one 64-bit integer atomic per
//             counter and workgroup into shard blockIdx % 32 of the accumulators (max_abs: atomicMax); zero contributions are skipped.
#include <hip/hip_runtime.h>

#include "m2s_device.h"

namespace m2s {
namespace {

constexpr int kCells = kScoreGridCells * kScoreGridCells;       // 289

// four pixels of a row starting at pixel `idx`; nx of them exist (kVec: nx == 4 and the address is 16-byte aligned)
template <bool kVec>
__device__ __forceinline__ uint4 load_row(const uint32_t* __restrict__ img, size_t idx, int nx) {
    if constexpr (kVec) {
        return *reinterpret_cast<const uint4*>(img + idx);
    } else {
        uint4 v = { 0u, 0u, 0u, 0u };
        v.x = img[idx];                                          // (nx >= 1: the cell starts inside the image)
        if (nx > 1) v.y = img[idx + 1];
        if (nx > 2) v.z = img[idx + 2];
        if (nx > 3) v.w = img[idx + 3];
        return v;
    }
}

__device__ __forceinline__ uint32_t luma(uint32_t p) {
    return (77u * (p & 255u) + 150u * ((p >> 8) & 255u) + 29u * ((p >> 16) & 255u) + 128u) >> 8;
}

__device__ __forceinline__ uint32_t absdiff8(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}
__device__ __forceinline__ long long wave_sum64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool kVec, bool kCover>
__global__ void __launch_bounds__(kScoreThreads) k_score(const ScoreK k, const uint32_t* __restrict__ A, const uint32_t* __restrict__ B,
                                                         const uint32_t* __restrict__ CA, const uint32_t* __restrict__ CB,
                                                         uint32_t* __restrict__ map, unsigned long long* __restrict__ acc) {
    __shared__ uint32_t s_cell[5][kCells];                      // per cell: s1, s2, ssq, s12, pixels that pass
    __shared__ unsigned long long s_acc[kScoreCounters];
    const int tid = (int)threadIdx.x;
    if (tid < kScoreCounters) s_acc[tid] = 0ull;
    const int lx = tid % kScoreGridCells, ly = tid / kScoreGridCells;
    const int tile_x = (int)(blockIdx.x % k.tiles_x), tile_y = (int)(blockIdx.x / k.tiles_x);
    const int x0 = 4 * (tile_x * kScoreTileCells + lx), y0 = 4 * (tile_y * kScoreTileCells + ly);
    const bool in_grid = tid < kCells;
    const bool own = in_grid && lx < kScoreTileCells && ly < kScoreTileCells;
    const bool inside = in_grid && x0 < k.W && y0 < k.H;
    const int nx = inside ? min(4, k.W - x0) : 0, ny = inside ? min(4, k.H - y0) : 0;
    // a halo cell matters only to windows, and a window takes whole cells only
    const bool work = inside && (own || (nx == 4 && ny == 4));

    uint32_t s1 = 0, s2 = 0, ssq = 0, s12 = 0, pass = 0;
    uint32_t cov0 = 0, cov1 = 0, cov2 = 0, cov3 = 0;
    uint32_t sse0 = 0, sse1 = 0, sse2 = 0, sad0 = 0, sad1 = 0, sad2 = 0, mx0 = 0, mx1 = 0, mx2 = 0;
    if (work) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r < ny) {
                const size_t idx = (size_t)(y0 + r) * (size_t)k.W + (size_t)x0;
                const uint4 va = load_row<kVec>(A, idx, nx), vb = load_row<kVec>(B, idx, nx);
                uint4 ca = { 0u, 0u, 0u, 0u }, cb = { 0u, 0u, 0u, 0u };
                if constexpr (kCover) { ca = load_row<kVec>(CA, idx, nx); cb = load_row<kVec>(CB, idx, nx); }
                const uint32_t pa[4] = { va.x, va.y, va.z, va.w }, pb[4] = { vb.x, vb.y, vb.z, vb.w };
                const uint32_t qa[4] = { ca.x, ca.y, ca.z, ca.w }, qb[4] = { cb.x, cb.y, cb.z, cb.w };
                uint32_t out[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    if (kVec || p < nx) {
                        const uint32_t ya = luma(pa[p]), yb = luma(pb[p]);
                        s1 += ya; s2 += yb; ssq += ya * ya + yb * yb; s12 += ya * yb;
                        const bool in_a = kCover ? (qa[p] >> 24) != 0u : true, in_b = kCover ? (qb[p] >> 24) != 0u : true;
                        const bool m = k.mask_mode == 0u ? true : k.mask_mode == 1u ? in_a : k.mask_mode == 2u ? (in_a || in_b) : (in_a && in_b);
                        pass += m ? 1u : 0u;
                        if (own) {
                            cov0 += (!in_a && !in_b) ? 1u : 0u; cov1 += (in_a && !in_b) ? 1u : 0u;
                            cov2 += (!in_a && in_b) ? 1u : 0u;  cov3 += (in_a && in_b) ? 1u : 0u;
                            if (m) {
                                const uint32_t d0 = absdiff8(pa[p] & 255u, pb[p] & 255u), d1 = absdiff8((pa[p] >> 8) & 255u, (pb[p] >> 8) & 255u),
                                               d2 = absdiff8((pa[p] >> 16) & 255u, (pb[p] >> 16) & 255u);
                                sse0 += d0 * d0; sse1 += d1 * d1; sse2 += d2 * d2;
                                sad0 += d0; sad1 += d1; sad2 += d2;
                                mx0 = max(mx0, d0); mx1 = max(mx1, d1); mx2 = max(mx2, d2);
                                out[p] = d0 | (d1 << 8) | (d2 << 16) | 0xFF000000u;
                            }
                        }
                    }
                }
                if (own && map) {
                    if constexpr (kVec) {
                        *reinterpret_cast<uint4*>(map + idx) = make_uint4(out[0], out[1], out[2], out[3]);
                    } else {
#pragma unroll
                        for (int p = 0; p < 4; ++p) if (p < nx) map[idx + p] = out[p];
                    }
                }
            }
        }
    }
    if (in_grid) { s_cell[0][tid] = s1; s_cell[1][tid] = s2; s_cell[2][tid] = ssq; s_cell[3][tid] = s12; s_cell[4][tid] = pass; }
    __syncthreads();

    // the window whose lower left cell this lane owns: 2 x 2 cells, all four whole
    uint32_t windows = 0;
    long long q = 0;
    if (own && x0 + 8 <= k.W && y0 + 8 <= k.H) {
        uint32_t w[5];
#pragma unroll
        for (int f = 0; f < 5; ++f)
            w[f] = (s_cell[f][tid] + s_cell[f][tid + 1]) + (s_cell[f][tid + kScoreGridCells] + s_cell[f][tid + kScoreGridCells + 1]);
        if (w[4] >= 32u) {
            const long long a1 = (long long)w[0], a2 = (long long)w[1], sq = (long long)w[2], cr = (long long)w[3];
            const long long c1 = 26634, c2 = 239708;
            const long long num = (2 * a1 * a2 + c1) * (128 * cr - 2 * a1 * a2 + c2);
            const long long den = (a1 * a1 + a2 * a2 + c1) * (64 * sq - a1 * a1 - a2 * a2 + c2);
            const double ssim = (double)num / (double)den;      // fp64, correctly rounded: no fast-math for this file
            q = llrint(ssim * 4294967296.0);
            windows = 1u;
        }
    }

    // wave -> workgroup -> one atomic per counter
    const uint32_t v[kScoreCounters - 1] = { wave_sum(own ? pass : 0u), wave_sum(cov0), wave_sum(cov1), wave_sum(cov2), wave_sum(cov3),
                                             wave_sum(sse0), wave_sum(sse1), wave_sum(sse2), wave_sum(sad0), wave_sum(sad1), wave_sum(sad2),
                                             wave_max(mx0), wave_max(mx1), wave_max(mx2), wave_sum(windows) };
    const long long qs = wave_sum64(q);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < kScoreCounters - 1; ++i) {
            if (v[i] == 0u) continue;
            if (i >= kScoreMaxFirst && i <= kScoreMaxLast) atomicMax(&s_acc[i], (unsigned long long)v[i]);
            else atomicAdd(&s_acc[i], (unsigned long long)v[i]);
        }
        if (qs != 0) atomicAdd(&s_acc[kScoreCounters - 1], (unsigned long long)qs);
    }
    __syncthreads();
    if (tid < kScoreCounters) {
        const unsigned long long t = s_acc[tid];
        unsigned long long* dst = acc + (size_t)(blockIdx.x % (uint32_t)kScoreShards) * kScoreCounters + tid;
        if (t != 0ull) {
            if (tid >= kScoreMaxFirst && tid <= kScoreMaxLast) atomicMax(dst, t);
            else atomicAdd(dst, t);
        }
    }
}

}  // namespace

hipError_t launch_score(const ScoreK& k, const uint32_t* a, const uint32_t* b, const uint32_t* cover_a, const uint32_t* cover_b, uint32_t* map,
                        unsigned long long* acc, hipStream_t st) {
    const bool cover = cover_a != nullptr && cover_b != nullptr;
    auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; };
    const bool vec = (k.W % 4) == 0 && aligned(a) && aligned(b) && aligned(cover_a) && aligned(cover_b) && aligned(map);
    const dim3 grid(k.tiles_x * score_tiles(k.H)), block(kScoreThreads);
    if (vec && cover) hipLaunchKernelGGL((k_score<true, true>), grid, block, 0, st, k, a, b, cover_a, cover_b, map, acc);
    else if (vec) hipLaunchKernelGGL((k_score<true, false>), grid, block, 0, st, k, a, b, cover_a, cover_b, map, acc);
    else if (cover) hipLaunchKernelGGL((k_score<false, true>), grid, block, 0, st, k, a, b, cover_a, cover_b, map, acc);
    else hipLaunchKernelGGL((k_score<false, false>), grid, block, 0, st, k, a, b, cover_a, cover_b, map, acc);
    return hipGetLastError();
}

hipError_t preload_score() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_score<true, true>)); }

}  // namespace m2s
