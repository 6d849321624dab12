// m2s_compact.hip — device side of the compact .ply export (include/m2s.h "compact export"): validity + bounding box,
// Morton keys, rocPRIM's stable radix sort, and the chunk encoder — one 256-lane workgroup per chunk of 256 sorted rows, which reduces
// the chunk's 18 bounds and packs every row into four words.  Every rounding, clamp and bit position is m2s_compactmath.h's, the very
// functions the host writer (m2s_compact_host.cpp) is built from; the logarithm is logf_glibc.  No atomics: per-wave partial results are
// left in memory and folded by a small kernel, the shape of the depth sort's {min, max} stage (m2s_sort.hip).
#include <rocprim/device/device_radix_sort.hpp>

#include "m2s_compactmath.h"
#include "m2s_device.h"
#include "m2s_logf.h"

#pragma clang fp contract(off)

namespace m2s {

namespace mc = m2s_compact;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// min / max of v over the wave by DPP: a butterfly inside every row of 16 lanes (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror,
// row_mirror), then row_bcast15 into rows 1 and 3 and row_bcast31 into rows 2 and 3; lane 63 holds the result.  A lane the step does
// not write keeps `old` = its own value, the neutral element of both.
template <bool kMin>
__device__ __forceinline__ uint32_t wave_reduce(uint32_t v) {
#define M2S_STEP(ctrl, rows)                                                                                   \
    {                                                                                                           \
        const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, rows, 0xf, false);     \
        v = kMin ? min(v, o) : max(v, o);                                                                       \
    }
    M2S_STEP(0xB1, 0xf)
    M2S_STEP(0x4E, 0xf)
    M2S_STEP(0x141, 0xf)
    M2S_STEP(0x140, 0xf)
    M2S_STEP(0x142, 0xa)
    M2S_STEP(0x143, 0xc)
#undef M2S_STEP
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Validity (pin 1) and the box (pin 2).  keys[i] = 0 for a valid record, kInvalidKey for any other (k_compact_keys reads it back instead
// of the three other fields); wave_box[wave] = { min.xyz, max.xyz (mc::ord), valid records, 0 }: 32 bytes per 64 records.  The position
// comes from the 16-byte plane where the context has one.
__global__ void __launch_bounds__(kBlock) k_compact_box(const float4* __restrict__ rec, const float4* __restrict__ plane, uint32_t n,
                                                        uint32_t* __restrict__ keys, u32x4* __restrict__ wave_box) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool ok = false;
    uint32_t lo0 = mc::kOrdMinNeutral, lo1 = mc::kOrdMinNeutral, lo2 = mc::kOrdMinNeutral;
    uint32_t hi0 = mc::kOrdMaxNeutral, hi1 = mc::kOrdMaxNeutral, hi2 = mc::kOrdMaxNeutral;
    if (i < n) {
        const float4* g = rec + (size_t)i * 6;
        const float4 pos = plane ? plane[i] : g[0], col = g[1], scl = g[2], rot = g[4];
        const float p[3] = { pos.x, pos.y, pos.z }, c[4] = { col.x, col.y, col.z, col.w }, s[3] = { scl.x, scl.y, scl.z }, q[4] = { rot.x, rot.y, rot.z, rot.w };
        ok = mc::valid(p, c, s, q);
        keys[i] = ok ? 0u : mc::kInvalidKey;
        if (ok) { lo0 = hi0 = mc::ord(pos.x); lo1 = hi1 = mc::ord(pos.y); lo2 = hi2 = mc::ord(pos.z); }
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(ok));
    lo0 = wave_reduce<true>(lo0); lo1 = wave_reduce<true>(lo1); lo2 = wave_reduce<true>(lo2);
    hi0 = wave_reduce<false>(hi0); hi1 = wave_reduce<false>(hi1); hi2 = wave_reduce<false>(hi2);
    if ((threadIdx.x & 63) == 0) {
        u32x4* w = wave_box + (size_t)((blockIdx.x * kBlock + threadIdx.x) >> 6) * 2;
        w[0] = u32x4{ lo0, lo1, lo2, hi0 };
        w[1] = u32x4{ hi1, hi2, cnt, 0u };
    }
}

// One workgroup folds the per-wave entries: head = { min.xyz, max.xyz, N, skipped }.
__global__ void __launch_bounds__(kBlock) k_compact_fold(const u32x4* __restrict__ wave_box, uint32_t n_waves, uint32_t n, uint32_t* __restrict__ head) {
    __shared__ uint32_t s_part[kBlock / 64][8];
    uint32_t lo0 = mc::kOrdMinNeutral, lo1 = mc::kOrdMinNeutral, lo2 = mc::kOrdMinNeutral;
    uint32_t hi0 = mc::kOrdMaxNeutral, hi1 = mc::kOrdMaxNeutral, hi2 = mc::kOrdMaxNeutral, cnt = 0;
    for (uint32_t w = threadIdx.x; w < n_waves; w += kBlock) {
        const u32x4 a = wave_box[(size_t)w * 2], b = wave_box[(size_t)w * 2 + 1];
        lo0 = min(lo0, a.x); lo1 = min(lo1, a.y); lo2 = min(lo2, a.z);
        hi0 = max(hi0, a.w); hi1 = max(hi1, b.x); hi2 = max(hi2, b.y);
        cnt += b.z;
    }
    lo0 = wave_reduce<true>(lo0); lo1 = wave_reduce<true>(lo1); lo2 = wave_reduce<true>(lo2);
    hi0 = wave_reduce<false>(hi0); hi1 = wave_reduce<false>(hi1); hi2 = wave_reduce<false>(hi2);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, d);
    if ((threadIdx.x & 63) == 0) {
        uint32_t* s = s_part[threadIdx.x >> 6];
        s[0] = lo0; s[1] = lo1; s[2] = lo2; s[3] = hi0; s[4] = hi1; s[5] = hi2; s[6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const uint32_t k = threadIdx.x;
        uint32_t v = s_part[0][k];
        for (int w = 1; w < kBlock / 64; ++w) v = k < 3 ? min(v, s_part[w][k]) : k < 6 ? max(v, s_part[w][k]) : v + s_part[w][k];
        head[k] = v;
        if (k == 6) head[7] = n - v;
    }
}

// Pin 3: the key of every valid record, and the record index as the sort's value.
__global__ void __launch_bounds__(kBlock) k_compact_keys(const float4* __restrict__ rec, const float4* __restrict__ plane, uint32_t n,
                                                         const uint32_t* __restrict__ head, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    vals[i] = i;
    if (keys[i] != 0u) return;                                  // kInvalidKey: behind every valid record
    const float4 pos = plane ? plane[i] : rec[(size_t)i * 6];
    const float p[3] = { pos.x, pos.y, pos.z };
    const float bmin[3] = { mc::unord(head[0]), mc::unord(head[1]), mc::unord(head[2]) };
    const float bmax[3] = { mc::unord(head[3]), mc::unord(head[4]), mc::unord(head[5]) };
    keys[i] = mc::morton_key(p, bmin, bmax);
}

// Pins 5 - 8.  Workgroup c = chunk c, lane t = sorted row 256 c + t (lanes past the last row are neutral).  The lane gathers position,
// colour, scale and rotation of record perm[row] (64 of its 96 bytes), with a baked plane also that record's plane row; the 18 bounds
// are reduced by DPP inside the wave and through LDS across the four waves; lanes 0..17 store them; every lane stores its row as one
// non-temporal 16-byte word.  The SH bytes (9 / 24 / 45 per row) are staged in LDS and leave as 16 bytes per lane.
constexpr uint32_t kShStageWords = kBlock * 45 / 16;           // 720 x 16 bytes: a chunk's SH bytes at degree 3
template <bool kSH>
__global__ void __launch_bounds__(kBlock) k_compact_pack(const float4* __restrict__ rec, const float* __restrict__ sh, const uint32_t* __restrict__ perm,
                                                         uint32_t N, float sm, uint32_t K, float* __restrict__ table, u32x4* __restrict__ rows,
                                                         u32x4* __restrict__ sh_out) {
    __shared__ uint32_t s_red[kBlock / 64][18];                 // per wave: 9 minima, 9 maxima (mc::ord)
    __shared__ float s_tab[18];
    __shared__ u32x4 s_sh[kSH ? kShStageWords : 1];
    const uint32_t c = blockIdx.x, t = threadIdx.x;
    const uint32_t row = c * kBlock + t;
    const bool active = row < N;
    float v[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };                 // p, ls, col
    float alpha = 0.0f, q[4] = { 1.0f, 0.0f, 0.0f, 0.0f };
    uint32_t src = 0;
    if (active) {
        src = perm[row];
        const float4* g = rec + (size_t)src * 6;
        const float4 pos = g[0], col = g[1], scl = g[2], rot = g[4];
        v[0] = pos.x; v[1] = pos.y; v[2] = pos.z;
        v[3] = mc::clamp_log_scale(logf_glibc(scl.x * sm));
        v[4] = mc::clamp_log_scale(logf_glibc(scl.y * sm));
        v[5] = mc::clamp_log_scale(logf_glibc(scl.z * sm));
        v[6] = col.x; v[7] = col.y; v[8] = col.z;
        if (sh) {
            const float* d = sh + (size_t)src * 48;
            v[6] = mc::sh_dc_colour(d[0]); v[7] = mc::sh_dc_colour(d[1]); v[8] = mc::sh_dc_colour(d[2]);
        }
        alpha = col.w;
        q[0] = rot.x; q[1] = rot.y; q[2] = rot.z; q[3] = rot.w;
    }
    uint32_t mn[9], mx[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const uint32_t o = mc::ord(v[k]);
        mn[k] = wave_reduce<true>(active ? o : mc::kOrdMinNeutral);
        mx[k] = wave_reduce<false>(active ? o : mc::kOrdMaxNeutral);
    }
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) { s_red[t >> 6][k] = mn[k]; s_red[t >> 6][9 + k] = mx[k]; }
    }
    if (kSH) {                                                  // this lane's SH bytes, channel-major (pin 8)
        uint8_t* b = reinterpret_cast<uint8_t*>(s_sh) + t * 3 * K;
        const float* d = sh + (size_t)src * 48;
        for (uint32_t ch = 0; ch < 3; ++ch)
            for (uint32_t i = 1; i <= K; ++i) b[ch * K + i - 1] = active ? (uint8_t)mc::sh_byte(d[mc::sh_plane_word(ch, i)]) : (uint8_t)0;
    }
    __syncthreads();
    if (t < 18) {                                               // min_xyz max_xyz | min_scale max_scale | min_rgb max_rgb
        const uint32_t grp = t / 6, r = t % 6, k = (r >= 3 ? 9u : 0u) + 3 * grp + r % 3;
        uint32_t o = s_red[0][k];
        for (int w = 1; w < kBlock / 64; ++w) o = r >= 3 ? max(o, s_red[w][k]) : min(o, s_red[w][k]);
        const float f = mc::unord(o);
        s_tab[t] = f;
        table[(size_t)c * 18 + t] = f;
    }
    __syncthreads();
    if (active) {
        float lo[9], hi[9];
#pragma unroll
        for (int grp = 0; grp < 3; ++grp)
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[3 * grp + a] = s_tab[6 * grp + a]; hi[3 * grp + a] = s_tab[6 * grp + 3 + a]; }
        const u32x4 w = { mc::pack_11_10_11(v, lo, hi), mc::pack_rotation(q), mc::pack_11_10_11(v + 3, lo + 3, hi + 3),
                          mc::pack_colour(v + 6, lo + 6, hi + 6, alpha) };
        __builtin_nontemporal_store(w, rows + row);
    }
    if (kSH) {                                                  // (sh_out holds whole chunks: the last piece of the last chunk stays inside it)
        const uint32_t in_chunk = min((uint32_t)kBlock, N - c * kBlock);
        const uint32_t pieces = (in_chunk * 3 * K + 15) / 16;
        u32x4* dst = sh_out + (size_t)c * (kBlock * 3 * K / 16);
        for (uint32_t j = t; j < pieces; j += kBlock) __builtin_nontemporal_store(s_sh[j], dst + j);
    }
}

size_t compact_sort_temp_bytes(uint32_t n) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 31, (hipStream_t)0);
    return bytes;
}

// keys_in / vals_in / keys_out / vals_out: n words each; wave_box: compact_waves(n) * 8 words; head: 8 words.  Afterwards head =
// { box, N, skipped } and the first N words of vals_out are the permutation.  marks: around box + keys (0, 1) and the sort (1, 2).
hipError_t compact_keys_and_sort(const float4* rec, const float4* plane, uint32_t n, uint32_t* wave_box, uint32_t* head, uint32_t* keys_in, uint32_t* vals_in,
                                 uint32_t* keys_out, uint32_t* vals_out, void* temp, size_t temp_bytes, const m2s_host::StageMarks& marks, hipStream_t st) {
    if (!n) return hipErrorInvalidValue;
    const dim3 grid((n + kBlock - 1) / kBlock);
    (void)marks.mark(0, st);
    hipLaunchKernelGGL(k_compact_box, grid, dim3(kBlock), 0, st, rec, plane, n, keys_in, reinterpret_cast<u32x4*>(wave_box));
    hipLaunchKernelGGL(k_compact_fold, dim3(1), dim3(kBlock), 0, st, reinterpret_cast<const u32x4*>(wave_box), compact_waves(n), n, head);
    hipLaunchKernelGGL(k_compact_keys, grid, dim3(kBlock), 0, st, rec, plane, n, (const uint32_t*)head, keys_in, vals_in);
    (void)marks.mark(1, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, 31, st);
    (void)marks.mark(2, st);
    return e;
}

// table: 18 floats per chunk; rows: N x 16 bytes; sh_out (K != 0): whole chunks of 256 x 3 K bytes.  sh: the baked plane or NULL.
hipError_t compact_pack(const float4* rec, const float* sh, const uint32_t* perm, uint32_t N, float sm, uint32_t K, float* table, void* rows, void* sh_out,
                        hipStream_t st) {
    if (!N) return hipSuccess;
    if (K && (!sh || !sh_out || (K != 3 && K != 8 && K != 15))) return hipErrorInvalidValue;
    const dim3 grid((N + kBlock - 1) / kBlock);
    if (K) hipLaunchKernelGGL(k_compact_pack<true>, grid, dim3(kBlock), 0, st, rec, sh, perm, N, sm, K, table, static_cast<u32x4*>(rows), static_cast<u32x4*>(sh_out));
    else hipLaunchKernelGGL(k_compact_pack<false>, grid, dim3(kBlock), 0, st, rec, sh, perm, N, sm, 0u, table, static_cast<u32x4*>(rows), (u32x4*)nullptr);
    return hipGetLastError();
}

}  // namespace m2s
