// m2s_vdedup.hip — the deduplicated vertex table of an uploaded scene (m2s_vtable.h), built once per upload from the SoA planes.
//
// The loader de-indexes its meshes: every vertex is stored once per corner that uses it (config 3: 3 006 756 corners, 501 128 distinct
// vertices).  The strips of k_fused3 gather a triangle's normals, tangents and positions per fragment; from a table of distinct vertices
// the same operand bits come out of a sixth of the memory, and neighbouring triangles read the same lines.
//
//   1. k_vt_insert   one lane per triangle, its three corners in turn: an open-addressing table (linear probing, at most half full) of
//                    OWNER CORNER INDICES.  A corner claims an empty slot with atomicCAS; at an occupied slot it compares its 12 words
//                    with the current owner's (bitwise: -0.0 and +0.0 differ, NaNs compare by payload) and, if they are equal, settles
//                    the owner with atomicMin — the slot of a key never changes, its owner only moves down.  The slot is kept per corner.
//   2. k_vt_flags    owner[c] = table[slot of c]; flag[c] = (owner[c] == c): the first corner of every distinct vertex.
//   3. exclusive scan of the flags (rocprim): rank[c]; rank[corners] = U, the number of rows.
//   4. k_vt_emit     ids of a triangle = ranks of its corners' owners, packed (vt_pack); an owner writes its row.
// Ids are therefore ranks in first-occurrence order: the table is deterministic and neighbouring triangles' rows are neighbours.
// Steps 1-3 are enqueued by vt_dedup_begin (no host wait); vt_dedup_finish reads U, decides (vt_rows_ok), allocates the exact
// table, runs step 4 and frees the temporaries.
#include "m2s_vdedup.h"

#include <rocprim/device/device_scan.hpp>

namespace m2s {
namespace {
constexpr uint32_t kVtEmpty = 0xFFFFFFFFu;

struct Planes32 {    // the planes as words
    const uint32_t *A0, *A1, *A2, *B0, *B1, *C0, *C1, *C2, *D0, *D1, *D2;
};
__host__ Planes32 as_words(const TriPlanes& tp) {
    return Planes32{ (const uint32_t*)tp.A0, (const uint32_t*)tp.A1, (const uint32_t*)tp.A2, (const uint32_t*)tp.B0, (const uint32_t*)tp.B1,
                     (const uint32_t*)tp.C0, (const uint32_t*)tp.C1, (const uint32_t*)tp.C2, (const uint32_t*)tp.D0, (const uint32_t*)tp.D1,
                     (const uint32_t*)tp.D2 };
}
// word j (0 .. 8) of the nine a triangle keeps in a (float4, float4, float) plane triple
__device__ __forceinline__ uint32_t word9(const uint32_t* p0, const uint32_t* p1, const uint32_t* p2, uint32_t t, uint32_t j) {
    return j < 4u ? p0[4u * t + j] : j < 8u ? p1[4u * t + (j - 4u)] : p2[t];
}
// the 12 words of corner c in row order: p.xyz u | n.xyz v | t.xyzw
__device__ __forceinline__ void load_corner(const Planes32& P, uint32_t c, uint32_t k[12]) {
    const uint32_t t = c / 3u, v = c - 3u * t;
#pragma unroll
    for (uint32_t i = 0; i < 3u; ++i) {
        k[i] = word9(P.A0, P.A1, P.A2, t, 3u * v + i);
        k[4u + i] = word9(P.C0, P.C1, P.C2, t, 3u * v + i);
    }
    k[3] = v < 2u ? P.B0[4u * t + 2u * v] : P.B1[2u * t];
    k[7] = v < 2u ? P.B0[4u * t + 2u * v + 1u] : P.B1[2u * t + 1u];
    const uint32_t* d = v == 0u ? P.D0 : v == 1u ? P.D1 : P.D2;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) k[8u + i] = d[4u * t + i];
}
__device__ __forceinline__ uint32_t hash12(const uint32_t k[12]) {
    uint32_t h = 0x9E3779B9u;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        h = (h ^ k[i]) * 0x85EBCA6Bu;
        h ^= h >> 13;
    }
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

__global__ void __launch_bounds__(256) k_vt_insert(Planes32 P, uint32_t n_tri, uint32_t* table, uint32_t mask, uint32_t* __restrict__ slot_of) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tri) return;
    for (uint32_t v = 0; v < 3u; ++v) {
        const uint32_t c = 3u * t + v;
        uint32_t key[12];
        load_corner(P, c, key);
        uint32_t slot = hash12(key) & mask;
        for (;;) {   // (the table is at most half full: an empty slot ends every probe sequence)
            uint32_t cur = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kVtEmpty) {
                cur = atomicCAS(&table[slot], kVtEmpty, c);
                if (cur == kVtEmpty) break;                       // claimed
            }
            uint32_t other[12];                                   // the slot belongs to the vertex of corner `cur` (whoever owns it later)
            load_corner(P, cur, other);
            bool same = true;
#pragma unroll
            for (int i = 0; i < 12; ++i) same = same && key[i] == other[i];
            if (same) { atomicMin(&table[slot], c); break; }
            slot = (slot + 1u) & mask;
        }
        slot_of[c] = slot;
    }
}

// slot_of[c] becomes owner[c]; flags has corners + 1 words (the last one 0: the scan then leaves U behind it)
__global__ void __launch_bounds__(256) k_vt_flags(const uint32_t* __restrict__ table, uint32_t corners, uint32_t* __restrict__ slot_of, uint32_t* __restrict__ flags) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c > corners) return;
    if (c == corners) { flags[c] = 0u; return; }
    const uint32_t own = table[slot_of[c]];
    slot_of[c] = own;
    flags[c] = own == c ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_vt_emit(Planes32 P, uint32_t n_tri, const uint32_t* __restrict__ owner, const uint32_t* __restrict__ rank,
                                                  uint32_t n_rows, uint4* __restrict__ rows, VtIds* __restrict__ ids) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_tri) return;
    uint32_t id[3];
#pragma unroll
    for (uint32_t v = 0; v < 3u; ++v) {
        const uint32_t c = 3u * t + v, own = owner[c];
        id[v] = rank[own];
        if (own == c && id[v] < n_rows) {
            uint32_t k[12];
            load_corner(P, c, k);
            uint4* r = rows + (size_t)id[v] * kVtRowF4;
            r[0] = make_uint4(k[0], k[1], k[2], k[3]);
            r[1] = make_uint4(k[4], k[5], k[6], k[7]);
            r[2] = make_uint4(k[8], k[9], k[10], k[11]);
        }
    }
    ids[t] = vt_pack(id[0], id[1], id[2]);
}

size_t scan_temp_bytes(uint32_t n) {
    size_t b = 0;
    (void)rocprim::exclusive_scan(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(), (hipStream_t)0);
    return b < 256 ? 256 : b;
}
}  // namespace

uint32_t vt_hash_words(uint32_t corners) {
    uint32_t w = 1024u;
    while (w < 2u * corners) w <<= 1;
    return w;
}

void VtWork::release() {
    if (mem) (void)hipFree(mem);
    mem = nullptr;
    table = owner = flags = rank = nullptr;
    temp = nullptr;
    temp_bytes = 0;
    corners = 0;
}

hipError_t vt_dedup_begin(const TriPlanes& tp, uint32_t n_tri, VtWork& w, hipStream_t st) {
    w.release();
    if (n_tri == 0 || n_tri > kVtMaxTriangles) return hipErrorInvalidValue;
    const uint32_t corners = 3u * n_tri, words = vt_hash_words(corners);
    const size_t tb = scan_temp_bytes(corners + 1u);
    // one allocation: table | owner | flags | rank | scan work area, each from a 256-byte boundary
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t o_owner = up((size_t)words * 4), o_flags = o_owner + up((size_t)corners * 4), o_rank = o_flags + up(((size_t)corners + 1) * 4),
                 o_temp = o_rank + up(((size_t)corners + 1) * 4);
    hipError_t e = hipMalloc(&w.mem, o_temp + tb);
    if (e != hipSuccess) { w.mem = nullptr; return e; }
    char* const m = (char*)w.mem;
    w.table = (uint32_t*)m; w.owner = (uint32_t*)(m + o_owner); w.flags = (uint32_t*)(m + o_flags); w.rank = (uint32_t*)(m + o_rank);
    w.temp = m + o_temp;
    w.temp_bytes = tb;
    w.corners = corners;
    const Planes32 P = as_words(tp);
    if ((e = hipMemsetAsync(w.table, 0xFF, (size_t)words * 4, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_vt_insert, dim3((n_tri + 255u) / 256u), dim3(256), 0, st, P, n_tri, w.table, words - 1u, w.owner);
    hipLaunchKernelGGL(k_vt_flags, dim3((corners + 1u + 255u) / 256u), dim3(256), 0, st, (const uint32_t*)w.table, corners, w.owner, w.flags);
    size_t bytes = w.temp_bytes;
    if ((e = rocprim::exclusive_scan(w.temp, bytes, (const uint32_t*)w.flags, w.rank, 0u, (size_t)corners + 1u, rocprim::plus<uint32_t>(), st)) != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t vt_dedup_finish(const TriPlanes& tp, uint32_t n_tri, VtWork& w, uint32_t id_limit, uint32_t min_sharing, m2s_host::DevBuf<float4>& rows,
                           m2s_host::DevBuf<VtIds>& ids, uint32_t* n_rows, bool* eligible, hipStream_t st) {
    *n_rows = 0;
    *eligible = false;
    if (!w.rank || w.corners != 3u * n_tri) { w.release(); return hipErrorInvalidValue; }
    uint32_t U = 0;
    hipError_t e = hipMemcpyAsync(&U, w.rank + w.corners, sizeof(U), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { w.release(); return e; }
    *n_rows = U;
    if (vt_rows_ok(U, w.corners, id_limit, min_sharing)) {
        std::string err;
        rows.release();
        ids.release();
        if (rows.reserve(err, (uint64_t)U * kVtRowF4, sizeof(float4)) != M2S_OK || ids.reserve(err, n_tri, sizeof(VtIds)) != M2S_OK) {
            rows.release(); ids.release(); w.release();
            (void)hipGetLastError();
            return hipErrorOutOfMemory;
        }
        hipLaunchKernelGGL(k_vt_emit, dim3((n_tri + 255u) / 256u), dim3(256), 0, st, as_words(tp), n_tri, (const uint32_t*)w.owner, (const uint32_t*)w.rank, U,
                           reinterpret_cast<uint4*>(rows.get()), ids.get());
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        *eligible = e == hipSuccess;
    }
    w.release();
    return e;
}

}  // namespace m2s
