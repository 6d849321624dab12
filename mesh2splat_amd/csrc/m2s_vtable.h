// m2s_vtable.h — the deduplicated vertex table of an uploaded scene (built by m2s_vdedup.hip, read by the indexed instance of k_fused3):
// its layout, the packing of a triangle's three row ids into 64 bits, and the rule that decides whether a scene uses it.
// Compiles for the host (a plain C++ compiler: tests/vtable) and for the device; no runtime header is needed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define M2S_VT_HD __host__ __device__ inline
#else
#define M2S_VT_HD inline
#endif

namespace m2s {

// Row r of the table is three float4: (p.xyz, u), (n.xyz, v), (t.xyzw) — 48 bytes, the 12 attribute floats of one distinct vertex.
constexpr uint32_t kVtRowF4 = 3;
constexpr uint32_t kVtIdBits = 21;                           // three ids fit 64 bits (the 8 bytes TriShadeSI keeps per triangle)
constexpr uint32_t kVtIdLimit = 1u << kVtIdBits;             // a table must have FEWER rows than this
constexpr uint32_t kVtMaxTriangles = 1u << 22;               // bounds the temporary hash table (2^25 words = 128 MB)
constexpr uint32_t kVtMinSharing = 2;                        // rows <= corners / this: below it a workgroup's rows (-> 72 B per triangle
                                                             // plus ids) no longer pay against the 120 B of the plane gathers

struct VtIds { uint32_t lo, hi; };                           // id0 | id1 << 21 | id2 << 42
M2S_VT_HD VtIds vt_pack(uint32_t i0, uint32_t i1, uint32_t i2) {
    const unsigned long long w = (unsigned long long)i0 | ((unsigned long long)i1 << kVtIdBits) | ((unsigned long long)i2 << (2 * kVtIdBits));
    return VtIds{ (uint32_t)w, (uint32_t)(w >> 32) };
}
M2S_VT_HD void vt_unpack(VtIds p, uint32_t& i0, uint32_t& i1, uint32_t& i2) {
    const uint32_t m = kVtIdLimit - 1u;
    i0 = p.lo & m;
    i1 = ((p.lo >> kVtIdBits) | (p.hi << (32u - kVtIdBits))) & m;
    i2 = (p.hi >> (2u * kVtIdBits - 32u)) & m;
}

// Decided once per upload.  id_limit / min_sharing are parameters (kVtIdLimit, kVtMinSharing in the library) so that a test reaches
// both "not eligible" exits with small inputs.
M2S_VT_HD bool vt_size_ok(bool lean_ok, uint64_t n_tri) { return lean_ok && n_tri >= 1 && n_tri <= kVtMaxTriangles; }
M2S_VT_HD bool vt_rows_ok(uint64_t rows, uint64_t corners, uint32_t id_limit, uint32_t min_sharing) {
    return rows >= 1 && rows < id_limit && rows * min_sharing <= corners;
}

// What the indexed instance of k_fused3 reads (device pointers; rows == nullptr: the scene has no table)
struct VtxTable {
    const void* rows;        // float4[U][3]
    const void* ids;         // VtIds per resident triangle (8 B: one coalesced read per lane in the triangle phase)
};

}  // namespace m2s
