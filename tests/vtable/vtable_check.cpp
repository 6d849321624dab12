// vtable_check — mesh2splat_amd/csrc/m2s_vtable.h with a plain host compiler under AddressSanitizer + UBSan (tests/test_vtable_cpu.py):
// the 3 x 21-bit id triple survives vt_pack / vt_unpack at the ends of its range in every position and mixed, and the eligibility rule
// turns exactly at its three edges.
#include "../../mesh2splat_amd/csrc/m2s_vtable.h"

#include <cstdio>
#include <cstdlib>

using namespace m2s;

#define REQUIRE(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static bool round_trip(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t x = ~0u, y = ~0u, z = ~0u;
    const VtIds p = vt_pack(a, b, c);
    vt_unpack(p, x, y, z);
    return x == a && y == b && z == c && (p.hi >> 31) == 0u;      // 63 bits
}

int main() {
    static_assert(sizeof(VtIds) == 8, "the ids take the 8 bytes of two floats");
    static_assert(kVtIdLimit == 1u << 21 && 3 * kVtIdBits <= 64, "three ids in 64 bits");
    const uint32_t ends[4] = { 0u, 1u, kVtIdLimit - 2u, kVtIdLimit - 1u };
    for (uint32_t a : ends)
        for (uint32_t b : ends)
            for (uint32_t c : ends) REQUIRE(round_trip(a, b, c));
    // each value alone in each position: no bit of one id reaches another
    for (uint32_t v : ends) {
        REQUIRE(round_trip(v, 0, 0) && round_trip(0, v, 0) && round_trip(0, 0, v));
        REQUIRE(round_trip(v, kVtIdLimit - 1u, kVtIdLimit - 1u) && round_trip(kVtIdLimit - 1u, v, kVtIdLimit - 1u) && round_trip(kVtIdLimit - 1u, kVtIdLimit - 1u, v));
    }
    uint32_t s = 12345u;   // mixed
    for (int i = 0; i < 100000; ++i) {
        uint32_t id[3];
        for (uint32_t& q : id) { s = s * 1664525u + 1013904223u; q = (s >> 9) & (kVtIdLimit - 1u); }
        REQUIRE(round_trip(id[0], id[1], id[2]));
    }
    REQUIRE(vt_pack(1, 0, 0).lo == 1u && vt_pack(0, 1, 0).lo == 1u << 21 && vt_pack(0, 0, 1).hi == 1u << 10);

    // edge 1: the scene may take the lean form at all; edge 2: n_tri <= 2^22
    REQUIRE(vt_size_ok(true, 1) && vt_size_ok(true, kVtMaxTriangles) && !vt_size_ok(true, (uint64_t)kVtMaxTriangles + 1) && !vt_size_ok(true, 0));
    REQUIRE(!vt_size_ok(false, 1) && !vt_size_ok(false, kVtMaxTriangles));
    // edge 3: rows < 2^21 and rows <= corners / 2
    const uint64_t many = 3ull * kVtMaxTriangles;
    REQUIRE(vt_rows_ok(kVtIdLimit - 1u, many, kVtIdLimit, kVtMinSharing) && !vt_rows_ok(kVtIdLimit, many, kVtIdLimit, kVtMinSharing));
    REQUIRE(vt_rows_ok(300, 600, kVtIdLimit, kVtMinSharing) && !vt_rows_ok(301, 600, kVtIdLimit, kVtMinSharing));
    REQUIRE(vt_rows_ok(300, 601, kVtIdLimit, kVtMinSharing) && !vt_rows_ok(301, 601, kVtIdLimit, kVtMinSharing));   // corners / 2 rounds down
    REQUIRE(!vt_rows_ok(0, 600, kVtIdLimit, kVtMinSharing));
    REQUIRE(vt_rows_ok(81, 384, 82, 4) && !vt_rows_ok(81, 384, 81, 4) && !vt_rows_ok(81, 384, 82, 5));              // the limits are parameters
    std::printf("vtable_check ok\n");
    return 0;
}
