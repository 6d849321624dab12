// vdedup_check — the vertex deduplication of mesh2splat_amd/csrc/m2s_vdedup.hip (this program links that translation unit) against a
// host std::map, on the GPU the suite runs on.  Usage: vdedup_check [file.f32]  (file: de-indexed vertices, 12 floats each — the
// caller's cube-sphere).  One JSON line per case; exit status 0 when every case passed.
//
// Every case checks: table[id[c]] == corner c bitwise for every corner; the number of rows equals the reference's; ids are ranks in
// first-occurrence order (the reference numbers its keys in corner order); a second run gives the same rows and ids.  The two
// "not eligible" cases pass small limits and expect no table.
#include "m2s_vdedup.h"

#include <array>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

using namespace m2s;
using Key = std::array<uint32_t, 12>;

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::printf("{\"error\": \"%s: %s\"}\n", #call, hipGetErrorString(e_)); return false; } } while (0)

namespace {
struct DevPlanes {
    void* mem = nullptr;
    TriPlanes tp{};
    ~DevPlanes() { if (mem) (void)hipFree(mem); }
};
// corners: n_tri * 3 rows of 12 words (p.xyz n.xyz t.xyzw uv.xy, the loader's order) -> the 11 planes of the library's layout
bool upload(const std::vector<Key>& corners, uint32_t n_tri, DevPlanes& d) {
    const size_t widths[11] = { 16, 16, 4, 16, 8, 16, 16, 4, 16, 16, 16 };
    size_t offs[11], cur = 0;
    for (int k = 0; k < 11; ++k) { offs[k] = cur; cur = (cur + n_tri * widths[k] + 255) / 256 * 256; }
    std::vector<uint32_t> h(cur / 4, 0u);
    auto W = [&](int plane) { return h.data() + offs[plane] / 4; };
    for (uint32_t t = 0; t < n_tri; ++t) {
        uint32_t pos[9], nrm[9];
        for (int v = 0; v < 3; ++v)
            for (int i = 0; i < 3; ++i) { pos[3 * v + i] = corners[3 * t + v][i]; nrm[3 * v + i] = corners[3 * t + v][3 + i]; }
        for (int j = 0; j < 4; ++j) { W(0)[4 * t + j] = pos[j]; W(1)[4 * t + j] = pos[4 + j]; W(5)[4 * t + j] = nrm[j]; W(6)[4 * t + j] = nrm[4 + j]; }
        W(2)[t] = pos[8]; W(7)[t] = nrm[8];
        for (int v = 0; v < 2; ++v) { W(3)[4 * t + 2 * v] = corners[3 * t + v][10]; W(3)[4 * t + 2 * v + 1] = corners[3 * t + v][11]; }
        W(4)[2 * t] = corners[3 * t + 2][10]; W(4)[2 * t + 1] = corners[3 * t + 2][11];
        for (int v = 0; v < 3; ++v)
            for (int i = 0; i < 4; ++i) W(8 + v)[4 * t + i] = corners[3 * t + v][6 + i];
    }
    CK(hipMalloc(&d.mem, cur));
    CK(hipMemcpy(d.mem, h.data(), cur, hipMemcpyHostToDevice));
    char* b = (char*)d.mem;
    d.tp.A0 = (const float4*)(b + offs[0]); d.tp.A1 = (const float4*)(b + offs[1]); d.tp.A2 = (const float*)(b + offs[2]);
    d.tp.B0 = (const float4*)(b + offs[3]); d.tp.B1 = (const float2*)(b + offs[4]);
    d.tp.C0 = (const float4*)(b + offs[5]); d.tp.C1 = (const float4*)(b + offs[6]); d.tp.C2 = (const float*)(b + offs[7]);
    d.tp.D0 = (const float4*)(b + offs[8]); d.tp.D1 = (const float4*)(b + offs[9]); d.tp.D2 = (const float4*)(b + offs[10]);
    return true;
}
// a corner in the table's row order: p.xyz u | n.xyz v | t.xyzw
Key row_of(const Key& c) { return Key{ c[0], c[1], c[2], c[10], c[3], c[4], c[5], c[11], c[6], c[7], c[8], c[9] }; }

struct Run { uint32_t rows = 0; bool eligible = false; std::vector<Key> table; std::vector<VtIds> ids; };
bool dedup_once(const TriPlanes& tp, uint32_t n_tri, uint32_t id_limit, uint32_t min_sharing, Run& r) {
    VtWork w;
    m2s_host::DevBuf<float4> rows;
    m2s_host::DevBuf<VtIds> ids;
    CK(vt_dedup_begin(tp, n_tri, w, nullptr));
    CK(vt_dedup_finish(tp, n_tri, w, id_limit, min_sharing, rows, ids, &r.rows, &r.eligible, nullptr));
    if (w.mem != nullptr) { std::printf("{\"error\": \"temporaries not released\"}\n"); return false; }
    if (!r.eligible) return rows.get() == nullptr && ids.get() == nullptr;
    r.table.resize(r.rows);
    r.ids.resize(n_tri);
    CK(hipMemcpy(r.table.data(), rows.get(), (size_t)r.rows * sizeof(Key), hipMemcpyDeviceToHost));
    CK(hipMemcpy(r.ids.data(), ids.get(), (size_t)n_tri * sizeof(VtIds), hipMemcpyDeviceToHost));
    return true;
}

// expect_table: the case must be eligible under (id_limit, min_sharing); otherwise it must not be
bool run_case(const char* name, const std::vector<Key>& corners, uint32_t id_limit, uint32_t min_sharing, bool expect_table) {
    const uint32_t n_tri = (uint32_t)(corners.size() / 3);
    DevPlanes d;
    if (!upload(corners, n_tri, d)) return false;
    // reference: keys numbered in the order of their first corner
    std::map<Key, uint32_t> seen;
    std::vector<uint32_t> want(corners.size());
    for (size_t c = 0; c < corners.size(); ++c) want[c] = seen.emplace(row_of(corners[c]), (uint32_t)seen.size()).first->second;
    const uint32_t U = (uint32_t)seen.size();
    Run a, b;
    if (!dedup_once(d.tp, n_tri, id_limit, min_sharing, a) || !dedup_once(d.tp, n_tri, id_limit, min_sharing, b)) return false;
    size_t bad_row = 0, bad_id = 0;
    bool same = a.rows == b.rows && a.eligible == b.eligible;
    if (a.eligible && a.rows == U) {
        for (size_t c = 0; c < corners.size(); ++c) {
            uint32_t id[3];
            vt_unpack(a.ids[c / 3], id[0], id[1], id[2]);
            const uint32_t got = id[c % 3];
            if (got != want[c]) ++bad_id;
            if (got >= a.rows || a.table[got] != row_of(corners[c])) ++bad_row;
        }
        same = same && a.table == b.table && a.ids.size() == b.ids.size() && std::memcmp(a.ids.data(), b.ids.data(), a.ids.size() * sizeof(VtIds)) == 0;
    }
    const bool ok = a.rows == U && a.eligible == expect_table && a.eligible == vt_rows_ok(U, corners.size(), id_limit, min_sharing) && bad_row == 0 &&
                    bad_id == 0 && same;
    std::printf("{\"case\": \"%s\", \"triangles\": %u, \"hash_words\": %u, \"rows\": %u, \"rows_ref\": %u, \"eligible\": %s, \"bad_rows\": %zu, "
                "\"ids_out_of_order\": %zu, \"runs_equal\": %s, \"ok\": %s}\n",
                name, n_tri, vt_hash_words(3 * n_tri), a.rows, U, a.eligible ? "true" : "false", bad_row, bad_id, same ? "true" : "false", ok ? "true" : "false");
    return ok;
}

uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
Key corner(float x, float y, float z, float u, float v) {
    return Key{ fbits(x), fbits(y), fbits(z), fbits(0.0f), fbits(0.0f), fbits(1.0f), fbits(1.0f), fbits(0.0f), fbits(0.0f), fbits(1.0f), fbits(u), fbits(v) };
}
// a grid of (n + 1)^2 shared vertices, 2 n^2 triangles
std::vector<Key> grid(uint32_t n) {
    std::vector<Key> c;
    auto at = [&](uint32_t i, uint32_t j) { return corner((float)i, (float)j, 0.25f * (float)((i * 7u + j * 3u) % 5u), (float)i / (float)n, (float)j / (float)n); };
    for (uint32_t j = 0; j < n; ++j)
        for (uint32_t i = 0; i < n; ++i) {
            c.push_back(at(i, j)); c.push_back(at(i + 1, j)); c.push_back(at(i + 1, j + 1));
            c.push_back(at(i, j)); c.push_back(at(i + 1, j + 1)); c.push_back(at(i, j + 1));
        }
    return c;
}
std::vector<Key> soup(uint32_t n_tri) {   // no two corners alike
    std::vector<Key> c;
    for (uint32_t k = 0; k < 3 * n_tri; ++k) c.push_back(corner((float)k, (float)(k % 17u), (float)(k % 5u), 0.001f * (float)k, 0.5f));
    return c;
}
}  // namespace

int main(int argc, char** argv) {
    bool ok = true;
    if (argc > 1) {   // the caller's mesh (cube_sphere(4))
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f) { std::printf("{\"error\": \"cannot open %s\"}\n", argv[1]); return 2; }
        std::vector<Key> c;
        Key k;
        while (std::fread(k.data(), 4, 12, f) == 12) c.push_back(k);
        std::fclose(f);
        if (c.empty() || c.size() % 3) { std::printf("{\"error\": \"%s: not whole triangles\"}\n", argv[1]); return 2; }
        ok = run_case("file", c, kVtIdLimit, kVtMinSharing, true) && ok;
    }
    ok = run_case("grid_8", grid(8), kVtIdLimit, kVtMinSharing, true) && ok;
    // no sharing at all: U = corners, over the sharing threshold
    ok = run_case("soup_300_no_sharing", soup(300), kVtIdLimit, kVtMinSharing, false) && ok;
    {   // every corner the same vertex: one slot under full contention
        std::vector<Key> c(600, corner(1.0f, 2.0f, 3.0f, 0.25f, 0.75f));
        ok = run_case("one_vertex_200_triangles", c, kVtIdLimit, kVtMinSharing, true) && ok;
    }
    {   // rows that differ only in the sign of a zero and in a NaN's payload: 4 distinct rows among 12 corners
        Key z = corner(0.0f, 1.0f, 2.0f, 0.5f, 0.5f), nz = z, n1 = z, n2 = z;
        nz[0] = 0x80000000u;                          // -0.0
        n1[1] = 0x7FC00001u; n2[1] = 0x7FC00002u;     // two quiet NaNs
        std::vector<Key> c = { z, nz, n1, n2, z, nz, n1, n2, n2, n1, nz, z };
        ok = run_case("signed_zero_and_nan_payload", c, kVtIdLimit, kVtMinSharing, true) && ok;
        if (std::map<Key, int>{ { row_of(z), 0 }, { row_of(nz), 0 }, { row_of(n1), 0 }, { row_of(n2), 0 } }.size() != 4) ok = false;
    }
    {   // one triangle, its corners distinct: 3 rows of 3 corners pass only a sharing threshold of 1
        std::vector<Key> c = { corner(0, 0, 0, 0, 0), corner(1, 0, 0, 1, 0), corner(0, 1, 0, 0, 1) };
        ok = run_case("one_triangle", c, kVtIdLimit, 1u, true) && ok;
    }
    // corner counts on both sides of a hash-table size boundary: 510 corners -> 1024 words, 513 corners -> 2048 words
    if (vt_hash_words(510) != 1024u || vt_hash_words(513) != 2048u) { std::printf("{\"error\": \"hash table sizes\"}\n"); ok = false; }
    {
        std::vector<Key> g = grid(10);                // 200 triangles
        std::vector<Key> a(g.begin(), g.begin() + 510), b(g.begin(), g.begin() + 513);
        ok = run_case("hash_boundary_below", a, kVtIdLimit, kVtMinSharing, true) && ok;
        ok = run_case("hash_boundary_above", b, kVtIdLimit, kVtMinSharing, true) && ok;
    }
    // the two "not eligible" exits with small limits: grid(8) has 81 rows among 384 corners
    ok = run_case("id_limit_reached", grid(8), 81u, kVtMinSharing, false) && ok;       // rows must be BELOW the limit
    ok = run_case("id_limit_not_reached", grid(8), 82u, kVtMinSharing, true) && ok;
    ok = run_case("sharing_too_low", grid(8), kVtIdLimit, 5u, false) && ok;            // 81 * 5 > 384
    ok = run_case("sharing_just_enough", grid(8), kVtIdLimit, 4u, true) && ok;         // 81 * 4 <= 384
    std::printf("{\"all_ok\": %s}\n", ok ? "true" : "false");
    return ok ? 0 : 1;
}
