// lodtree_check.cpp — LodTree and LodWork of mesh2splat_amd/csrc/m2s_lodtree.h against a malloc-backed stand-in for the runtime, built with
// the host compiler under AddressSanitizer + UBSan (tests/test_lodtree_cpu.py).  Links no HIP runtime; exits non-zero at the first
// failure.  Every "device" block is exactly as large as it was asked for, so ASan judges each kept-row copy against the planes' sizes.
#include "../../mesh2splat_amd/csrc/m2s_lodtree.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

namespace {
std::map<void*, size_t> g_live;          // every live "device" block and its size
long g_frees = 0, g_copies = 0, g_syncs = 0;
int g_fail_after = -1;                   // armed (>= 0): the allocation after this many more fails, once

hipStream_t const kStream = nullptr;
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_fail_after >= 0 && g_fail_after-- == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes);
    g_live[*p] = bytes;
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (!p) return hipSuccess;
    if (!g_live.erase(p)) { std::fprintf(stderr, "free of a block that is not live (double free?)\n"); std::exit(3); }
    std::free(p);
    ++g_frees;
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) { std::memcpy(dst, src, bytes); ++g_copies; return hipSuccess; }
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) { std::memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { ++g_syncs; return hipSuccess; }
}

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

using namespace m2s_host;

static const size_t kRow[kLodPlanes] = { 96, 4, 16, 192 };

// a fill pattern of its own per plane: byte i of plane w
static unsigned char pattern(uint32_t w, size_t i) { return (unsigned char)(i * (2 * w + 3) + 17 * w + 1); }
static void fill(const LodTree& t, uint32_t w, uint64_t rows) {
    unsigned char* p = t.rows<unsigned char>(w);
    for (size_t i = 0; i < rows * kRow[w]; ++i) p[i] = pattern(w, i);
}
static bool intact(const LodTree& t, uint32_t w, uint64_t rows) {
    const unsigned char* p = t.rows<unsigned char>(w);
    for (size_t i = 0; i < rows * kRow[w]; ++i)
        if (p[i] != pattern(w, i)) return false;
    return true;
}
// every plane the tree has is a live block of exactly capacity x row size
static bool exact(const LodTree& t, uint32_t planes) {
    for (uint32_t w = 0; w < planes; ++w)
        if (!t.rows<void>(w) || g_live.at(t.rows<void>(w)) != t.cap(w) * kRow[w]) return false;
    return true;
}

static void check_first_reservation() {
    std::string err;
    for (uint32_t w = 0; w < kLodPlanes; ++w) CHECK(LodTree::row_bytes(w) == kRow[w]);
    {
        LodTree t;
        CHECK(t.reserve(err, kStream, 100, 0, false) == M2S_OK && err.empty());
        for (uint32_t w = 0; w < 3; ++w) CHECK(t.cap(w) == 100);                        // max(want, 2 * 0, 1)
        CHECK(exact(t, 3) && g_live.size() == 3 && !t.rows<void>(kLodSh) && t.cap(kLodSh) == 0);
        CHECK(g_copies == 0 && g_syncs == 0);                                           // nothing kept: nothing copied or waited for
        for (uint32_t w = 0; w < 3; ++w) fill(t, w, 100);
        void* const nodes = t.rows<void>(kLodRecords);
        CHECK(t.reserve(err, kStream, 100, 100, false) == M2S_OK && t.rows<void>(kLodRecords) == nodes && g_frees == 0);   // large enough: kept
    }
    CHECK(g_live.empty());
    {
        LodTree t;                                                                      // a tree of no nodes still gets planes to point at
        CHECK(t.reserve(err, kStream, 0, 0, true) == M2S_OK);
        for (uint32_t w = 0; w < kLodPlanes; ++w) CHECK(t.cap(w) == 1 && t.rows<void>(w));
    }
    CHECK(g_live.empty());
}

// three successive growths with kept nodes, without and with the SH plane
static void check_growth(bool sh) {
    std::string err;
    const uint32_t planes = sh ? 4 : 3;
    {
        LodTree t;
        CHECK(t.reserve(err, kStream, 100, 0, sh) == M2S_OK && g_live.size() == planes);
        if (sh) CHECK(t.cap(kLodSh) == 100);                                            // max(want, the node planes' capacity, 1)
        const uint64_t want[3] = { 150, 450, 451 }, keep[3] = { 100, 180, 450 }, cap[3] = { 200, 450, 900 };   // max(want, 2 * cap, 1)
        for (int g = 0; g < 3; ++g) {
            for (uint32_t w = 0; w < planes; ++w) fill(t, w, keep[g]);
            void* old[kLodPlanes];
            for (uint32_t w = 0; w < planes; ++w) old[w] = t.rows<void>(w);
            const long frees = g_frees, copies = g_copies, syncs = g_syncs;
            CHECK(t.reserve(err, kStream, want[g], keep[g], sh) == M2S_OK);
            CHECK(g_frees == frees + planes && g_copies == copies + planes && g_syncs == syncs + 1);   // each old block once; one synchronise
            for (uint32_t w = 0; w < planes; ++w) {
                CHECK(t.cap(w) == cap[g] && !g_live.count(old[w]) && intact(t, w, keep[g]));
                fill(t, w, cap[g]);                                                     // the whole new block is the plane's
            }
            CHECK(exact(t, planes) && g_live.size() == planes);
        }
        CHECK(err.empty());
    }
    CHECK(g_live.empty());
}

// a tree reserved without a plane, then with one: while the node planes stay, and while they grow
static void check_plane_added() {
    std::string err;
    for (uint64_t want : { 100, 300 }) {
        LodTree t;
        CHECK(t.reserve(err, kStream, 100, 0, false) == M2S_OK);
        for (uint32_t w = 0; w < 3; ++w) fill(t, w, 100);
        void* const nodes = t.rows<void>(kLodRecords);
        CHECK(t.reserve(err, kStream, want, 80, true) == M2S_OK);
        CHECK((t.rows<void>(kLodRecords) == nodes) == (want == 100));
        CHECK(t.cap(kLodRecords) == (want == 100 ? 100u : 300u) && t.cap(kLodSh) >= t.cap(kLodRecords) && exact(t, 4) && g_live.size() == 4);
        for (uint32_t w = 0; w < 3; ++w) CHECK(intact(t, w, 80));
        fill(t, kLodSh, t.cap(kLodSh));
    }
    CHECK(g_live.empty());
}

// an allocation failure at each of the four allocations of a growth in turn
static void check_failed_allocation() {
    std::string err;
    for (int k = 0; k < 4; ++k) {
        LodTree t;
        CHECK(t.reserve(err, kStream, 100, 0, true) == M2S_OK);
        void* old[kLodPlanes];
        for (uint32_t w = 0; w < kLodPlanes; ++w) { fill(t, w, 100); old[w] = t.rows<void>(w); }
        err.clear();
        g_fail_after = k;
        CHECK(t.reserve(err, kStream, 1000, 100, true) == M2S_ERR_OOM && !err.empty() && g_fail_after < 0);
        for (uint32_t w = 0; w < kLodPlanes; ++w) CHECK(t.rows<void>(w) == old[w] && t.cap(w) == 100 && intact(t, w, 100));
        CHECK(g_live.size() == 4);                                                      // what the failed call had allocated is gone again
        CHECK(t.reserve(err, kStream, 1000, 100, true) == M2S_OK && exact(t, 4));
        for (uint32_t w = 0; w < kLodPlanes; ++w) CHECK(t.cap(w) == 1000 && intact(t, w, 100));
    }
    {
        LodTree t;                                                                      // ... and of a first reservation: still empty
        g_fail_after = 1;
        CHECK(t.reserve(err, kStream, 100, 0, false) == M2S_ERR_OOM && g_live.empty() && !t.rows<void>(kLodRecords) && t.cap(kLodRecords) == 0);
        CHECK(t.reserve(err, kStream, 100, 0, false) == M2S_OK && exact(t, 3));
    }
    CHECK(g_live.empty());
}

struct Bound { float x, y, z, edge; };
struct LevelsK { const Bound* bounds; const uint32_t* parent; const uint64_t* first; uint32_t levels; };

static void check_end_and_release() {
    std::string err;
    LodTree t;
    CHECK(t.levels == 0 && t.nodes() == 0 && t.gen == 0);
    for (uint32_t w = 0; w < kLodPlanes; ++w) CHECK(t.plane(w) == nullptr);
    CHECK(t.reserve(err, kStream, 100, 0, true) == M2S_OK);
    for (uint32_t w = 0; w < kLodPlanes; ++w) CHECK(t.plane(w) == nullptr);             // planes, but no tree yet
    const uint64_t first[4] = { 0, 60, 90, 100 };
    t.commit(3, first, 128, false, 0, M2S_MERGE_MODEL_GAUSSIAN, 2.5f);
    CHECK(t.levels == 3 && t.nodes() == 100 && t.R == 128 && !t.has_sh && t.model == M2S_MERGE_MODEL_GAUSSIAN && t.sigma == 2.5f);
    for (uint32_t l = 0; l < M2S_LOD_MAX_STEPS + 2; ++l) CHECK(t.first[l] == first[l < 3 ? l : 3]);
    for (uint32_t w = 0; w < 3; ++w) CHECK(t.plane(w) == t.rows<void>(w) && t.plane(w) && g_live.at(t.rows<void>(w)) >= t.nodes() * LodTree::row_bytes(w));
    CHECK(t.plane(kLodSh) == nullptr);                                                  // a block, but not this tree's
    const LevelsK k = t.levels_k<LevelsK>();
    CHECK(k.bounds == t.plane(kLodBounds) && k.parent == t.plane(kLodParent) && k.first == t.first && k.levels == 3);
    t.commit(3, first, 128, true, 3, M2S_MERGE_MODEL_FOOTPRINT, 1.0f);
    CHECK(t.plane(kLodSh) == t.rows<void>(kLodSh) && t.plane(kLodSh) && t.sh_degree == 3);
    const uint64_t none[2] = { 0, 0 };
    t.commit(1, none, 1, true, 3, M2S_MERGE_MODEL_FOOTPRINT, 1.0f);                     // a tree of no nodes hands out no plane
    for (uint32_t w = 0; w < kLodPlanes; ++w) CHECK(t.nodes() == 0 && t.plane(w) == nullptr);
    t.commit(3, first, 128, true, 3, M2S_MERGE_MODEL_FOOTPRINT, 1.0f);

    t.end();
    CHECK(t.levels == 0 && t.gen == 1 && !t.has_sh && t.nodes() == 0 && g_live.size() == 4 && t.cap(kLodRecords) == 100);
    for (uint32_t w = 0; w < kLodPlanes; ++w) CHECK(t.plane(w) == nullptr);
    t.end();
    CHECK(t.levels == 0 && t.gen == 2 && g_live.size() == 4);
    t.drop_sh();
    CHECK(g_live.size() == 3 && t.cap(kLodSh) == 0);
    t.commit(3, first, 128, false, 0, M2S_MERGE_MODEL_FOOTPRINT, 1.0f);
    t.release();
    CHECK(t.levels == 0 && t.gen == 3 && g_live.empty());
    for (uint32_t w = 0; w < kLodPlanes; ++w) CHECK(t.cap(w) == 0 && !t.rows<void>(w) && t.plane(w) == nullptr);
    t.release();
    CHECK(t.gen == 4 && g_live.empty());
    CHECK(t.reserve(err, kStream, 10, 0, false) == M2S_OK && g_live.size() == 3);       // released, not broken
}

static void check_work() {
    std::string err;
    RecordState cur;
    cur.records_adopted(&cur, 5, 1);
    LodWork w;
    CHECK(w.open.reserve(err, 300, 1) == M2S_OK && w.vis.reserve(err, 300, 1) == M2S_OK && w.lh.reserve(err, 300, 8) == M2S_OK);
    CHECK(w.occ_depth.reserve(err, 64, 4) == M2S_OK && w.blend_t.reserve(err, 64, 4) == M2S_OK);
    CHECK(w.counts.reserve(err, 64, 4) == M2S_OK && w.ids.reserve(err, 64, 4) == M2S_OK && w.budget_state.reserve(err, 64, 4) == M2S_OK);
    CHECK(w.blend_counts.reserve(err, 64, 4) == M2S_OK && g_live.size() == 9);
    w.blend_tag.set(cur, 5);
    w.ids_gen = 7;
    CHECK(w.blend_tag.holds(cur, 5));
    w.release_tree_sized();
    CHECK(g_live.size() == 4 && !w.open && !w.vis && !w.lh.get() && !w.occ_depth && !w.blend_t && !w.blend_tag.is_set());
    CHECK(w.counts && w.ids && w.budget_state && w.blend_counts && w.ids_gen == 7);     // what is kept
    w.release_tree_sized();
    CHECK(g_live.size() == 4);
}

int main() {
    check_first_reservation();
    check_growth(false);
    check_growth(true);
    check_plane_added();
    check_failed_allocation();
    check_end_and_release();
    CHECK(g_live.empty());
    check_work();
    CHECK(g_live.empty());
    std::puts("lodtree_check ok");
    return 0;
}
