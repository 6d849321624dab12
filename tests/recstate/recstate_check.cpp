// recstate_check.cpp — the record state of mesh2splat_amd/csrc/m2s_recstate.h: every transition driven from a state in which every
// dependent is set, every cell of the header's table asserted; and what RecordsTag::holds() answers.  Built with the host compiler under
// AddressSanitizer + UBSan (tests/test_recstate_cpu.py); needs no HIP header and no runtime; exits non-zero at the first failure.
#include "../../mesh2splat_amd/csrc/m2s_recstate.h"

#include <cstdio>
#include <cstdlib>

using namespace m2s_host;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

char g_mem[8][64];                        // addresses to stand for record buffers: [0] the old records, [1] the pool, [2..] others
const uint32_t g_perm[4] = { 3, 1, 0, 2 };
constexpr uint64_t kN = 40;               // the established records

// every dependent set, for kN records at g_mem[0], R = 8, converted at 64 before m2s_records_to_world_units (so conv_R is set too)
RecordState established() {
    RecordState s;
    s.records_adopted(g_mem[0], kN, 8);
    s.conv_R = 64;
    s.pos_plane_tag.set(s, kN);
    s.sorted_n = kN;
    s.pp_visible = 31;
    s.sq_n = 29;
    s.sq_src = g_perm;
    s.sq_src_tag.set(s, kN);
    s.contrib_tag.set(s, kN);
    s.refit_tag.set(s, kN);
    s.merge_map_tag.set(s, 100);          // (n: the records before the merge)
    s.lod_ids_tag.set(s, kN);
    s.sh_tag.set(s, kN);
    s.bake_has_counts = true;
    return s;
}

RecordsTag* const* tags_of(RecordState& s) {
    static RecordsTag* t[7];
    t[0] = &s.pos_plane_tag; t[1] = &s.sq_src_tag; t[2] = &s.contrib_tag; t[3] = &s.refit_tag; t[4] = &s.merge_map_tag; t[5] = &s.lod_ids_tag;
    t[6] = &s.sh_tag;
    return t;
}

bool same(const RecordsTag& a, const RecordsTag& b) { return a.of == b.of && a.n == b.n && a.epoch == b.epoch; }

// the cells of one row: the records, then "keep" (bit-identical to the established state) or not per dependent
struct Row {
    const void* ptr; uint64_t total, stored; uint32_t R, conv_R; bool stale; uint64_t epoch_step;
    bool counts_kept;                     // sorted_n, pp_visible, sq_n
    bool src_kept;                        // sq_src
    bool contrib_kept, refit_kept, sh_kept, sh_retagged, bake_counts;
};

void check_row(const RecordState& was, RecordState& now, const Row& r) {
    CHECK(now.last_records == r.ptr && now.last_total == r.total && now.last_stored == r.stored);
    CHECK(now.last_R == r.R && now.conv_R == r.conv_R && now.records_stale == r.stale);
    CHECK(now.records_epoch == was.records_epoch + r.epoch_step);
    // never touched by a transition: the position plane's tag, the sources' tag, the map, the node indices
    CHECK(same(now.pos_plane_tag, was.pos_plane_tag) && same(now.sq_src_tag, was.sq_src_tag));
    CHECK(same(now.merge_map_tag, was.merge_map_tag) && same(now.lod_ids_tag, was.lod_ids_tag));
    if (r.counts_kept) CHECK(now.sorted_n == was.sorted_n && now.pp_visible == was.pp_visible && now.sq_n == was.sq_n);
    else CHECK(now.sorted_n == 0 && now.pp_visible == 0 && now.sq_n == 0);
    CHECK(now.sq_src == (r.src_kept ? was.sq_src : nullptr));
    CHECK(r.contrib_kept ? same(now.contrib_tag, was.contrib_tag) : !now.contrib_tag.is_set());
    CHECK(r.refit_kept ? same(now.refit_tag, was.refit_tag) : !now.refit_tag.is_set());
    if (r.sh_retagged) CHECK(now.sh_tag.holds(now, r.stored));
    else CHECK(r.sh_kept ? same(now.sh_tag, was.sh_tag) : !now.sh_tag.is_set());
    CHECK(now.bake_has_counts == r.bake_counts);
    // whatever was kept: once the epoch has moved or the records are gone, nothing but a retagged plane holds for the current records
    if (r.epoch_step || !r.ptr) {
        RecordsTag* const* t = tags_of(now);
        for (int k = 0; k < 7; ++k) CHECK(!t[k]->holds(now) || (k == 6 && r.sh_retagged));
    }
}

void transitions() {
    const RecordState was = established();
    RecordState s = was;
    {   // before anything: every tag holds
        RecordsTag* const* t = tags_of(s);
        for (int k = 0; k < 7; ++k) CHECK(t[k]->is_set() && t[k]->holds(s));
        CHECK(s.contrib_tag.holds(s, kN) && !s.contrib_tag.holds(s, kN + 1) && !s.merge_map_tag.holds(s, kN));
    }
    //                                   ptr       total stored R  conv stale +epoch counts src   contrib refit sh     retag  taps
    s = was; s.conversion_started(16);
    check_row(was, s, Row{ g_mem[0], kN,   kN,    16, 0,  false, 0,   true,  true, true,   true, true,  false, true });
    {   // (the early write alone moves no epoch: everything still holds for the OLD records, now said to be at R = 16)
        RecordsTag* const* t = tags_of(s);
        for (int k = 0; k < 7; ++k) CHECK(t[k]->holds(s));
    }
    s.conversion_finished(g_mem[2], 300, 256);
    check_row(was, s, Row{ g_mem[2], 300,  256,   16, 0,  false, 1,   true,  true, true,   true, true,  false, true });
    s = was; s.records_stale = true; s.conversion_started(16);                  // (and it clears the flag of the records it has not replaced yet)
    CHECK(!s.records_stale && s.records_epoch == was.records_epoch);
    s = was; s.slot_adopted(g_mem[1], 70, 64, 12, false);
    check_row(was, s, Row{ g_mem[1], 70,   64,    12, 0,  false, 1,   true,  true, true,   true, true,  false, true });
    s = was; s.slot_adopted(g_mem[1], 70, 64, 12, true);
    check_row(was, s, Row{ g_mem[1], 70,   64,    12, 0,  true,  1,   true,  true, true,   true, true,  false, true });
    s = was; s.records_uploaded(g_mem[3], 9);
    check_row(was, s, Row{ g_mem[3], 9,    9,     0,  0,  false, 1,   false, true, true,   true, true,  false, true });
    s = was; s.records_adopted(g_mem[4], 11, 5);
    check_row(was, s, Row{ g_mem[4], 11,   11,    5,  0,  false, 1,   false, true, true,   true, true,  false, true });
    s = was; s.records_stale = true; s.scene_replaced();
    check_row(was, s, Row{ nullptr,  0,    0,     8,  64, false, 1,   true,  true, true,   true, true,  false, true });
    s = was; s.pool_released(g_mem[1]);                                         // (another buffer: nothing happens)
    check_row(was, s, Row{ g_mem[0], kN,   kN,    8,  64, false, 0,   true,  true, true,   true, true,  false, true });
    s.pool_released(nullptr);
    check_row(was, s, Row{ g_mem[0], kN,   kN,    8,  64, false, 0,   true,  true, true,   true, true,  false, true });
    s.pool_released(g_mem[0]);
    check_row(was, s, Row{ nullptr,  kN,   0,     8,  64, false, 0,   true,  true, true,   true, true,  false, true });
    s = was; s.rewritten(g_mem[1], 30, 8, Rewrite::Prune);
    check_row(was, s, Row{ g_mem[1], 30,   30,    8,  64, false, 1,   false, false, false, true, true,  false, true });
    s = was; s.rewritten(g_mem[1], 30, 8, Rewrite::PruneWithSh);
    check_row(was, s, Row{ g_mem[1], 30,   30,    8,  64, false, 1,   false, false, false, true, false, true,  false });
    s = was; s.rewritten(g_mem[1], kN, 8, Rewrite::RefitApply);
    check_row(was, s, Row{ g_mem[1], kN,   kN,    8,  64, false, 1,   false, false, false, false, false, false, true });
    s = was; s.rewritten(g_mem[1], 12, 8, Rewrite::Merge);
    check_row(was, s, Row{ g_mem[1], 12,   12,    8,  64, false, 1,   false, false, false, false, false, false, true });
    s = was; s.rewritten(g_mem[1], 17, 32, Rewrite::LodCut);
    check_row(was, s, Row{ g_mem[1], 17,   17,    32, 64, false, 1,   false, false, false, true, false, false, true });
    s = was; s.rewritten(g_mem[1], kN, 1, Rewrite::WorldUnits);                 // (conv_R set already: kept)
    check_row(was, s, Row{ g_mem[1], kN,   kN,    1,  64, false, 1,   false, false, false, false, false, false, true });
    RecordState fresh = was;
    fresh.conv_R = 0;
    s = fresh; s.rewritten(g_mem[1], kN, 1, Rewrite::WorldUnits);               // (a conversion's records: the R they had goes to conv_R)
    check_row(fresh, s, Row{ g_mem[1], kN,  kN,    1,  8,  false, 1,   false, false, false, false, false, false, true });
    s = was; s.records_stale = true; s.rewritten(g_mem[0], kN, 8, Rewrite::Prune);   // (in place, and stale before: the flag goes)
    check_row(was, s, Row{ g_mem[0], kN,   kN,    8,  64, false, 1,   false, false, false, true, true,  false, true });
}

void holds() {
    // false after an epoch bump, a pointer change, a count change, stale
    RecordState s = established();
    RecordsTag t;
    CHECK(!t.is_set() && !t.holds(s));
    t.set(s, kN);
    CHECK(t.is_set() && t.holds(s) && t.holds(s, kN));
    RecordState bumped = s;
    bumped.records_adopted(s.last_records, s.last_stored, s.last_R);            // the same address, the same count: only the epoch moved
    CHECK(bumped.last_records == s.last_records && !t.holds(bumped) && !t.holds(bumped, kN));
    RecordState moved = s;
    moved.pool_released(g_mem[0]);                                              // the pointer alone (no epoch bump)
    CHECK(moved.records_epoch == s.records_epoch && !t.holds(moved));
    CHECK(!t.holds(s, kN - 1));                                                 // a count that is not the tag's
    RecordState stale = s;
    stale.slot_adopted(s.last_records, s.last_total, s.last_stored, s.last_R, true);   // the only way the flag is ever raised
    CHECK(stale.records_stale && stale.last_records == s.last_records && !t.holds(stale));
    t.clear();
    CHECK(!t.is_set() && !t.holds(s));

    // a tag set on the caller's records (epoch 0) never holds for the context's, not even at the same address
    RecordsTag f;
    f.set_foreign(g_mem[0], kN);
    CHECK(f.is_set() && f.epoch == 0 && !f.holds(s) && !f.holds(s, kN));
    RecordState first;                                                          // a context that has seen no records yet
    CHECK(first.records_epoch >= 1);
    first.records_adopted(g_mem[0], kN, 1);
    CHECK(!f.holds(first));
    for (int k = 0; k < 1000; ++k) { first.records_adopted(g_mem[0], kN, 1); CHECK(!f.holds(first)); }

    // the pool reallocated under the current records, then an adoption at the SAME address: every old tag stays invalid
    RecordState p = established();
    const RecordState before = p;
    p.pool_released(g_mem[0]);
    {
        RecordsTag* const* ts = tags_of(p);
        for (int k = 0; k < 7; ++k) CHECK(ts[k]->is_set() && !ts[k]->holds(p));
    }
    p.conversion_finished(g_mem[0], kN, kN);
    CHECK(p.last_records == before.last_records && p.last_stored == before.last_stored);
    {
        RecordsTag* const* ts = tags_of(p);
        for (int k = 0; k < 7; ++k) CHECK(ts[k]->is_set() && !ts[k]->holds(p) && !ts[k]->holds(p, kN));
    }
    p = before; p.pool_released(g_mem[0]); p.records_adopted(g_mem[0], kN, 8);
    {
        RecordsTag* const* ts = tags_of(p);
        for (int k = 0; k < 7; ++k) CHECK(!ts[k]->holds(p));
    }
    p = before; p.pool_released(g_mem[0]); p.rewritten(g_mem[0], kN, 8, Rewrite::Prune);
    {
        RecordsTag* const* ts = tags_of(p);
        for (int k = 0; k < 7; ++k) CHECK(!ts[k]->holds(p));
    }
}

}  // namespace

int main() {
    transitions();
    holds();
    std::printf("recstate_check ok\n");
    return 0;
}
