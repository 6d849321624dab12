// recstate_sh_check.cpp — the two transitions m2s_set_carry_sh adds to mesh2splat_amd/csrc/m2s_recstate.h, Rewrite::MergeWithSh and
// Rewrite::LodCutWithSh, against their rows of the header's table: each is its plain form (Merge, LodCut) in every cell but the SH
// plane's, which is retagged for the new records and loses its tap counts as after PruneWithSh.  Built with the host compiler under
// AddressSanitizer + UBSan (tests/test_recstate_sh_cpu.py); needs no HIP header and no runtime; exits non-zero at the first failure.
#include "../../mesh2splat_amd/csrc/m2s_recstate.h"

#include <cstdio>
#include <cstdlib>

using namespace m2s_host;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

char g_mem[4][64];                        // addresses to stand for record buffers: [0] the old records, [1] the pool
const uint32_t g_perm[4] = { 3, 1, 0, 2 };
constexpr uint64_t kN = 40;

// every dependent set, for kN records at g_mem[0], R = 8, converted at 64 before m2s_records_to_world_units
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
    s.merge_map_tag.set(s, 100);
    s.lod_ids_tag.set(s, kN);
    s.sh_tag.set(s, kN);
    s.bake_has_counts = true;
    return s;
}

bool same(const RecordsTag& a, const RecordsTag& b) { return a.of == b.of && a.n == b.n && a.epoch == b.epoch; }

// everything but the plane and its counts: `with` must be what `plain` is
void same_but_the_plane(const RecordState& with, const RecordState& plain) {
    CHECK(with.last_records == plain.last_records && with.last_total == plain.last_total && with.last_stored == plain.last_stored);
    CHECK(with.last_R == plain.last_R && with.conv_R == plain.conv_R && with.records_stale == plain.records_stale);
    CHECK(with.records_epoch == plain.records_epoch);
    CHECK(with.sorted_n == plain.sorted_n && with.pp_visible == plain.pp_visible && with.sq_n == plain.sq_n && with.sq_src == plain.sq_src);
    CHECK(same(with.pos_plane_tag, plain.pos_plane_tag) && same(with.sq_src_tag, plain.sq_src_tag) && same(with.contrib_tag, plain.contrib_tag));
    CHECK(same(with.refit_tag, plain.refit_tag) && same(with.merge_map_tag, plain.merge_map_tag) && same(with.lod_ids_tag, plain.lod_ids_tag));
}

void rows() {
    const RecordState was = established();

    // MergeWithSh | pool n n R  keep(conv_R) 0 +1 | keep 0 0 0 0 keep 0(contrib) 0(refit) keep keep tag 0
    RecordState s = was, plain = was;
    s.rewritten(g_mem[1], 12, 8, Rewrite::MergeWithSh);
    plain.rewritten(g_mem[1], 12, 8, Rewrite::Merge);
    same_but_the_plane(s, plain);
    CHECK(s.last_records == g_mem[1] && s.last_total == 12 && s.last_stored == 12 && s.last_R == 8 && s.conv_R == 64 && !s.records_stale);
    CHECK(s.records_epoch == was.records_epoch + 1);
    CHECK(s.sorted_n == 0 && s.pp_visible == 0 && s.sq_n == 0 && s.sq_src == nullptr);
    CHECK(!s.contrib_tag.is_set() && !s.refit_tag.is_set());
    CHECK(same(s.pos_plane_tag, was.pos_plane_tag) && !s.pos_plane_tag.holds(s));             // kept, and no longer holding
    CHECK(same(s.merge_map_tag, was.merge_map_tag) && same(s.lod_ids_tag, was.lod_ids_tag));
    CHECK(s.sh_tag.holds(s, 12) && !s.sh_tag.holds(s, kN) && !s.bake_has_counts);
    CHECK(!plain.sh_tag.is_set() && plain.bake_has_counts);                                   // (the plain form: dropped, the flag kept)

    // LodCutWithSh | pool n n R keep(conv_R) 0 +1 | keep 0 0 0 0 keep 0(contrib) keep(refit) keep keep tag 0
    s = was; plain = was;
    s.rewritten(g_mem[1], 17, 32, Rewrite::LodCutWithSh);
    plain.rewritten(g_mem[1], 17, 32, Rewrite::LodCut);
    same_but_the_plane(s, plain);
    CHECK(s.last_records == g_mem[1] && s.last_total == 17 && s.last_stored == 17 && s.last_R == 32 && s.conv_R == 64 && !s.records_stale);
    CHECK(s.records_epoch == was.records_epoch + 1);
    CHECK(s.sorted_n == 0 && s.pp_visible == 0 && s.sq_n == 0 && s.sq_src == nullptr);
    CHECK(!s.contrib_tag.is_set() && same(s.refit_tag, was.refit_tag) && !s.refit_tag.holds(s));
    CHECK(s.sh_tag.holds(s, 17) && !s.bake_has_counts);
    CHECK(!plain.sh_tag.is_set() && plain.bake_has_counts);

    // no plane before: the transition still tags one (the caller only uses it where it has made the rows)
    RecordState bare = was;
    bare.sh_tag.clear();
    bare.bake_has_counts = false;
    bare.rewritten(g_mem[1], 0, 8, Rewrite::LodCutWithSh);                                    // zero selected records: an empty plane, valid
    CHECK(bare.sh_tag.is_set() && bare.sh_tag.holds(bare, 0) && !bare.sh_tag.holds(bare, 1) && !bare.bake_has_counts);

    // in place (the pool was the source): the new tag holds, the tag of the members does not
    s = was;
    const RecordsTag members = s.sh_tag;
    s.rewritten(g_mem[0], kN, 8, Rewrite::MergeWithSh);
    CHECK(s.sh_tag.holds(s, kN) && !members.holds(s));

    // what follows drops the plane again as it always did
    s.rewritten(g_mem[0], kN, 8, Rewrite::RefitApply);
    CHECK(!s.sh_tag.is_set());
    s = was; s.rewritten(g_mem[1], 12, 8, Rewrite::MergeWithSh); s.rewritten(g_mem[1], 12, 1, Rewrite::WorldUnits);
    CHECK(!s.sh_tag.is_set());
    s = was; s.rewritten(g_mem[1], 12, 8, Rewrite::MergeWithSh); s.rewritten(g_mem[1], 5, 8, Rewrite::Prune);
    CHECK(s.sh_tag.is_set() && !s.sh_tag.holds(s));                                           // (Prune keeps the tag it found: it no longer holds)
}

}  // namespace

int main() {
    rows();
    std::printf("recstate_sh_check ok\n");
    return 0;
}
