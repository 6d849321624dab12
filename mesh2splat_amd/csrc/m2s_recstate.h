// m2s_recstate.h — the context's current records and everything whose validity hangs on them: one state type (RecordState, a base of
// m2s_ctx), one validity tag (RecordsTag), and the only code that says "these are the current records now" (the transitions below).
// <cstdint> only: tests/recstate/recstate_check.cpp builds it with the host compiler, no HIP header in sight.
#pragma once
#include <cstdint>

namespace m2s_host {
struct RecordState;

// "Valid for these records": what a pass leaves behind it tags with the records it was made of — address, count, the epoch they were
// current in.  holds() is the one validity test.  It does not read `stale`: the passes that tag refuse stale records, and the flag is
// only ever raised together with an epoch bump (slot_adopted), so a tag of the current epoch was not made of stale records.
// epoch 0 (set_foreign): made of records the CALLER passed, which are never the context's — the epochs start at 1.
struct RecordsTag {
    const void* of = nullptr;       // nullptr: not set (no pass has run, or the transition / the pass itself dropped what it left)
    uint64_t n = 0, epoch = 0;
    void clear() { of = nullptr; n = 0; epoch = 0; }
    inline void set(const RecordState& cur, uint64_t count);
    void set_foreign(const void* records, uint64_t count) { of = records; n = count; epoch = 0; }
    bool is_set() const { return of != nullptr; }
    inline bool holds(const RecordState& cur) const;
    bool holds(const RecordState& cur, uint64_t count) const { return holds(cur) && n == count; }
};

// What a pass that rewrites the records into the pool was (RecordState::rewritten): the columns of the table's last rows.
enum class Rewrite { Prune, PruneWithSh, RefitApply, Merge, LodCut, WorldUnits, MergeWithSh, LodCutWithSh };

struct RecordState {
    // ---- the current records
    const void* last_records = nullptr;
    uint64_t last_total = 0, last_stored = 0;
    uint32_t last_R = 0;            // resolutionTarget of the current records: the unit of their scales (0: uploaded, taken as 1)
    uint32_t conv_R = 0;            // after m2s_records_to_world_units (last_R == 1): the R they were converted at (converted_R); else 0
    bool records_stale = false;     // the conversion last waited for has been overwritten by a later submission
    uint64_t records_epoch = 1;     // advances whenever the records behind last_records may have changed
    // ---- what hangs on them.  A tag: valid for the records it names; a count: entries of a buffer derived from them (0: none)
    RecordsTag pos_plane_tag;       // the 16-byte position plane (d_pos_plane): left by a depth sort or by the sparse kernel
    uint64_t sorted_n = 0;          // m2s_sort_by_depth: records in d_sorted
    uint64_t pp_visible = 0;        // m2s_prepass: survivors in d_quads
    uint64_t sq_n = 0;              // sorted quads in d_sorted_quads
    const uint32_t* sq_src = nullptr;   // their sources (nullptr: absent): words of the sort's permutation, or d_sq_src
    RecordsTag sq_src_tag;          // ... and the records those index into
    RecordsTag contrib_tag;         // the contribution accumulators (set: m2s_contrib_begin has run)
    RecordsTag refit_tag;           // the refit accumulators (set: m2s_refit_begin has run)
    RecordsTag merge_map_tag;       // the map of the last merge; n: the records BEFORE it
    RecordsTag lod_ids_tag;         // the node index of every record of the last cut
    RecordsTag sh_tag;              // the baked SH plane (set: a bake has completed); n: its rows
    bool bake_has_counts = false;   // ... and its tap counts

    // The transitions: every event that replaces the current records, and what each does to the dependents.  keep: untouched (a tag then
    // stops holding because the epoch moved on; a count goes on describing a buffer of the OLD records); 0: zeroed / cleared; tag: retagged
    //                      | records: ptr total stored R    conv_R stale epoch | pos  sorted_n pp_visible sq_n sq_src src_tag contrib refit map  ids  sh     counts
    // conversion_started   |          keep keep  keep   R    0      0     keep  | keep keep     keep       keep keep   keep    keep    keep  keep keep keep   keep
    // conversion_finished  |          ptr  total stored keep keep   keep  +1    | keep keep     keep       keep keep   keep    keep    keep  keep keep keep   keep
    // slot_adopted         |          ptr  total stored R    0      stale +1    | keep keep     keep       keep keep   keep    keep    keep  keep keep keep   keep
    // records_uploaded     |          ptr  n     n      0    0      0     +1    | keep 0        0          0    keep   keep    keep    keep  keep keep keep   keep
    // records_adopted      |          ptr  n     n      R    0      0     +1    | keep 0        0          0    keep   keep    keep    keep  keep keep keep   keep
    // scene_replaced       |          0    0     0      keep keep   0     +1    | keep keep     keep       keep keep   keep    keep    keep  keep keep keep   keep
    // pool_released        |          0    keep  0      keep keep   keep  keep  | keep keep     keep       keep keep   keep    keep    keep  keep keep keep   keep
    // rewritten, as        |          pool n     n      R    *      0     +1    | keep 0        0          0    0      keep    0       *     keep keep *      *
    //   Prune              |                                 keep                                                                      keep            keep   keep
    //   PruneWithSh        |                                 keep                                                                      keep            tag    0
    //   RefitApply, Merge  |                                 keep                                                                      0               0      keep
    //   LodCut             |                                 keep                                                                      keep            0      keep
    //   MergeWithSh        |                                 keep                                                                      0               tag    0
    //   LodCutWithSh       |                                 keep                                                                      keep            tag    0
    //   WorldUnits         |                                 old R, unless set                                                         0               0      keep
    // (Merge and LodCut then tag the map / the node indices, run_pass the position plane its sparse kernel wrote: what they produce.
    // MergeWithSh, LodCutWithSh: m2s_set_carry_sh — the plane was reduced with the records / compacted out of the tree's; as PruneWithSh.)

    // a conversion at R is about to be launched (written before it can fail: a failed one leaves the OLD records with the new R) ...
    void conversion_started(uint32_t R) { last_R = R; conv_R = 0; records_stale = false; }
    // ... and has finished, into the context's pool or into the caller's buffer
    void conversion_finished(const void* records, uint64_t total, uint64_t stored) { current(records, total, stored); }
    // m2s_convert_wait: the awaited slot's records; stale: a later submission at another R has been enqueued over them
    void slot_adopted(const void* records, uint64_t total, uint64_t stored, uint32_t R, bool stale) {
        current(records, total, stored);
        last_R = R; conv_R = 0; records_stale = stale;
    }
    // m2s_set_records: the caller's device records, zero copy; m2s_upload_records: host records in d_loaded, without a resolutionTarget
    void records_adopted(const void* records, uint64_t n, uint32_t R) {
        current(records, n, n);
        last_R = R; conv_R = 0; records_stale = false;
        sorted_n = 0; pp_visible = 0; sq_n = 0;
    }
    void records_uploaded(const void* records, uint64_t n) { records_adopted(records, n, 0); }
    void scene_replaced() { current(nullptr, 0, 0); records_stale = false; }   // m2s_upload_scene: the old scene's records are not this one's
    // ensure_records is about to release `pool`: records that live there go with it (no epoch bump: nothing can hold for no records)
    void pool_released(const void* pool) { if (pool && last_records == pool) { last_records = nullptr; last_stored = 0; } }
    // a pass has rewritten the current records into `pool` (the stream has drained): n of them, at resolutionTarget R
    void rewritten(const void* pool, uint64_t n, uint32_t R, Rewrite as) {
        const uint32_t old_R = last_R;
        current(pool, n, n);
        last_R = R; records_stale = false; sorted_n = 0; pp_visible = 0; sq_n = 0; sq_src = nullptr;
        contrib_tag.clear();
        if (as == Rewrite::RefitApply || as == Rewrite::Merge || as == Rewrite::MergeWithSh || as == Rewrite::WorldUnits) refit_tag.clear();
        if (as == Rewrite::PruneWithSh || as == Rewrite::MergeWithSh || as == Rewrite::LodCutWithSh) {
            sh_tag.set(*this, n); bake_has_counts = false;   // (the plane was compacted / reduced with them, its tap counts were not)
        }
        else if (as != Rewrite::Prune) sh_tag.clear();
        if (as == Rewrite::WorldUnits && !conv_R) conv_R = old_R;   // (set already: a cut through a tree of stored-unit leaves brought their R back since)
    }
private:
    void current(const void* records, uint64_t total, uint64_t stored) { last_records = records; last_total = total; last_stored = stored; ++records_epoch; }
};
inline void RecordsTag::set(const RecordState& cur, uint64_t count) { of = cur.last_records; n = count; epoch = cur.records_epoch; }
inline bool RecordsTag::holds(const RecordState& cur) const { return of && of == cur.last_records && epoch == cur.records_epoch; }
}  // namespace m2s_host
