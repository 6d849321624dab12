// m2s_ctx.h — the context behind the C ABI (include/m2s.h) and the helpers its translation units share.  Internal.
//   m2s_context.cpp  lifetime, setters, record pool, in-flight waits, launch tags   m2s_upload.cpp   m2s_upload_scene / m2s_prepare
//   m2s_pass.cpp     the conversion pass driver (== ConversionPass::execute), what a lane needs before a conversion (ensure_lane)
//   m2s_async.cpp    m2s_convert_submit / _wait
//   m2s_records.cpp  read-back, .ply export, record adoption               m2s_viewer.cpp   depth sort, viewer prepass
//   m2s_splat.cpp    the splat pass (== GaussianSplattingPass::execute) and its G-buffer
//   m2s_light.cpp    the shadow and relighting passes (== GaussianShadowPass / GaussianRelightingPass::execute)
//   m2s_meshdepth.cpp  the mesh depth prepass (== DepthPrepass::execute)
//   m2s_meshrender.cpp the mesh render pass (== MeshRenderPass::execute) and the mesh G-buffer
//   m2s_score.cpp    the fidelity score (m2s_score_frames): mesh frame against splat frame
//   m2s_contrib.cpp  the contribution pass and pruning (m2s_contrib_accumulate, m2s_prune)
//   m2s_budget.cpp   pruning to a budget (m2s_prune_budget): the radix select in front of m2s_prune's compaction
//   m2s_refit.cpp    the colour refit (m2s_refit_accumulate, m2s_refit_apply): the albedo error of K views carried back to the records
//   m2s_merge.cpp    the merge pass (m2s_merge): neighbouring records replaced by their moment-matched parent, a baked SH plane merged with them (m2s_set_carry_sh)
//   m2s_worldunits.cpp  m2s_records_to_world_units: a conversion's scales divided by its resolutionTarget
//   m2s_lod.cpp      the level-of-detail tree and its per-camera cut (m2s_lod_build, m2s_lod_select, m2s_lod_select_budget, their _frustum forms): a chain of merges kept and linked; the blend of a cut towards its parents (m2s_lod_blend)
//   m2s_bake.cpp     the light baked into spherical harmonics (m2s_bake_light, m2s_sh_shade_records, m2s_export_ply_sh)
//   m2s_compact.cpp  the compact .ply export (m2s_export_ply_compact); its host writer and decoder: m2s_compact_host.cpp
//   m2s_devbuf.h     the owners of everything the context keeps: DevBuf, PinnedBuf, EventSet, StreamSet; BinWork (viewer passes), Lane (conversions)
//   m2s_stageclock.h stage timing: StageClock, one per pass below and the marks of each (the enums of that header), StageMarks for the launchers
//   m2s_lodtree.h    the level-of-detail tree and what its passes work in: LodTree (planes, levels, generation; the only code that grows, ends or commits one), LodWork
//   m2s_recstate.h   the current records, what hangs on them and the transitions between them: RecordState (a base of m2s_ctx), RecordsTag
#pragma once
#include "../../include/m2s.h"
#include "m2s_devbuf.h"
#include "m2s_device.h"
#include "m2s_lodtree.h"
#include "m2s_recstate.h"
#include "m2s_vdedup.h"

#include <cstdint>
#include <cstdlib>
#include <map>
#include <string>

namespace m2s_host {
constexpr uint32_t kMaxGaussiansToSort = 7000000u;  // RenderPass.hpp:9
constexpr uint64_t kMaxTriangles = (1ull << 28) - 1;  // 32-bit byte offsets into the 16 B/triangle planes
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline const char* const kStaleMsg = "the records of the conversion last waited for have been overwritten by a later submission at another R "
                                     "(wait for it, or submit into your own buffers)";
inline const char* const kInFlightMsg = "conversions are still in flight: m2s_convert_wait first";
// The five planes of a G-buffer (8, 8, 4, 8, 4 bytes per pixel), each with room for the same number of pixels; ptr: as the kernels take them.
struct GBufPlanes {
    DevBuf<void> plane[5];
    void* ptr[5] = {};
    m2s_status reserve(std::string& err, uint64_t px) {
        for (int k = 0; k < 5; ++k) {
            const m2s_status s = plane[k].reserve(err, px, (k == 2 || k == 4) ? 4 : 8);
            ptr[k] = plane[k].get();
            if (s) return s;
        }
        return M2S_OK;
    }
};
}  // namespace m2s_host

constexpr int kBandSlotsMax = 64;   // (scene, R) entries remembered per context: band tables, decisions
struct m2s_ctx : m2s_host::RecordState {   // (the current records and their dependents: m2s_recstate.h)
    int device = 0;
    m2s_host::StreamSet<2> streams;         // lane k's stream; in front of every buffer and event: destroyed after them
    hipStream_t stream = nullptr;           // streams[0] == lane[0].stream: what every pass but a second-lane conversion runs on
    std::string err;

    // scene
    m2s_host::DevBuf<char> tri_mem;         // the geometry planes; released with the scene, like the arena
    m2s::SceneDev scene{};
    m2s::MeshParams* d_meshes = nullptr;
    uint32_t* d_mesh_first = nullptr;
    uint32_t n_meshes_total = 0;
    bool has_scene = false;
    bool lean_ok = false;                   // every mesh of the scene samples its combo texture or no map at all: k_fused3 may run
    uint64_t range_first = 0, range_count = UINT64_MAX;
    // the resident shard's distinct vertices (m2s_vdedup.hip), decided once per upload: conversions in the lean form gather from the
    // table (the indexed instance of k_fused3) while vt_use holds; the planes stay for everything else
    m2s_host::DevBuf<float4> d_vt_rows;     // three float4 per row; capacity in float4
    m2s_host::DevBuf<m2s::VtIds> d_vt_ids;  // per resident triangle
    uint32_t vt_rows = 0;                   // distinct vertices of the last upload (0: not counted — the scene was out of the table's range)
    bool vt_use = false;
    // the resident triangles' geometry planes (m2s_geoplanes.hip): Quaternion, Scale and the orthogonal UVs, built once per upload behind
    // the repack; conversions in the lean form read them (the kGeo instances of k_fused3) while geo_use holds, every other kernel computes
    m2s_host::DevBuf<float4> d_geo;         // G0 | G1 | G2, geo_stride float4 apart; capacity in float4
    size_t geo_stride = 0;
    bool geo_use = false;

    // work buffers (sized by the scene)
    uint32_t* d_cnt = nullptr;
    uint32_t* d_partials = nullptr;
    m2s_host::PinnedBuf<unsigned long long> h_total;   // kPinnedWords words: [0] = fragment counter, [1] = status words of the fused kernel,
                                            // [2 + 2k], [3 + 2k] = the same of in-flight slot k, then one word each for the prepass and the depth sort
    static constexpr int kPinnedPrepass = 2 + 2 * M2S_MAX_IN_FLIGHT;   // m2s_prepass: TWO words — survivors, then the status words of its look-back
    static constexpr int kPinnedSortMM = 4 + 2 * M2S_MAX_IN_FLIGHT;    // the depth sorts: {min, max} of the keys (two 32-bit words); NOT the prepass's second word —
                                                                       // m2s_prepass_sorted uses both inside one call
    static constexpr int kPinnedWords = 6 + 2 * M2S_MAX_IN_FLIGHT;                  // (the sorts' word and the one behind it: {min, max}, {survivors, clash})
    m2s::BigItem* d_biglist = nullptr;           // triangles deferred by the fused kernel (capacity: triangles in range)
    uint32_t* d_bigmeta = nullptr;          // [0] entries in d_biglist, [1] largest, [2] total fragment count; zero between conversions
    // What the context remembers about the uploaded scene at a given resolution R.  The reference converts on load and
    // whenever the density slider moves (guiRendererConcreteMediator.cpp:51-57), i.e. mostly at an R it has not seen
    // before, so nothing here may be REQUIRED for a fast conversion: a new R costs no counting pass and no extra host
    // round trip (the AUTO decision is taken from frag_per_R2, the band bases are a by-product of the first launch).
    struct RInfo {
        int form = M2S_PIPELINE_AUTO;   // what the next conversion at this R runs: M2S_PIPELINE_SPARSE / _LEAN / _TEAM / _MULTIPASS
                                        // (m2s_pass.cpp: decide() sets it, demote() moves it down the ladder); AUTO: not decided yet
        uint32_t tpw = 0;          // AUTO: k_fused2 in batches of this many triangles (0: fused_tpw) — the 11-18 fragments-per-triangle band
        bool async_ok = false;     // a completed conversion needed no host decision between kernels
        bool mp_ready = false;     // a multi-pass conversion has completed (its work buffers are sized)
        bool bands_ready = false;  // the run table of this R (slot band_slot of d_bands: where every run's output starts) is in place ...
        uint32_t bands_unit = 0;   // ... in units of this many triangles (256: recorded by a k_fused2 launch, 512: k_sparse)
        int band_slot = 0;
        uint32_t gen = 0;          // generation of the table this entry belongs to (the table starts over when it is full)
    };
    // smallest R at which a workgroup of k_sparse / k_fused3 / k_fused2 did not fit its LDS stream (k_fused3: or deferred many
    // triangles): a property of the SCENE (fragments grow with R), so a new R above it starts with the next form at once instead
    // of re-discovering the overflow (demote() lowers them, decide() applies them)
    uint32_t sparse_off_R = UINT32_MAX, team_off_R = UINT32_MAX, lean_off_R = UINT32_MAX;
    uint32_t rinfo_gen = 0;
    std::map<uint32_t, RInfo> rinfo;
    double frag_per_R2 = -1.0;              // fragments / R^2 of this scene: from the exact count m2s_upload_scene takes (warm_scene), refreshed by every conversion
    uint64_t warm_total = 0;                // fragments of the scene at warm_R (exact: warm_scene's count)
    uint64_t warm_big = 0;                  // ... of which in triangles of more than 96 fragments (what a single-pass kernel would defer)
    bool warm_mismatch_seen = false;        // a launch in runs disagreed with that count once (run_pass): not retried again
    uint32_t hint_R = 0;                    // m2s_set_resolution_hint: the R the next upload prepares for (0: the last R converted at, else 1024)
    uint32_t warm_R = 0;                    // the R the resident scene was prepared for
    uint32_t warm_spec_unit = 0, warm_spec_shift = 0;   // run table + dispatch order enqueued with the upload's count, for units of this many triangles (0: none)
    unsigned long long* d_bands = nullptr;  // kBandSlots run tables of run_table_words words each (RunInfo, m2s_device.h)
    size_t run_table_words = 0;
    uint32_t* d_run_order = nullptr;        // dispatch order of the runs (launch_run_order), built by warm_scene from the exact counts ...
    uint32_t run_order_unit = 0, run_order_shift = 0;   // ... for runs of (1 << shift) units of this many triangles (0: none)
    void* d_run_rank = nullptr;             // launch_run_order's scratch: the runs' costs and ids in rank order (run_order_scratch_bytes)
    uint32_t* d_batch_first = nullptr;      // work-balanced batches of k_fused2 (small scenes; built from the first exact count)
    uint32_t n_batch_tab = 0;               // batches in it (0: uniform batches)
    size_t chain_words = 0;                 // words of every lane's chain
    int last_pipeline = 0;                  // what the last conversion ran (m2s_last_pipeline)
    // What conversions work in (m2s_devbuf.h), one set per lane.  Lane 0: every synchronous conversion, and the record pool (records:
    // ensure_records).  Lane 1, for context-owned asynchronous submissions: odd slots run on their own stream with their own chain
    // and record buffer, so that consecutive single-kernel conversions overlap (the tail of one, where the GPU drains, with the head
    // of the next) instead of paying ~8 us between dependent kernels on one stream; and multi-pass conversions too — with a work set
    // of its own, k_count_scan of conversion i + 1 runs beside k_emit2 of conversion i.  Lane 1 is filled at its first use (ensure_lane).
    m2s_host::Lane lane[2];
    int lanes = 1;                          // m2s_set_async_lanes
    int pipeline = M2S_PIPELINE_AUTO;
    uint32_t epoch = 0;                     // launch counter of the fused kernel (tags the chain words)

    // asynchronous submissions (m2s_convert_submit / m2s_convert_wait): a ring of result slots.  Slot k uses
    // h_total[2 + 2k] (counter) and h_total[3 + 2k] (status words), written by the kernel itself.
    struct Slot { m2s_host::EventSet<1> done; m2s_host::EventSet<2> t;   // completion (flags: m2s_create); start / end of the kernel, profiling on
                  uint64_t limit = 0; void* d_out = nullptr; uint32_t R = 0;
                  bool sync_result = false; uint64_t sync_total = 0; bool prof = false; float ms[M2S_K_N] = {};
                  int own_lane = -1; uint32_t gen = 0;   // the lane whose record buffer it writes and that buffer's generation at submission; -1: caller's buffer
                  bool wrote_bands = false; uint32_t bands_unit = 0; uint32_t ri_gen = 0;   // the launch leaves band bases behind, for the RInfo entry of that table generation
                  hipStream_t st = nullptr; bool shared_work = false; };   // stream it ran on; did it use the context's shared work buffers (chain, deferred list)?
    Slot slot[M2S_MAX_IN_FLIGHT];
    uint32_t slot_head = 0, slot_count = 0; // oldest in-flight slot, number in flight

    int64_t cap_policy = -1;

    // depth sort (f-2)
    m2s_host::DevBuf<float4> d_sorted;     // capacity in records (sorted_n of them)
    m2s_host::DevBuf<uint32_t> d_sort_u32;   // keys_in | vals_in | keys_out | vals_out: capacity in records (four words each), sliced by the CURRENT n
    uint32_t sorted_key_offset = 0;   // keys_out holds key - this (m2s_device_sorted_keys adds it back once)
    m2s_host::DevBuf<void> d_sort_temp;      // capacity: the bytes last asked for
    float last_sort_ms = 0.0f;
    float last_sort_stage_ms[3] = { 0, 0, 0 };   // keys | radix sort | gather of the last m2s_sort_by_depth (profiling on)
    m2s_host::ClockOf<m2s_host::SortMark> sort_clock;                // m2s_sort_by_depth and m2s_prepass_sorted: the sort's marks and the prepass's chain
    // the positions of the current records as a compact plane (16 B each), left behind by the first depth sort after the records
    // changed and used for the keys of every later one (m2s_sort.hip); valid while pos_plane_tag holds
    m2s_host::DevBuf<float4> d_pos_plane;
    bool keep_positions = false;      // m2s_set_keep_positions: conversions leave the plane behind themselves where their kernel can (k_sparse)
    // viewer prepass (m2s_prepass): survivors, their depths, the look-back chain of its kernel, a copy of the depth image
    m2s_host::DevBuf<float4> d_quads;
    m2s_host::DevBuf<float> d_pp_depths;      // (pp_visible of each)
    m2s_host::DevBuf<unsigned long long> d_pp_chain;     // capacity in words
    uint32_t pp_epoch = 0;
    m2s_host::DevBuf<float> d_pp_depthtex;
    float last_prepass_ms = 0.0f;
    m2s_host::ClockOf<m2s_host::SpanMark> prepass_clock;   // m2s_prepass's (m2s_prepass_sorted: sort_clock)
    m2s_host::PinnedBuf<m2s_gaussian> h_export[2];      // pinned chunk buffers of m2s_export_ply
    // upload staging: two pinned host chunks (filled by a few host threads while the previous chunk is on the bus) and
    // two device chunks for the AoS -> SoA repack; allocated at the first upload, kept
    m2s_host::PinnedBuf<char> h_stage[2];
    m2s_host::DevBuf<char> d_stage[2];
    m2s_host::EventSet<2> stage_ev;          // (no timing)
    m2s_host::DevBuf<char> scene_arena;      // one allocation for mesh table, textures, combo textures and work buffers; released with the scene
    float last_upload_ms[5] = { 0, 0, 0, 0, 0 }; // [0] total, [1] geometry, [2] textures + mips + combo, [3] allocations, [4] warm_scene
    m2s_host::DevBuf<uint8_t> d_rows;        // m2s_export_ply: .ply rows encoded on the device (formats 1 and 2); capacity in bytes
    m2s_host::DevBuf<void> d_loaded;         // m2s_upload_records (a loaded .ply)
    m2s_host::DevBuf<float4> d_sorted_quads; // m2s_sort_prepass (sq_n of them)
    float last_sort_prepass_ms = 0.0f;
    m2s_host::ClockOf<m2s_host::SpanMark> sort_prepass_clock;
    // splat pass (m2s_splat.cpp): the five G-buffer planes of the last call and the pass's grow-only work buffers
    m2s_host::GBufPlanes d_gbuf;
    int32_t gbuf_w = 0, gbuf_h = 0;          // resolution of the planes' contents (0: no splat has run)
    m2s_host::BinWork splat_work;            // per quad a 128-byte record; totals: [0] pairs, [1] skipped quads, [2] fragments blended
    m2s_host::DevBuf<uint32_t> d_splat_tiles;   // ranges (2 words) | lengths | sorted lengths | order, one capacity of tiles each
    float last_splat_ms = 0.0f;
    m2s_host::ClockOf<m2s_host::BinMark> bin_clock;              // splat_bin's, a member like splat_work: m2s_splat, m2s_contrib_accumulate, m2s_refit_accumulate add the blend's mark
    float last_splat_stage_ms[3] = { 0, 0, 0 };     // setup + bin, grouping, blend (profiling on)
    uint64_t last_splat_counts[3] = { 0, 0, 0 };    // pairs, fragments blended, quads skipped
    // sources of the sorted quads (m2s_prepass_sorted): which record each was made from.  Dense path: the first sq_n words of the
    // permutation in d_sort_u32 (an alias: dropped by whatever rewrites those words); compacting path: d_sq_src, written by k_prepass
    // (sq_src points at whichever it is, sq_src_tag names the records they index into)
    m2s_host::DevBuf<uint32_t> d_sq_src;
    // contribution pass and pruning (m2s_contrib.cpp): wmax | npix, one capacity of words each, valid while contrib_tag holds
    m2s_host::DevBuf<uint32_t> d_contrib;
    float last_contrib_ms = 0.0f;
    float last_contrib_stage_ms[3] = { 0, 0, 0 };
    m2s_host::DevBuf<uint32_t> d_prune_u32;  // flags | offsets, one capacity of words each
    m2s_host::DevBuf<char> d_prune_temp;     // scan work area, then two counters (u64) in its last 16 bytes; capacity in bytes
    m2s_host::DevBuf<float4> d_prune_stage;  // survivors on their way back into the buffer they came from; capacity in bytes
    uint64_t last_prune_counts[4] = { 0, 0, 0, 0 };
    float last_prune_ms = 0.0f;
    m2s_host::ClockOf<m2s_host::SpanMark> prune_clock;
    // pruning to a budget (m2s_budget.cpp): one key per record and the select's words (m2s_device.h); flags, offsets, scan area and
    // staging are m2s_prune's
    m2s_host::DevBuf<uint32_t> d_budget_keys;
    m2s_host::DevBuf<uint32_t> d_budget_state;
    uint64_t last_budget_counts[6] = { 0, 0, 0, 0, 0, 0 };
    float last_budget_stage_ms[3] = { 0, 0, 0 };   // keys + select rounds, flags + scans, compaction (profiling on)
    m2s_host::ClockOf<m2s_host::BudgetMark> budget_clock;
    // colour refit (m2s_refit.cpp): num (int64, three words per record) | den (uint64), one capacity of records; valid while refit_tag holds
    m2s_host::DevBuf<unsigned long long> d_refit;
    m2s_host::DevBuf<unsigned long long> d_refit_counts;   // m2s_refit_apply: updated, clamped, left for lack of weight
    float last_refit_stage_ms[3] = { 0, 0, 0 };    // setup + bin, grouping, refit blend (profiling on)
    float last_refit_apply_ms = 0.0f;
    m2s_host::ClockOf<m2s_host::SpanMark> refit_apply_clock;
    // merge pass (m2s_merge.cpp): flag | run_start | packed (64-bit) | sums (64-bit) | seg_start (7 capacities of words; sized for n + 1), the totals, and the
    // map of the last merge, valid while merge_map_tag holds; keys, permutation and the sort's work area are the compact export's
    m2s_host::DevBuf<uint32_t> d_merge_u32;
    m2s_host::DevBuf<uint32_t> d_merge_totals;
    m2s_host::DevBuf<uint32_t> d_merge_map;
    uint64_t last_merge_counts[4] = { 0, 0, 0, 0 };
    float last_merge_stage_ms[3] = { 0, 0, 0 };          // keys + sort, heads + scans, reduce + adopt
    m2s_host::ClockOf<m2s_host::MergeMark> merge_clock;                      // always on
    // m2s_set_carry_sh (pin 5s): a merge reduces a baked plane of the current records with them, into d_sh_alt, which then trades places
    // with d_sh (no copy back); a tree built with the switch on owns a plane of its nodes and its cuts compact it into d_sh
    bool carry_sh = false;
    m2s_host::DevBuf<float> d_sh_alt;                    // capacity in rows of 48 floats
    // m2s_set_merge_model: how a merge reads a record (pins 2g, 5g, 5sg, 4g under M2S_MERGE_MODEL_GAUSSIAN), and what its scales are
    // multiplied with to be standard deviations; not read under M2S_MERGE_MODEL_FOOTPRINT
    uint32_t merge_model = M2S_MERGE_MODEL_FOOTPRINT;
    float merge_sigma = 1.0f;
    float last_merge_sh_ms = 0.0f;                       // the SH reduction of the last merge (0: none ran); inside stage [2]
    m2s_host::ClockOf<m2s_host::SpanMark> merge_sh_clock;    // always on
    // level-of-detail tree (m2s_lod.cpp; m2s_lodtree.h): the tree — its node planes, levels and generation — and what its passes work in;
    // below them what the passes report, per pass: the build, the cut (m2s_lod_select), the cut that fits a budget (m2s_lod_select_budget),
    // the cuts over a frustum (_frustum) and behind an occluder (_occluded), the blend (m2s_lod_blend)
    m2s_host::LodTree lod;
    m2s_host::LodWork lod_work;
    float last_lod_build_ms = 0.0f;
    m2s_host::ClockOf<m2s_host::SpanMark> lod_build_clock;   // always on
    uint64_t last_lod_select_counts[4] = { 0, 0, 0, 0 };
    uint64_t last_lod_level_counts[M2S_LOD_MAX_STEPS + 1] = {};
    float last_lod_select_stage_ms[3] = { 0, 0, 0 };     // level sweep, scan + node indices, compaction (profiling on)
    m2s_host::ClockOf<m2s_host::LodCutMark> lod_cut_clock;
    float last_lod_budget_stage_ms[3] = { 0, 0, 0 };     // thresholds, the four select rounds, the cut (profiling on)
    m2s_host::ClockOf<m2s_host::LodBudgetMark> lod_budget_clock;
    uint64_t last_lod_frustum_counts[2] = { 0, 0 };      // the leaves inside, the nodes the plain cut selects and the frustum dropped
    float last_lod_frustum_ms = 0.0f;
    m2s_host::ClockOf<m2s_host::SpanMark> lod_vis_clock;     // the visibility stage
    uint64_t last_lod_occlusion_counts[4] = { 0, 0, 0, 0 };  // the leaves inside the frustum, occluded, behind the image but kept, and the nodes dropped
    uint64_t last_lod_blend_counts[4] = { 0, 0, 0, 0 };
    float last_lod_blend_ms = 0.0f;
    float last_lod_blend_stage_ms[3] = { 0, 0, 0 };      // weights, records, SH rows (profiling on)
    m2s_host::ClockOf<m2s_host::LodBlendMark> lod_blend_clock;
    // world units (m2s_worldunits.cpp)
    float last_world_units_ms = 0.0f;
    m2s_host::ClockOf<m2s_host::SpanMark> wu_clock;
    // shadow pass (m2s_light.cpp): the six per-face quad lists back to back in one exact-size, grow-only buffer, the depth cube,
    // and the pass's grow-only work buffers
    m2s_host::DevBuf<float4> d_shadow_quads; // 48 B each
    uint32_t shadow_base[7] = { 0, 0, 0, 0, 0, 0, 0 };   // first quad of every face's list; [6] = all quads (of the last m2s_shadow)
    bool shadow_lists = false;               // the lists of the last m2s_shadow exist (false after m2s_upload_shadow_cubemap)
    m2s_host::DevBuf<float> d_shadow_cube;   // float[6][S][S]; capacity in texels
    int32_t shadow_S = 0;                    // 0: no cube yet
    m2s_host::DevBuf<uint32_t> d_sh_tab;     // stage A: counts | offsets, one capacity of words each
    m2s_host::DevBuf<float> d_sh_views;      // six view matrices (96 floats) | bases (8 words)
    m2s_host::BinWork shadow_work;           // stage B: per quad a 48-byte record; totals: [0] pairs, [1] skipped quads, [2] atomics sent
                                             // (pinned: those three words, then the bases and the view matrices); its work area serves stage A too
    m2s_host::ClockOf<m2s_host::ShadowMark> shadow_clock;
    float last_shadow_ms = 0.0f;
    float last_shadow_stage_ms[3] = { 0, 0, 0 };    // stage A (count + scan + emit), setup + binning, raster (profiling on)
    uint64_t last_shadow_counts[9] = {};            // quads of face 0..5, (tile, quad) pairs, texel writes (atomics sent), quads skipped
    // relighting pass: the frame, the optional plane of shadow counts
    m2s_host::DevBuf<uint32_t> d_frame;      // capacities in pixels
    m2s_host::DevBuf<uint8_t> d_shadow_counts;
    int32_t frame_w = 0, frame_h = 0;        // 0: no relight has run
    bool frame_has_counts = false;
    float last_relight_ms = 0.0f;
    m2s_host::ClockOf<m2s_host::SpanMark> relight_clock;   // m2s_relight, m2s_relight_split, m2s_relight_mesh
    // mesh depth prepass (m2s_meshdepth.cpp): the image and the pass's grow-only work buffers
    m2s_host::DevBuf<float> d_md_image;      // float[H][W], row 0 = bottom; capacity in texels
    int32_t md_w = 0, md_h = 0;              // 0: no image yet
    int32_t md_inplace = -1;                 // m2s_debug_set_mesh_depth_inplace (-1: the default, kMdInplace)
    m2s_host::DevBuf<uint32_t> d_md_deferred;   // triangles the setup kernel left to the binned path (capacity in triangles)
    m2s_host::BinWork md_work;               // per deferred triangle six slots of a 48-byte record; totals: 8 words, see meshdepth_setup
    m2s_host::ClockOf<m2s_host::MeshMark> md_clock;              // mesh_raster: this pass and the visibility stage of the mesh render pass
    float last_md_ms = 0.0f;
    float last_md_stage_ms[3] = { 0, 0, 0 };     // setup + in-place, clip + binning, tile raster (profiling on)
    uint64_t last_md_counts[5] = {};             // drawn, clipped, non-finite, pairs, texel updates sent
    // mesh render pass (m2s_meshrender.cpp): the visibility image and the mesh G-buffer; its work buffers are the mesh depth prepass's
    m2s_host::DevBuf<unsigned long long> d_mr_vis;   // uint64[H][W], row 0 = bottom: (bits of z) << 32 | global triangle index
    m2s_host::GBufPlanes d_mr_gbuf;              // layouts of d_gbuf
    int32_t mr_w = 0, mr_h = 0;                  // 0: no mesh G-buffer yet
    float last_mr_ms = 0.0f;
    m2s_host::ClockOf<m2s_host::SpanMark> mr_clock;   // (the shading; the visibility stage: md_clock)
    float last_mr_stage_ms[4] = { 0, 0, 0, 0 };  // visibility setup + in-place, clip + binning, tile raster, shading (profiling on)
    uint64_t last_mr_counts[6] = {};             // drawn, clipped, non-finite, pairs, texel updates sent, culled as back-facing
    // fidelity score (m2s_light.cpp: m2s_relight_mesh; m2s_score.cpp): the mesh-lit frame, the comparison's counters and error map
    m2s_host::DevBuf<uint32_t> d_mesh_frame;     // uchar4[H][W], row 0 = bottom
    int32_t mesh_frame_w = 0, mesh_frame_h = 0;  // 0: no m2s_relight_mesh has run
    m2s_host::DevBuf<unsigned long long> d_score_acc;    // kScoreShards x kScoreCounters words (m2s_device.h), summed on the host
    m2s_host::PinnedBuf<unsigned long long> h_score;     // pinned copy
    m2s_host::DevBuf<uint32_t> d_score_map;      // uchar4[H][W]
    int32_t score_map_w = 0, score_map_h = 0;    // 0: the last m2s_score_frames kept no map
    float last_score_ms = 0.0f;
    m2s_host::ClockOf<m2s_host::SpanMark> score_clock;

    // light baked into spherical harmonics (m2s_bake.cpp): the coefficient plane, the optional tap counts, the quadrature table
    m2s_host::DevBuf<float> d_sh;                // float[n][48]: f_dc[3], f_rest[45] channel-major; capacity in records; sh_tag: set once a
                                                 // bake has completed, n rows of the records it names — m2s_prune compacts the plane of the records it compacts
    m2s_host::DevBuf<uint8_t> d_bake_counts;     // uint8[n] (bake_has_counts)
    m2s_host::DevBuf<float> d_bake_table;        // n_theta * n_phi rows of kBakeTableRow floats
    uint32_t bake_table_nt = 0, bake_table_np = 0;
    float last_bake_ms = 0.0f;
    m2s_host::ClockOf<m2s_host::SpanMark> bake_clock;
    uint32_t sh_degree = 0;                      // degree of the last bake (the compact export's SH element)

    // compact .ply export (m2s_compact.cpp): the pass's own buffers — the depth sort's words are the prune pass's sources and stay as they are
    m2s_host::DevBuf<uint32_t> d_compact_u32;    // keys_in | vals_in | keys_out | vals_out, one capacity of words each
    m2s_host::DevBuf<uint32_t> d_compact_waves;  // per-wave boxes (8 words each), then the 8 words of the fold; capacity in waves
    m2s_host::DevBuf<void> d_compact_temp;       // the sort's work area; capacity in bytes
    m2s_host::DevBuf<uint8_t> d_compact_out;     // chunk table | rows | SH bytes, each from a 256-byte boundary; capacity in bytes
    m2s_host::PinnedBuf<uint32_t> h_compact;     // pinned { N, skipped }
    m2s_host::ClockOf<m2s_host::CompactMark> compact_clock;          // always on
    float last_compact_stage_ms[4] = { 0, 0, 0, 0 };   // box + keys, sort, pack, download + write

    // measurement
    bool profiling = false;
    m2s_host::ClockOf<m2s_host::ConvMark> conv_clock;           // the conversion driver (m2s_pass.cpp)
    float last_ms[M2S_K_N] = {};
};

#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
            return e_ == hipErrorOutOfMemory ? M2S_ERR_OOM : M2S_ERR_HIP;                         \
        }                                                                                         \
    } while (0)
#define M2S_TRY(expr)                                                                             \
    do {                                                                                          \
        if (m2s_status s_ = (expr)) return s_;                                                    \
    } while (0)

namespace m2s_host {
inline m2s_status fail(m2s_ctx* c, m2s_status s, const std::string& msg) {
    if (c) c->err = msg;
    return s;
}
template <class T, size_t N> inline m2s_status get_array(const m2s_ctx* c, T (m2s_ctx::*member)[N], T* out) {   // the getters of a member array
    if (c && out) for (size_t k = 0; k < N; ++k) out[k] = (c->*member)[k];
    return c && out ? M2S_OK : M2S_ERR_INVALID;
}
// the R last converted at, for the readers that mean the scene's density and not the unit of the records (the upload's warm_R,
// m2s_download_triangle_counts): last_R, unless m2s_records_to_world_units has taken that to 1 since
inline uint32_t converted_R(const m2s_ctx* c) { return c->conv_R ? c->conv_R : c->last_R; }
// argument checks the entry points share
inline m2s_status check_resolution(m2s_ctx* c, int W, int H, const char* what = "resolution") {
    if (W < 1 || W > 8192 || H < 1 || H > 8192) return fail(c, M2S_ERR_INVALID, std::string(what) + " outside 1..8192");
    return M2S_OK;
}
// the context's records, or the caller's
inline m2s_status pick_records(m2s_ctx* c, const void*& d_records, uint64_t& n) {
    if (!d_records) {
        if (!c->last_records) return fail(c, M2S_ERR_STATE, "no conversion has run, no records were uploaded and none were passed");
        if (c->records_stale) return fail(c, M2S_ERR_STATE, kStaleMsg);
        d_records = c->last_records;
        n = c->last_stored;
    }
    if (n > 0xFFFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^32-1 records");
    return M2S_OK;
}
// What the passes over the context's own records open with: nothing in flight, records, not overwritten (have_records), at most
// 2^32-1 of them (need_records; *n: how many).
inline m2s_status have_records(m2s_ctx* c) {
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    if (!c->last_records) return fail(c, M2S_ERR_STATE, "no conversion has run and no records were uploaded");
    if (c->records_stale) return fail(c, M2S_ERR_STATE, kStaleMsg);
    return M2S_OK;
}
inline m2s_status need_records(m2s_ctx* c, uint64_t* n) {
    M2S_TRY(have_records(c));
    *n = c->last_stored;
    if (*n > 0xFFFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^32-1 records");
    return M2S_OK;
}
// the position plane belongs to the n current records (m2s_positions_ready: and there are some)
inline bool positions_valid(const m2s_ctx* c, uint64_t n) { return c->d_pos_plane && c->pos_plane_tag.holds(*c, n); }
constexpr int kBandSlots = kBandSlotsMax;

// m2s_context.cpp
// Waiting for a conversion.  The runtime's hipStreamSynchronize / hipEventSynchronize hand the caller back 10-18 us after the last
// kernel has finished — 8-13 % of a 0.12 ms conversion, the reference's glFinish (ConversionPass.cpp:54).  These poll the same
// completion signal (hipStreamQuery / hipEventQuery: the stream's own "all work done") for up to 400 us and only then block.
hipError_t wait_stream(hipStream_t st);
hipError_t wait_event(hipEvent_t ev);
void free_scene(m2s_ctx* c);
m2s_ctx::RInfo& rinfo_for(m2s_ctx* c, uint32_t R);
// The in-flight slots, oldest first; and the newest one that pred holds for (nullptr: none).
template <class F>
inline void each_in_flight(m2s_ctx* c, F f) {
    for (uint32_t q = 0; q < c->slot_count; ++q) f(c->slot[(c->slot_head + q) % M2S_MAX_IN_FLIGHT]);
}
template <class P>
inline m2s_ctx::Slot* newest_in_flight(m2s_ctx* c, P pred) {
    for (uint32_t q = c->slot_count; q-- > 0;) {
        m2s_ctx::Slot& sl = c->slot[(c->slot_head + q) % M2S_MAX_IN_FLIGHT];
        if (pred(sl)) return &sl;
    }
    return nullptr;
}
// every conversion still in flight (lane >= 0: into that lane's record buffer) has finished when this returns
void drain_in_flight(m2s_ctx* c, int lane = -1);
hipError_t next_epoch(m2s_ctx* c, uint32_t* out);
m2s_status ensure_records(m2s_ctx* c, uint64_t want);
// m2s_upload.cpp
m2s_status ensure_stage(m2s_ctx* c);
// m2s_splat.cpp
// The stages of the splat pass in front of the blend — setup / bin, pairs, grouping by tile, tile order — over n quads on a W x H
// viewport, in the context's splat work buffers: what m2s_splat, m2s_contrib_accumulate and m2s_refit_accumulate start with.  Opens
// bin_clock (profiling) and records BinMark::Setup .. Grouped; synchronises once (the pair count).  vals / ranges / order are NULL without pairs.
struct SplatBins { const uint32_t* vals = nullptr; const uint2* ranges = nullptr; const uint32_t* order = nullptr; uint64_t pairs = 0, skipped = 0; };
m2s_status splat_bin(m2s_ctx* c, const void* d_quads, uint32_t nq, int W, int H, SplatBins* out);
m2s_status splat_stage_ms(m2s_ctx* c, float out[3]);   // ... and their times + the blend's (the caller's BinMark::Blended), bin_clock on
// m2s_contrib.cpp
inline bool contrib_valid(const m2s_ctx* c) { return c->contrib_tag.holds(*c, c->last_stored); }   // the accumulators belong to the current records
// What m2s_prune and m2s_prune_budget end with.  prune_compact_enqueue: the `kept` flagged records of the n current ones (and the rows of
// a baked plane, with sh) go into the pool in order, through the staging buffer where they would land on themselves; n = 0: a pool to
// point at.  Once the stream has drained the caller records the event: c->rewritten(pool, kept, R, Rewrite::...) (m2s_recstate.h).
inline bool prune_sh_plane(const m2s_ctx* c, uint64_t n) { return c->sh_tag.holds(*c, n); }   // a baked plane of exactly these n current records exists
// src (m2s_lod_select): the n records are these, in memory that is not the pool, instead of the current ones; no plane then.
m2s_status prune_compact_enqueue(m2s_ctx* c, uint64_t n, uint64_t kept, const uint32_t* flags, const uint32_t* offsets, bool sh,
                                 const void* src = nullptr);
// m2s_merge.cpp
// What m2s_merge does behind its argument checks (level 0..10, max_group 2..64, no NaN), m2s_lod_build once per step; the counts are
// left in last_merge_counts.  Dry: only the counts; IfAny: as Dry where no segment has two members, as Apply otherwise.
enum class MergeMode { Apply, Dry, IfAny };
m2s_status merge_run(m2s_ctx* c, uint32_t level, uint32_t max_group, float min_axis_dot, MergeMode mode, bool unsigned_axis);
// m2s_meshdepth.cpp
// What the mesh depth prepass and the visibility stage of the mesh render pass share: clear, setup + in-place lanes, clipper + binning,
// tile raster over `image` (float[W * H], or uint64[W * H] when vis), synchronous.  ms: the three stage times (profiling on);
// c->md_work.h_totals holds the pass's totals afterwards (m2s_device.h: meshdepth_setup, meshvis_setup).
m2s_status mesh_raster(m2s_ctx* c, const m2s::MeshDepthK& k, bool vis, void* image, float ms[3]);
// (P V) M in glm's order, every operation rounded to fp32: the clip transform of both passes
void mesh_pvm(const float* proj, const float* view, const float* model, float* out);
// m2s_pass.cpp
uint32_t unit_of(int form);   // triangles per band unit of a single-pass form
void launch_single(const m2s_ctx* c, const m2s_ctx::RInfo& ri, uint32_t R, unsigned long long* chain, uint64_t limit, float4* d_out,
                   unsigned long long* res, uint32_t epoch, const m2s::RunInfo& runs, hipStream_t st, float4* plane);
m2s::RunInfo bands_for(const m2s_ctx* c, const m2s_ctx::RInfo& ri, uint32_t unit, bool may_write, bool* writes);
m2s::BatchTable batches_for(const m2s_ctx* c, const m2s_ctx::RInfo& ri);
uint64_t resolve_cap(const m2s_ctx* c, uint32_t R);
m2s_status warm_scene(m2s_ctx* c, uint32_t R, bool counted = false);   // called by m2s_upload_scene once the scene is resident
m2s_status warm_count_enqueue(m2s_ctx* c, uint32_t R);                  // ... its exact count, enqueued earlier (in front of the texture copies)
m2s_status enqueue_multipass(m2s_ctx* c, int lane, uint32_t R, float4* d_out, uint64_t limit, const StageMarks& marks, unsigned long long* h_res, hipStream_t st);
// what `lane` needs before a conversion is enqueued on it; multipass: its multi-pass work set for n_start slices included
m2s_status ensure_lane(m2s_ctx* c, int lane, bool multipass, uint32_t n_start);
m2s_status run_pass(m2s_ctx* c, uint32_t R, void* d_user, uint64_t user_cap, hipStream_t st, uint64_t* out_total,
                    bool from_submit = false);
}  // namespace m2s_host
