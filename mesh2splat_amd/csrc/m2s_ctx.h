// m2s_ctx.h — the context behind the C ABI (include/m2s.h) and the helpers its translation units share.  Internal.
//   m2s_context.cpp  lifetime, setters, record pool, launch tags          m2s_upload.cpp   m2s_upload_scene / m2s_prepare
//   m2s_pass.cpp     the conversion pass driver (== ConversionPass::execute)   m2s_async.cpp    m2s_convert_submit / _wait
//   m2s_records.cpp  read-back, .ply export, record adoption               m2s_viewer.cpp   depth sort, viewer prepass
//   m2s_splat.cpp    the splat pass (== GaussianSplattingPass::execute) and its G-buffer
//   m2s_light.cpp    the shadow and relighting passes (== GaussianShadowPass / GaussianRelightingPass::execute)
//   m2s_meshdepth.cpp  the mesh depth prepass (== DepthPrepass::execute)
//   m2s_meshrender.cpp the mesh render pass (== MeshRenderPass::execute) and the mesh G-buffer
//   m2s_score.cpp    the fidelity score (m2s_score_frames): mesh frame against splat frame
//   m2s_contrib.cpp  the contribution pass and pruning (m2s_contrib_accumulate, m2s_prune)
//   m2s_bake.cpp     the light baked into spherical harmonics (m2s_bake_light, m2s_sh_shade_records, m2s_export_ply_sh)
#pragma once
#include "../../include/m2s.h"
#include "m2s_device.h"

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
}  // namespace m2s_host

constexpr int kBandSlotsMax = 64;   // (scene, R) entries remembered per context: band tables, decisions
struct m2s_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // scene
    void* tri_mem = nullptr;
    m2s::SceneDev scene{};
    m2s::MeshParams* d_meshes = nullptr;
    uint32_t* d_mesh_first = nullptr;
    uint32_t n_meshes_total = 0;
    bool has_scene = false;
    bool lean_ok = false;                   // every mesh of the scene samples its combo texture or no map at all: k_fused3 may run
    uint64_t range_first = 0, range_count = UINT64_MAX;

    // work buffers (sized by the scene)
    uint32_t* d_cnt = nullptr;
    uint32_t* d_off = nullptr;
    uint32_t* d_partials = nullptr;
    uint32_t* d_start = nullptr;
    size_t start_cap = 0;
    unsigned long long* d_total = nullptr;
    unsigned long long* h_total = nullptr;  // pinned, kPinnedWords words: [0] = fragment counter, [1] = status words of the fused kernel,
                                            // [2 + 2k], [3 + 2k] = the same of in-flight slot k, then one word each for the prepass and the depth sort
    static constexpr int kPinnedPrepass = 2 + 2 * M2S_MAX_IN_FLIGHT;   // m2s_prepass: TWO words — survivors, then the status words of its look-back
    static constexpr int kPinnedSortMM = 4 + 2 * M2S_MAX_IN_FLIGHT;    // the depth sorts: {min, max} of the keys (two 32-bit words); NOT the prepass's second word —
                                                                       // m2s_prepass_sorted uses both inside one call
    static constexpr int kPinnedWords = 6 + 2 * M2S_MAX_IN_FLIGHT;                  // (the sorts' word and the one behind it: {min, max}, {survivors, clash})
    unsigned long long* d_chain = nullptr;  // look-back chain of the fused kernel, one word per wave
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
    int warm_spec_form = 0;                             // ... ordered for the first resident set of this single-pass form's kernel
    uint32_t warm_spec_unit = 0, warm_spec_shift = 0;   // run table + dispatch order enqueued with the upload's count, for units of this many triangles (0: none)
    unsigned long long* d_bands = nullptr;  // kBandSlots run tables of run_table_words words each (RunInfo, m2s_device.h)
    size_t run_table_words = 0;
    uint32_t* d_run_order = nullptr;        // dispatch order of the runs (launch_run_order), built by warm_scene from the exact counts ...
    uint32_t run_order_unit = 0, run_order_shift = 0;   // ... for runs of (1 << shift) units of this many triangles (0: none)
    uint32_t* d_batch_first = nullptr;      // work-balanced batches of k_fused2 (small scenes; built from the first exact count)
    uint32_t n_batch_tab = 0;               // batches in it (0: uniform batches)
    size_t chain_words = 0;                 // words of d_chain (and of the second lane's chain)
    void* d_setup = nullptr;                // multi-pass pipeline: per-triangle TriSetup records (allocated at its first use)
    int last_pipeline = 0;                  // what the last conversion ran (m2s_last_pipeline)
    // second lane for context-owned asynchronous submissions: odd slots run on their own stream with their own chain
    // and record buffer, so that consecutive single-kernel conversions overlap (the tail of one, where the GPU drains,
    // with the head of the next) instead of paying ~8 us between dependent kernels on one stream
    int lanes = 1;                          // m2s_set_async_lanes
    hipStream_t stream_b = nullptr;
    unsigned long long* d_chain_b = nullptr;
    void* d_records_b = nullptr;
    uint64_t records_b_cap = 0;
    // ... and multi-pass conversions too: the second lane's own offsets / slice starts / TriSetup records / counter (allocated at
    // its first multi-pass submission), so that k_count_scan of conversion i + 1 runs beside k_emit2 of conversion i
    uint32_t* d_off_b = nullptr;
    uint32_t* d_start_b = nullptr;
    size_t start_b_cap = 0;
    void* d_setup_b = nullptr;
    unsigned long long* d_total_b = nullptr;
    int pipeline = M2S_PIPELINE_AUTO;
    uint32_t epoch = 0;                     // launch counter of the fused kernel (tags the chain words)

    // asynchronous submissions (m2s_convert_submit / m2s_convert_wait): a ring of result slots.  Slot k uses
    // h_total[2 + 2k] (counter) and h_total[3 + 2k] (status words), written by the kernel itself.
    struct Slot { hipEvent_t done = nullptr, t0 = nullptr, t1 = nullptr; uint64_t limit = 0; void* d_out = nullptr; uint32_t R = 0;
                  bool sync_result = false; uint64_t sync_total = 0; bool prof = false; float ms[M2S_K_N] = {};
                  int own_lane = -1; uint32_t gen = 0;   // context-owned buffer (0 / 1) and its generation at submission; -1: caller's buffer
                  bool wrote_bands = false; uint32_t bands_unit = 0; uint32_t ri_gen = 0;   // the launch leaves band bases behind, for the RInfo entry of that table generation
                  hipStream_t st = nullptr; bool shared_work = false; };   // stream it ran on; did it use the context's shared work buffers (chain, deferred list)?
    Slot slot[M2S_MAX_IN_FLIGHT];
    uint32_t slot_head = 0, slot_count = 0; // oldest in-flight slot, number in flight
    hipStream_t last_submit_stream = nullptr;   // stream of the newest in-flight submission (work buffers are shared: see submit)
    uint32_t buf_R[2] = { 0, 0 };           // context-owned record buffers (lane a / b): R of the newest conversion enqueued into it ...
    uint32_t buf_gen[2] = { 0, 0 };         // ... and a generation that advances whenever that R changes
    bool records_stale = false;             // the conversion last waited for has been overwritten by a later submission

    // output
    void* d_records = nullptr;
    uint64_t records_cap = 0;  // records
    const void* last_records = nullptr;
    int64_t cap_policy = -1;
    uint64_t last_total = 0, last_stored = 0;
    uint32_t last_R = 0;

    // depth sort (f-2)
    void* d_sorted = nullptr;
    uint64_t sorted_cap = 0, sorted_n = 0;
    uint32_t* d_sort_u32 = nullptr;   // keys_in | vals_in | keys_out | vals_out
    uint32_t sorted_key_offset = 0;   // keys_out holds key - this (m2s_device_sorted_keys adds it back once)
    void* d_sort_temp = nullptr;
    size_t sort_temp_cap = 0;
    uint64_t sort_u32_cap = 0;
    float last_sort_ms = 0.0f;
    float last_sort_stage_ms[3] = { 0, 0, 0 };   // keys | radix sort | gather of the last m2s_sort_by_depth (profiling on)
    // the positions of the current records as a compact plane (16 B each), left behind by the first depth sort after the records
    // changed and used for the keys of every later one (m2s_sort.hip); valid for (pos_plane_of, pos_plane_n, pos_plane_epoch)
    void* d_pos_plane = nullptr;
    uint64_t pos_plane_cap = 0, pos_plane_n = 0, pos_plane_epoch = 0;
    const void* pos_plane_of = nullptr;
    bool keep_positions = false;      // m2s_set_keep_positions: conversions leave the plane behind themselves where their kernel can (k_sparse)
    uint64_t records_epoch = 1;       // advances whenever the records behind last_records may have changed
    // viewer prepass (m2s_prepass): survivors, their depths, the look-back chain of its kernel, a copy of the depth image
    void* d_quads = nullptr;
    float* d_pp_depths = nullptr;
    uint64_t pp_cap = 0, pp_depths_cap = 0, pp_visible = 0;
    unsigned long long* d_pp_chain = nullptr;
    uint64_t pp_chain_words = 0;
    uint32_t pp_epoch = 0;
    float* d_pp_depthtex = nullptr;
    uint64_t pp_depthtex_cap = 0;
    float last_prepass_ms = 0.0f;
    m2s_gaussian* h_export[2] = { nullptr, nullptr };   // pinned chunk buffers of m2s_export_ply
    // upload staging: two pinned host chunks (filled by a few host threads while the previous chunk is on the bus) and
    // two device chunks for the AoS -> SoA repack; allocated at the first upload, kept
    void* h_stage[2] = { nullptr, nullptr };
    void* d_stage[2] = { nullptr, nullptr };
    hipEvent_t stage_ev[2] = { nullptr, nullptr };
    void* scene_arena = nullptr;             // one allocation for mesh table, textures, combo textures and work buffers
    float last_upload_ms[5] = { 0, 0, 0, 0, 0 }; // [0] total, [1] geometry, [2] textures + mips + combo, [3] allocations, [4] warm_scene
    void* d_rows = nullptr;                  // m2s_export_ply: .ply rows encoded on the device (formats 1 and 2)
    uint64_t rows_cap = 0;                   // bytes
    void* d_loaded = nullptr;                // m2s_upload_records (a loaded .ply)
    uint64_t loaded_cap = 0;
    void* d_sorted_quads = nullptr;          // m2s_sort_prepass
    uint64_t sq_cap = 0, sq_n = 0;
    float last_sort_prepass_ms = 0.0f;
    // splat pass (m2s_splat.cpp): the five G-buffer planes of the last call and the pass's grow-only work buffers
    void* d_gbuf[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    uint64_t gbuf_cap_px = 0;                // pixels every plane has room for
    int32_t gbuf_w = 0, gbuf_h = 0;          // resolution of the planes' contents (0: no splat has run)
    void* d_splat_rec = nullptr;             // per quad: 128-byte record, tile count (u32), exclusive scan of the counts (u64)
    uint32_t* d_splat_cnt = nullptr;
    unsigned long long* d_splat_off = nullptr;
    uint64_t splat_quad_cap = 0;
    uint32_t* d_splat_pairs = nullptr;       // keys_in | vals_in | keys_out | vals_out, splat_pairs_cap each
    uint64_t splat_pairs_cap = 0;
    uint32_t* d_splat_tiles = nullptr;       // ranges (2 words) | lengths | sorted lengths | order, splat_tiles_cap tiles each
    uint64_t splat_tiles_cap = 0;
    void* d_splat_temp = nullptr;            // scan / radix sort work area
    size_t splat_temp_cap = 0;
    unsigned long long* d_splat_totals = nullptr;   // [0] pairs, [1] skipped quads, [2] fragments blended
    unsigned long long* h_splat = nullptr;          // pinned copy of those three words
    float last_splat_ms = 0.0f;
    float last_splat_stage_ms[3] = { 0, 0, 0 };     // setup + bin, grouping, blend (profiling on)
    uint64_t last_splat_counts[3] = { 0, 0, 0 };    // pairs, fragments blended, quads skipped
    // sources of the sorted quads (m2s_prepass_sorted): which record each was made from.  Dense path: the first sq_n words of the
    // permutation in d_sort_u32 (an alias: dropped by whatever rewrites those words); compacting path: d_sq_src, written by k_prepass
    const uint32_t* sq_src = nullptr;        // nullptr: absent
    uint64_t sq_src_epoch = 0;               // records_epoch they index into
    uint32_t* d_sq_src = nullptr;
    uint64_t sq_src_cap = 0;
    // contribution pass and pruning (m2s_contrib.cpp): wmax | npix, contrib_cap words each, valid for (contrib_of, contrib_n, contrib_epoch)
    uint32_t* d_contrib = nullptr;
    uint64_t contrib_cap = 0, contrib_n = 0, contrib_epoch = 0;
    const void* contrib_of = nullptr;
    bool contrib_active = false;
    float last_contrib_ms = 0.0f;
    float last_contrib_stage_ms[3] = { 0, 0, 0 };
    uint32_t* d_prune_u32 = nullptr;         // flags | offsets, prune_cap words each, then two counters (u64)
    uint64_t prune_cap = 0;
    void* d_prune_temp = nullptr;            // scan work area
    uint64_t prune_temp_cap = 0;
    void* d_prune_stage = nullptr;           // survivors on their way back into the buffer they came from
    uint64_t prune_stage_cap = 0;            // bytes
    uint64_t last_prune_counts[4] = { 0, 0, 0, 0 };
    float last_prune_ms = 0.0f;
    hipEvent_t prune_ev[2] = {};
    // shadow pass (m2s_light.cpp): the six per-face quad lists back to back in one exact-size, grow-only buffer, the depth cube,
    // and the pass's grow-only work buffers
    void* d_shadow_quads = nullptr;          // 48 B each
    uint64_t shadow_quads_cap = 0;
    uint32_t shadow_base[7] = { 0, 0, 0, 0, 0, 0, 0 };   // first quad of every face's list; [6] = all quads (of the last m2s_shadow)
    bool shadow_lists = false;               // the lists of the last m2s_shadow exist (false after m2s_upload_shadow_cubemap)
    float* d_shadow_cube = nullptr;          // float[6][S][S]
    uint64_t shadow_cube_cap = 0;            // texels
    int32_t shadow_S = 0;                    // 0: no cube yet
    uint32_t* d_sh_tab = nullptr;            // stage A: counts | offsets, sh_tab_cap words each
    uint64_t sh_tab_cap = 0;
    float* d_sh_views = nullptr;             // six view matrices (96 floats) | bases (8 words)
    void* d_sh_rec = nullptr;                // stage B: per quad 48-byte record, tile count (u32), scan of the counts (u64)
    uint32_t* d_sh_cnt = nullptr;
    unsigned long long* d_sh_off = nullptr;
    uint64_t sh_quad_cap = 0;
    uint32_t* d_sh_pairs = nullptr;          // keys_in | vals_in | keys_out | vals_out, sh_pairs_cap each
    uint64_t sh_pairs_cap = 0;
    void* d_sh_temp = nullptr;               // scan / radix sort work area
    uint64_t sh_temp_cap = 0;
    unsigned long long* d_sh_totals = nullptr;   // [0] pairs, [1] skipped quads, [2] atomics sent
    unsigned long long* h_sh = nullptr;          // pinned: those three words, then the bases
    hipEvent_t light_ev[10] = {};
    float last_shadow_ms = 0.0f;
    float last_shadow_stage_ms[3] = { 0, 0, 0 };    // stage A (count + scan + emit), setup + binning, raster (profiling on)
    uint64_t last_shadow_counts[9] = {};            // quads of face 0..5, (tile, quad) pairs, texel writes (atomics sent), quads skipped
    // relighting pass: the frame, the optional plane of shadow counts
    uint32_t* d_frame = nullptr;
    uint8_t* d_shadow_counts = nullptr;
    uint64_t frame_cap_px = 0;
    int32_t frame_w = 0, frame_h = 0;        // 0: no relight has run
    bool frame_has_counts = false;
    float last_relight_ms = 0.0f;
    // mesh depth prepass (m2s_meshdepth.cpp): the image and the pass's grow-only work buffers
    float* d_md_image = nullptr;             // float[H][W], row 0 = bottom
    uint64_t md_image_cap = 0;               // texels
    int32_t md_w = 0, md_h = 0;              // 0: no image yet
    int32_t md_inplace = -1;                 // m2s_debug_set_mesh_depth_inplace (-1: the default, kMdInplace)
    uint32_t* d_md_deferred = nullptr;       // triangles the setup kernel left to the binned path (capacity: md_tri_cap)
    uint64_t md_tri_cap = 0;
    void* d_md_rec = nullptr;                // per deferred triangle six slots: 48-byte record, tile count (u32), scan of the counts (u64)
    uint32_t* d_md_cnt = nullptr;
    unsigned long long* d_md_off = nullptr;
    uint64_t md_slot_cap = 0;
    uint32_t* d_md_pairs = nullptr;          // keys_in | vals_in | keys_out | vals_out, md_pairs_cap each
    uint64_t md_pairs_cap = 0;
    void* d_md_temp = nullptr;               // scan / radix sort work area
    uint64_t md_temp_cap = 0;
    unsigned long long* d_md_totals = nullptr;   // 8 words: see meshdepth_setup
    unsigned long long* h_md = nullptr;          // pinned copy
    hipEvent_t md_ev[6] = {};
    float last_md_ms = 0.0f;
    float last_md_stage_ms[3] = { 0, 0, 0 };     // setup + in-place, clip + binning, tile raster (profiling on)
    uint64_t last_md_counts[5] = {};             // drawn, clipped, non-finite, pairs, texel updates sent
    // mesh render pass (m2s_meshrender.cpp): the visibility image and the mesh G-buffer; its work buffers are the mesh depth prepass's
    unsigned long long* d_mr_vis = nullptr;      // uint64[H][W], row 0 = bottom: (bits of z) << 32 | global triangle index
    uint64_t mr_vis_cap = 0;                     // pixels
    void* d_mr_gbuf[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };   // layouts of d_gbuf
    uint64_t mr_gbuf_cap_px[5] = { 0, 0, 0, 0, 0 };   // pixels each plane has room for
    int32_t mr_w = 0, mr_h = 0;                  // 0: no mesh G-buffer yet
    hipEvent_t mr_ev[2] = {};
    float last_mr_ms = 0.0f;
    float last_mr_stage_ms[4] = { 0, 0, 0, 0 };  // visibility setup + in-place, clip + binning, tile raster, shading (profiling on)
    uint64_t last_mr_counts[6] = {};             // drawn, clipped, non-finite, pairs, texel updates sent, culled as back-facing
    // fidelity score (m2s_light.cpp: m2s_relight_mesh; m2s_score.cpp): the mesh-lit frame, the comparison's counters and error map
    uint32_t* d_mesh_frame = nullptr;            // uchar4[H][W], row 0 = bottom
    uint64_t mesh_frame_cap_px = 0;
    int32_t mesh_frame_w = 0, mesh_frame_h = 0;  // 0: no m2s_relight_mesh has run
    unsigned long long* d_score_acc = nullptr;   // kScoreShards x kScoreCounters words (m2s_device.h), summed on the host
    unsigned long long* h_score = nullptr;       // pinned copy
    uint32_t* d_score_map = nullptr;             // uchar4[H][W]
    uint64_t score_map_cap_px = 0;
    int32_t score_map_w = 0, score_map_h = 0;    // 0: the last m2s_score_frames kept no map
    hipEvent_t score_ev[2] = {};
    float last_score_ms = 0.0f;

    // light baked into spherical harmonics (m2s_bake.cpp): the coefficient plane, the optional tap counts, the quadrature table
    float* d_sh = nullptr;                       // float[n][48]: f_dc[3], f_rest[45] channel-major
    uint64_t sh_cap = 0, sh_n = 0;               // records it has room for / holds
    bool sh_valid = false;                       // a bake has completed since the plane was last (re)allocated
    const void* sh_of = nullptr;                 // the records it was baked from, and their records_epoch when they were the context's
    uint64_t sh_epoch = 0;                       // (0: the caller's records) — m2s_prune compacts the plane of the records it compacts
    uint8_t* d_bake_counts = nullptr;            // uint8[n]
    uint64_t bake_counts_cap = 0;
    bool bake_has_counts = false;
    float* d_bake_table = nullptr;               // n_theta * n_phi rows of kBakeTableRow floats
    uint32_t bake_table_nt = 0, bake_table_np = 0;
    hipEvent_t bake_ev[2] = {};
    float last_bake_ms = 0.0f;

    // measurement
    bool profiling = false;
    hipEvent_t ev[8] = {};
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

namespace m2s_host {
inline m2s_status fail(m2s_ctx* c, m2s_status s, const std::string& msg) {
    if (c) c->err = msg;
    return s;
}
constexpr int kBandSlots = kBandSlotsMax;

// m2s_context.cpp
// Waiting for a conversion.  The runtime's hipStreamSynchronize / hipEventSynchronize hand the caller back 10-18 us after the last
// kernel has finished — 8-13 % of a 0.12 ms conversion, the reference's glFinish (ConversionPass.cpp:54).  These poll the same
// completion signal (hipStreamQuery / hipEventQuery: the stream's own "all work done") for up to 400 us and only then block.
hipError_t wait_stream(hipStream_t st);
hipError_t wait_event(hipEvent_t ev);
void free_scene(m2s_ctx* c);
m2s_ctx::RInfo& rinfo_for(m2s_ctx* c, uint32_t R);
void drain_in_flight(m2s_ctx* c);          // every conversion still in flight has finished when this returns
hipError_t next_epoch(m2s_ctx* c, uint32_t* out);
m2s_status ensure_records(m2s_ctx* c, uint64_t want);
// m2s_upload.cpp
m2s_status ensure_stage(m2s_ctx* c);
// A grow-only device buffer of `want` units of `unit` bytes: kept when large enough, else freed and allocated anew (contents lost).
template <typename T>
inline m2s_status grow_buffer(m2s_ctx* c, T*& p, uint64_t& cap, uint64_t want, size_t unit) {
    if (cap >= want) return M2S_OK;
    if (p) { (void)hipFree((void*)p); p = nullptr; }
    cap = 0;
    void* q = nullptr;
    HIPCHK(c, hipMalloc(&q, (size_t)want * unit < 256 ? 256 : (size_t)want * unit));
    p = static_cast<T*>(q);
    cap = want;
    return M2S_OK;
}
// m2s_splat.cpp
// The stages of the splat pass in front of the blend — setup / bin, pairs, grouping by tile, tile order — over n quads on a W x H
// viewport, in the context's splat work buffers: what m2s_splat and m2s_contrib_accumulate both start with.  Records ev[0..4] when
// profiling (setup: 0-1, pairs: 2-3, grouping: 3-4); synchronises once (the pair count).  vals / ranges / order are NULL without pairs.
struct SplatBins { const uint32_t* vals = nullptr; const uint2* ranges = nullptr; const uint32_t* order = nullptr; uint64_t pairs = 0, skipped = 0; };
m2s_status splat_bin(m2s_ctx* c, const void* d_quads, uint32_t nq, int W, int H, SplatBins* out);
m2s_status splat_stage_ms(m2s_ctx* c, bool any_quads, float out[3]);   // ... and their times + the blend's (ev[4..5]), profiling on
// m2s_meshdepth.cpp
// What the mesh depth prepass and the visibility stage of the mesh render pass share: clear, setup + in-place lanes, clipper + binning,
// tile raster over `image` (float[W * H], or uint64[W * H] when vis), synchronous.  ms: the three stage times (profiling on);
// c->h_md holds the pass's totals afterwards (m2s_device.h: meshdepth_setup, meshvis_setup).
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
m2s_status enqueue_multipass(m2s_ctx* c, uint32_t R, float4* d_out, uint64_t limit, bool prof,
                             unsigned long long* h_res, hipStream_t st, bool second_lane = false);
m2s_status ensure_second_lane(m2s_ctx* c);                       // stream, chain and record buffer of the second lane
m2s_status ensure_second_lane_multipass(m2s_ctx* c, uint32_t n_start);   // ... and its multi-pass work buffers
m2s_status run_pass(m2s_ctx* c, uint32_t R, void* d_user, uint64_t user_cap, hipStream_t st, uint64_t* out_total,
                    bool from_submit = false);
}  // namespace m2s_host
