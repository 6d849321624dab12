// m2s_lod.cpp — the level-of-detail tree and its per-camera cut (m2s_lod_build, m2s_lod_select, m2s_lod_select_budget, their
// _frustum and _occluded forms, m2s_lod_blend): host side of m2s_lod.hip, m2s_lodbudget.hip, m2s_lodfrustum.hip and m2s_lodblend.hip.  The tree is a chain of the merge pass's steps (merge_run, m2s_merge.cpp) whose results are
// copied into a node pool and linked by their maps; the
// cut's flags and offsets live where m2s_prune leaves its own, and the compaction is m2s_prune's (m2s_contrib.cpp: prune_compact_enqueue);
// what a cut does to the context: m2s_recstate.h, Rewrite::LodCut.  The tree itself (c->lod) and what the passes work in (c->lod_work):
// m2s_lodtree.h.
#include "m2s_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace m2s;
using namespace m2s_host;

namespace {

constexpr uint64_t kLodMaxNodes = 0xFFFFFFFFull;   // fewer than this: M2S_LOD_NO_PARENT is no node

const char* const kNoTreeMsg = "no level-of-detail tree (m2s_lod_build)";

bool lod_ids_valid(const m2s_ctx* c) { return c->lod_ids_tag.holds(*c); }

// The state every cut and the blend need behind their argument checks: nothing in flight, a tree.
m2s_status lod_ready(m2s_ctx* c) {
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    if (!c->lod.levels) return fail(c, M2S_ERR_STATE, kNoTreeMsg);
    return M2S_OK;
}

// The camera of a cut, a budget search or a blend, in the order their parameter checks report it; tau_px (NULL: the caller has none, or
// checks its own later) between the focal length and the near distance.
m2s_status lod_camera_check(m2s_ctx* c, const float position[3], float focal_px, float near, const float* tau_px = nullptr) {
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(position[k])) return fail(c, M2S_ERR_INVALID, "camera_position is not finite");
    if (!std::isfinite(focal_px) || !(focal_px > 0.0f)) return fail(c, M2S_ERR_INVALID, "focal_px is not finite or not positive");
    if (tau_px && (!std::isfinite(*tau_px) || !(*tau_px >= 0.0f))) return fail(c, M2S_ERR_INVALID, "tau_px is not finite or negative");
    if (!std::isfinite(near) || !(near > 0.0f)) return fail(c, M2S_ERR_INVALID, "near is not finite or not positive");
    return M2S_OK;
}

LodFrustumK lod_frustum_k(const m2s_lod_frustum* fr) {
    LodFrustumK f;
    std::memcpy(f.M, fr->model_to_world, sizeof(f.M));
    std::memcpy(f.V, fr->world_to_view, sizeof(f.V));
    std::memcpy(f.P, fr->view_to_clip, sizeof(f.P));
    f.guard = fr->guard_band;
    return f;
}

m2s_status lod_frustum_check(m2s_ctx* c, const m2s_lod_frustum* fr) {
    if (!fr) return fail(c, M2S_ERR_INVALID, "no frustum");
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(fr->model_to_world[k]) || !std::isfinite(fr->world_to_view[k]) || !std::isfinite(fr->view_to_clip[k]))
            return fail(c, M2S_ERR_INVALID, "a matrix entry of the frustum is not finite");
    if (!std::isfinite(fr->guard_band) || !(fr->guard_band >= 1.0f)) return fail(c, M2S_ERR_INVALID, "guard_band is not finite or below 1");
    if (fr->reserved[0] || fr->reserved[1] || fr->reserved[2]) return fail(c, M2S_ERR_INVALID, "a reserved word of the frustum is not 0");
    return M2S_OK;
}

// pin 4 of the occluded cuts, but for the state of the context (lod_occluder_state)
m2s_status lod_occluder_check(m2s_ctx* c, const m2s_lod_occluder* oc) {
    if (!oc) return fail(c, M2S_ERR_INVALID, "no occluder");
    if (!std::isfinite(oc->depth_bias) || !(oc->depth_bias >= 0.0f)) return fail(c, M2S_ERR_INVALID, "depth_bias is not finite or negative");
    if (oc->reserved[0] || oc->reserved[1]) return fail(c, M2S_ERR_INVALID, "a reserved word of the occluder is not 0");
    if (oc->depth && (!oc->depth_w || !oc->depth_h)) return fail(c, M2S_ERR_INVALID, "a depth image of width or height 0");
    if (!oc->depth && c->md_w && (oc->depth_w || oc->depth_h) && (oc->depth_w != (uint32_t)c->md_w || oc->depth_h != (uint32_t)c->md_h))
        return fail(c, M2S_ERR_INVALID, "depth is NULL and depth_w x depth_h is not the size of the context's mesh depth image");
    return M2S_OK;
}

m2s_status lod_occluder_state(m2s_ctx* c, const m2s_lod_occluder* oc) {
    if (!oc->depth && !c->md_w) return fail(c, M2S_ERR_STATE, "depth is NULL and no m2s_mesh_depth has run");
    return M2S_OK;
}

// The visibility plane of the tree's N > 0 nodes for one frustum, timed by lod_vis_clock, which whoever calls this has opened for the call
// (in front of its test for an empty tree, so that the cut reads 0 where this never ran).
// The cut's count words are zeroed here, in front of the stage that writes the first of them.
// oc (NULL: none): the leaves are tested against this depth image too; a host image is copied in front of the stage, into a buffer
// that no other pass reads.
m2s_status lod_vis_enqueue(m2s_ctx* c, const m2s_lod_frustum* fr, const m2s_lod_occluder* oc) {
    M2S_TRY(c->lod_work.vis.reserve(c->err, c->lod.nodes(), 1));
    M2S_TRY(c->lod_work.counts.reserve(c->err, kLodCountWords, sizeof(uint32_t)));
    LodOccluderK ok = {};
    if (oc) {
        ok.nodes = c->lod.rows<const float>(kLodRecords);
        ok.bias = oc->depth_bias;
        if (!oc->depth) {
            ok.depth = c->d_md_image; ok.depth_w = (uint32_t)c->md_w; ok.depth_h = (uint32_t)c->md_h;
        } else {
            ok.depth_w = oc->depth_w; ok.depth_h = oc->depth_h;
            if (oc->depth_on_device) ok.depth = oc->depth;
            else {
                const uint64_t texels = (uint64_t)oc->depth_w * oc->depth_h;
                M2S_TRY(c->lod_work.occ_depth.reserve(c->err, texels, sizeof(float)));
                HIPCHK(c, hipMemcpyAsync(c->lod_work.occ_depth, oc->depth, texels * sizeof(float), hipMemcpyHostToDevice, c->stream));
                ok.depth = c->lod_work.occ_depth;
            }
        }
        if (!ok.depth || !ok.depth_w || !ok.depth_h) return fail(c, M2S_ERR_STATE, "the occluder has no depth image (internal error)");
    }
    HIPCHK(c, hipMemsetAsync(c->lod_work.counts, 0, kLodCountWords * sizeof(uint32_t), c->stream));
    HIPCHK(c, c->lod_vis_clock.mark(SpanMark::Begin, c->stream));
    HIPCHK(c, lod_visibility(c->lod.levels_k<LodLevelsK>(), lod_frustum_k(fr), oc ? &ok : nullptr, c->lod_work.vis, c->lod_work.counts + kLodInsideWord, c->stream));
    HIPCHK(c, c->lod_vis_clock.mark(SpanMark::End, c->stream));
    return M2S_OK;
}

// The cut behind m2s_lod_select's checks of its arguments and the context's state (m2s_lod_select_budget takes its own through it).
// fr (NULL: the plain cut): only nodes with a leaf inside this frustum are selected.  vis: who runs lod_vis_enqueue for it, which also
// zeroes the cut's count words in front of the inside count it adds to them.  oc (NULL: none; only with fr): ... and not behind this image.
enum class LodVis { None, Here, Enqueued };     // no frustum | lod_cut enqueues it | the caller has, earlier on the stream (the budget search reads the plane first)
m2s_status lod_cut(m2s_ctx* c, const m2s_lod_select_params* p, uint64_t out_counts[4], const m2s_lod_frustum* fr, LodVis vis,
                   const m2s_lod_occluder* oc = nullptr) {
    if ((fr != nullptr) != (vis != LodVis::None) || (oc && !fr)) return fail(c, M2S_ERR_INVALID, "lod_cut: frustum and visibility mode disagree (internal error)");
    const bool dry = (p->flags & M2S_LOD_DRY_RUN) != 0;
    const bool with_sh = c->lod.has_sh && !dry;     // (pin 3s: the tree's property decides, not the switch at the time of the cut)
    ClockOf<LodCutMark>& clock = c->lod_cut_clock;
    const uint32_t levels = c->lod.levels;
    const uint64_t N = c->lod.nodes();
    HIPCHK(c, hipSetDevice(c->device));
    M2S_TRY(clock.begin(c->err, c->profiling));
    if (vis == LodVis::Here) M2S_TRY(c->lod_vis_clock.begin(c->err, c->profiling));
    uint32_t h[kLodCountWords] = {};
    uint64_t selected = 0;
    if (N) {
        M2S_TRY(c->lod_work.open.reserve(c->err, N, 1));
        M2S_TRY(c->lod_work.counts.reserve(c->err, kLodCountWords, sizeof(uint32_t)));
        M2S_TRY(c->d_prune_u32.reserve(c->err, N, 2 * sizeof(uint32_t)));
        if (!dry) {
            M2S_TRY(c->d_prune_temp.reserve(c->err, align_up(prune_scan_temp_bytes((uint32_t)N), 16) + 2 * sizeof(unsigned long long), 1));
            M2S_TRY(c->lod_work.ids.reserve(c->err, N, sizeof(uint32_t)));
            c->lod_ids_tag.clear();
        }
        uint32_t* const flags = c->d_prune_u32;
        uint32_t* const offsets = flags + c->d_prune_u32.cap();
        const LodSelectK k = { p->camera_position[0], p->camera_position[1], p->camera_position[2], p->focal_px, p->tau_px * p->tau_px, p->near * p->near };
        if (vis == LodVis::Here) M2S_TRY(lod_vis_enqueue(c, fr, oc));
        HIPCHK(c, clock.mark(LodCutMark::Start, c->stream));
        // (with a frustum the words were zeroed by lod_vis_enqueue, here or in the caller, and hold the inside count by now: not again)
        if (vis == LodVis::None) HIPCHK(c, hipMemsetAsync(c->lod_work.counts, 0, kLodCountWords * sizeof(uint32_t), c->stream));
        HIPCHK(c, lod_sweep(c->lod.levels_k<LodLevelsK>(), k, c->lod_work.open, flags, c->lod_work.counts, fr ? c->lod_work.vis.get() : nullptr, c->stream));
        HIPCHK(c, clock.mark(LodCutMark::Swept, c->stream));
        if (!dry) {
            HIPCHK(c, lod_scan(flags, offsets, (uint32_t)N, c->d_prune_temp, c->d_prune_temp.cap() - 2 * sizeof(unsigned long long), c->stream));
            HIPCHK(c, lod_node_ids(flags, offsets, (uint32_t)N, c->lod_work.ids, c->stream));
            HIPCHK(c, clock.mark(LodCutMark::Indexed, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(h, c->lod_work.counts, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint32_t l = 0; l < levels; ++l) selected += h[l];
        // (a frustum may leave nothing; the plain cut holds every leaf's ancestor-or-self)
        if ((selected < 1 && !fr) || selected > N || h[kLodRefineWord] > N || (fr && (h[kLodPlainWord] < selected || h[kLodPlainWord] > N || h[kLodInsideWord] > N)) ||
            (uint64_t)h[kLodOccludedWord] + h[kLodKeptWord] > h[kLodInsideWord])
            return fail(c, M2S_ERR_HIP, "the cut's counts came back inconsistent");
        if (!dry) {
            M2S_TRY(prune_compact_enqueue(c, N, selected, flags, offsets, false, c->lod.rows<const void>(kLodRecords)));
            if (with_sh) {
                // the selected nodes' rows of the tree's plane, by the same flags and offsets, straight into the context's plane (the
                // source is the tree's: nothing lands on itself); whatever plane the context had is gone from here on
                c->sh_tag.clear();
                c->bake_has_counts = false;
                M2S_TRY(c->d_sh.reserve(c->err, std::max<uint64_t>(selected, 1), 48 * sizeof(float)));
                if (selected) HIPCHK(c, prune_compact(c->lod.rows<const float4>(kLodSh), flags, offsets, (uint32_t)N, kMergeShLanes, (float4*)c->d_sh.get(), c->stream));
            }
            HIPCHK(c, clock.mark(LodCutMark::Compacted, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    } else {
        if (!dry) {
            c->lod_ids_tag.clear();
            M2S_TRY(prune_compact_enqueue(c, 0, 0, nullptr, nullptr, false));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    if (clock.on()) {   // (a dry run records neither Indexed nor Compacted, an empty tree nothing: those spans are 0)
        float* ms = c->last_lod_select_stage_ms;
        HIPCHK(c, clock.span(LodCutMark::Start, LodCutMark::Swept, &ms[0]));
        HIPCHK(c, clock.span(LodCutMark::Swept, LodCutMark::Indexed, &ms[1]));
        HIPCHK(c, clock.span(LodCutMark::Indexed, LodCutMark::Compacted, &ms[2]));   // (the round trip of the counts included)
        if (fr) HIPCHK(c, c->lod_vis_clock.span(SpanMark::Begin, SpanMark::End, &c->last_lod_frustum_ms));   // (an empty tree: 0 too)
    }
    if (!dry) {
        // (a baked plane of the context is one of other records: dropped; a tree with a plane has left the selected nodes' rows in its place)
        c->rewritten(c->lane[0].records, selected, c->lod.R, with_sh ? Rewrite::LodCutWithSh : Rewrite::LodCut);
        if (with_sh) c->sh_degree = c->lod.sh_degree;
        c->lod_ids_tag.set(*c, selected);
        c->lod_work.ids_gen = c->lod.gen;                                // (which tree the indices are of: m2s_lod_blend reads it through them)
    }
    c->last_lod_select_counts[0] = N; c->last_lod_select_counts[1] = selected; c->last_lod_select_counts[2] = h[0];
    c->last_lod_select_counts[3] = h[kLodRefineWord];
    for (uint32_t l = 0; l <= M2S_LOD_MAX_STEPS; ++l) c->last_lod_level_counts[l] = l < levels ? h[l] : 0;
    if (fr) { c->last_lod_frustum_counts[0] = h[kLodInsideWord]; c->last_lod_frustum_counts[1] = h[kLodPlainWord] - selected; }
    if (oc) {
        c->last_lod_occlusion_counts[0] = h[kLodInsideWord]; c->last_lod_occlusion_counts[1] = h[kLodOccludedWord];
        c->last_lod_occlusion_counts[2] = h[kLodKeptWord]; c->last_lod_occlusion_counts[3] = h[kLodPlainWord] - selected;
    }
    if (out_counts) std::memcpy(out_counts, c->last_lod_select_counts, sizeof(c->last_lod_select_counts));
    return M2S_OK;
}

m2s_status lod_select_check(m2s_ctx* c, const m2s_lod_select_params* p) {
    M2S_TRY(lod_camera_check(c, p->camera_position, p->focal_px, p->near, &p->tau_px));
    if ((p->flags & ~(uint32_t)M2S_LOD_DRY_RUN) || p->reserved != 0) return fail(c, M2S_ERR_INVALID, "unknown flag bits or reserved != 0");
    return M2S_OK;
}

m2s_status lod_budget_check(m2s_ctx* c, const m2s_lod_budget_params* p) {
    M2S_TRY(lod_camera_check(c, p->camera_position, p->focal_px, p->near));
    if (!std::isfinite(p->tau_min_px) || !(p->tau_min_px >= 0.0f)) return fail(c, M2S_ERR_INVALID, "tau_min_px is not finite or negative");
    if (p->max_records < 1) return fail(c, M2S_ERR_INVALID, "max_records is 0");
    if (p->flags & ~(uint32_t)M2S_LOD_DRY_RUN) return fail(c, M2S_ERR_INVALID, "unknown flag bits");
    return M2S_OK;
}

// m2s_lod_select_budget behind its checks.  fr (NULL: the plain search): the nodes without a leaf inside are selected at no key, and
// the budget is raised to the visible nodes of the last level on the device.  oc (NULL: none; only with fr): as for lod_cut.
m2s_status lod_budget(m2s_ctx* c, const m2s_lod_budget_params* p, const m2s_lod_frustum* fr, m2s_lod_budget_result* out, uint64_t out_counts[4],
                      const m2s_lod_occluder* oc = nullptr) {
    ClockOf<LodBudgetMark>& clock = c->lod_budget_clock;
    const uint64_t N = c->lod.nodes(), last = N - c->lod.first[c->lod.levels - 1];
    uint32_t floor_key = 0, key = 0;
    if (p->tau_min_px > 0.0f) std::memcpy(&floor_key, &p->tau_min_px, sizeof(floor_key));
    uint32_t h[3] = {};                                                 // prefix, below, finer
    HIPCHK(c, hipSetDevice(c->device));
    M2S_TRY(clock.begin(c->err, c->profiling));
    if (fr) M2S_TRY(c->lod_vis_clock.begin(c->err, c->profiling));
    if (N) {
        M2S_TRY(c->lod_work.lh.reserve(c->err, N, sizeof(uint2)));
        M2S_TRY(c->lod_work.budget_state.reserve(c->err, kLodBudgetStateWords, sizeof(uint32_t)));
        const uint32_t n_eff = fr ? p->max_records : (uint32_t)std::max<uint64_t>(p->max_records, last);
        const LodSelectK k = { p->camera_position[0], p->camera_position[1], p->camera_position[2], p->focal_px, 0.0f, p->near * p->near };
        if (fr) M2S_TRY(lod_vis_enqueue(c, fr, oc));
        HIPCHK(c, clock.mark(LodBudgetMark::Start, c->stream));
        uint2* const lh = static_cast<uint2*>(c->lod_work.lh.get());
        HIPCHK(c, lod_thresholds(c->lod.levels_k<LodLevelsK>(), k, lh, fr ? c->lod_work.vis.get() : nullptr, c->stream));
        HIPCHK(c, clock.mark(LodBudgetMark::Thresholds, c->stream));
        HIPCHK(c, lod_budget_search(lh, (uint32_t)N, n_eff, fr != nullptr, c->lod_work.budget_state, c->stream));
        HIPCHK(c, clock.mark(LodBudgetMark::Searched, c->stream));
        HIPCHK(c, hipMemcpyAsync(h, c->lod_work.budget_state, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        key = h[kLodBudgetPrefix];
        if (key > 0x7F7FFFFFu) return fail(c, M2S_ERR_HIP, "the budget search came back with no finite tau_px");
    }
    const bool by_floor = floor_key > key;
    if (by_floor) key = floor_key;
    m2s_lod_select_params sp = {};
    std::memcpy(sp.camera_position, p->camera_position, sizeof(sp.camera_position));
    sp.focal_px = p->focal_px;
    std::memcpy(&sp.tau_px, &key, sizeof(key));
    sp.near = p->near;
    sp.flags = p->flags;
    uint64_t counts[4] = {};
    M2S_TRY(lod_cut(c, &sp, counts, fr, fr ? LodVis::Enqueued : LodVis::None, oc));
    if (clock.on()) {
        float* ms = c->last_lod_budget_stage_ms;
        HIPCHK(c, clock.span(LodBudgetMark::Start, LodBudgetMark::Thresholds, &ms[0]));      // (an empty tree: 0, like the next)
        HIPCHK(c, clock.span(LodBudgetMark::Thresholds, LodBudgetMark::Searched, &ms[1]));
        ms[2] = (c->last_lod_select_stage_ms[0] + c->last_lod_select_stage_ms[1]) + c->last_lod_select_stage_ms[2];
    }
    if (out) {
        out->tau_px = sp.tau_px;
        out->met = counts[1] <= p->max_records ? 1u : 0u;
        out->selected_finer = (!N || key == 0 || by_floor) ? counts[1] : h[kLodBudgetFiner];
    }
    if (out_counts) std::memcpy(out_counts, counts, sizeof(counts));
    return M2S_OK;
}

m2s_status lod_blend_check(m2s_ctx* c, const m2s_lod_blend_params* p) {
    M2S_TRY(lod_camera_check(c, p->camera_position, p->focal_px, p->near, &p->tau_px));
    if (!std::isfinite(p->band) || !(p->band > 0.0f) || !(p->band <= 1.0f)) return fail(c, M2S_ERR_INVALID, "band is not finite or outside (0, 1]");
    if (p->reserved != 0) return fail(c, M2S_ERR_INVALID, "reserved != 0");
    return M2S_OK;
}

// m2s_lod_blend behind its checks of the arguments and the state: the n records of the last cut, which live in the pool, are rewritten
// there out of the tree (the source is never the pool: nothing lands on itself), and the rows of the context's plane out of the tree's.
m2s_status lod_blend(m2s_ctx* c, const m2s_lod_blend_params* p, uint64_t out_counts[4]) {
    const uint64_t n = c->lod_ids_tag.n;
    const bool with_sh = c->lod.has_sh && c->sh_tag.holds(*c, n);       // (pin 6)
    ClockOf<LodBlendMark>& clock = c->lod_blend_clock;
    uint32_t h[kLodBlendCountWords] = {};
    HIPCHK(c, hipSetDevice(c->device));
    M2S_TRY(clock.begin(c->err, true));                                 // (measured whatever m2s_set_profiling says)
    c->lod_work.blend_tag.clear();
    if (n) {
        M2S_TRY(c->lod_work.blend_t.reserve(c->err, n, sizeof(float)));
        M2S_TRY(c->lod_work.blend_counts.reserve(c->err, kLodBlendCountWords, sizeof(uint32_t)));
        float4* const pool = (float4*)c->lane[0].records.get();
        const uint32_t* const parent = c->lod.rows<const uint32_t>(kLodParent);
        const LodBlendK k = { p->camera_position[0], p->camera_position[1], p->camera_position[2], p->focal_px, p->tau_px * p->tau_px, p->near * p->near, p->band };
        HIPCHK(c, hipMemsetAsync(c->lod_work.blend_counts, 0, kLodBlendCountWords * sizeof(uint32_t), c->stream));
        HIPCHK(c, clock.mark(LodBlendMark::Start, c->stream));
        HIPCHK(c, lod_blend_weights(c->lod_work.ids, parent, c->lod.rows<const float4>(kLodBounds), (uint32_t)n, k, c->lod_work.blend_t, c->lod_work.blend_counts, c->stream));
        HIPCHK(c, clock.mark(LodBlendMark::Weighted, c->stream));
        HIPCHK(c, lod_blend_records(c->lod.rows<const float4>(kLodRecords), c->lod_work.ids, parent, c->lod_work.blend_t, (uint32_t)n, pool, c->lod_work.blend_counts, c->stream));
        HIPCHK(c, clock.mark(LodBlendMark::Blended, c->stream));
        if (with_sh) {
            HIPCHK(c, lod_blend_sh(c->lod.rows<const float4>(kLodSh), c->lod_work.ids, parent, c->lod_work.blend_t, (uint32_t)n, (float4*)c->d_sh.get(), c->stream));
            HIPCHK(c, clock.mark(LodBlendMark::ShBlended, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(h, c->lod_work.blend_counts, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (h[kLodBlendBlended] > n || h[kLodBlendSaturated] > h[kLodBlendBlended] || h[kLodBlendTurned] > h[kLodBlendBlended])
            return fail(c, M2S_ERR_HIP, "the blend's counts came back inconsistent");
    }
    float* ms = c->last_lod_blend_stage_ms;                             // (zero records record nothing: those spans are 0)
    HIPCHK(c, clock.span(LodBlendMark::Start, LodBlendMark::Weighted, &ms[0]));
    HIPCHK(c, clock.span(LodBlendMark::Weighted, LodBlendMark::Blended, &ms[1]));
    HIPCHK(c, clock.span(LodBlendMark::Blended, LodBlendMark::ShBlended, &ms[2]));
    HIPCHK(c, clock.span(LodBlendMark::Start, with_sh ? LodBlendMark::ShBlended : LodBlendMark::Blended, &c->last_lod_blend_ms));
    // pin 7: what a cut does to the context, then the two planes the cut and this pass left are the new records' again
    c->rewritten(c->lane[0].records, n, c->lod.R, with_sh ? Rewrite::LodCutWithSh : Rewrite::LodCut);
    if (with_sh) c->sh_degree = c->lod.sh_degree;
    c->lod_ids_tag.set(*c, n);
    c->lod_work.blend_tag.set(*c, n);
    c->last_lod_blend_counts[0] = n; c->last_lod_blend_counts[1] = h[kLodBlendBlended]; c->last_lod_blend_counts[2] = h[kLodBlendSaturated];
    c->last_lod_blend_counts[3] = h[kLodBlendTurned];
    if (out_counts) std::memcpy(out_counts, c->last_lod_blend_counts, sizeof(c->last_lod_blend_counts));
    return M2S_OK;
}

}  // namespace

extern "C" {

m2s_status m2s_lod_blend(m2s_ctx* c, const m2s_lod_blend_params* p, uint64_t out_counts[4]) {
    if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
    if (!c || !p) return M2S_ERR_INVALID;
    M2S_TRY(lod_blend_check(c, p));
    M2S_TRY(lod_ready(c));
    if (c->lod.model != M2S_MERGE_MODEL_FOOTPRINT)
        return fail(c, M2S_ERR_STATE, "the tree was built under M2S_MERGE_MODEL_GAUSSIAN: the blend's frame turns and axis-by-axis lerp assume the footprint's axis order");
    if (!lod_ids_valid(c) || c->lod_work.ids_gen != c->lod.gen || c->last_records != c->lane[0].records.get() || c->last_stored != c->lod_ids_tag.n)
        return fail(c, M2S_ERR_STATE, "the current records are not what the last cut of this tree left (m2s_lod_select without M2S_LOD_DRY_RUN first)");
    return lod_blend(c, p, out_counts);
}

const void* m2s_device_lod_blend_t(const m2s_ctx* c) { return c && c->lod_work.blend_tag.holds(*c) && c->lod_work.blend_tag.n ? c->lod_work.blend_t.get() : nullptr; }

m2s_status m2s_download_lod_blend_t(m2s_ctx* c, float* dst, uint64_t capacity, uint64_t* out_n) {
    if (out_n) *out_n = 0;
    if (!c) return M2S_ERR_INVALID;
    if (!c->lod_work.blend_tag.holds(*c)) return fail(c, M2S_ERR_STATE, "no blend weights of the current records (m2s_lod_blend; the records changed since)");
    if (out_n) *out_n = c->lod_work.blend_tag.n;
    if (!dst) return capacity ? fail(c, M2S_ERR_INVALID, "no destination") : M2S_OK;
    if (capacity < c->lod_work.blend_tag.n) return fail(c, M2S_ERR_CAPACITY, "destination holds fewer entries than there are records");
    if (!c->lod_work.blend_tag.n) return M2S_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->lod_work.blend_t, c->lod_work.blend_tag.n * sizeof(float), hipMemcpyDeviceToHost));
    return M2S_OK;
}

m2s_status m2s_last_lod_blend_counts(const m2s_ctx* c, uint64_t out[4]) { return get_array(c, &m2s_ctx::last_lod_blend_counts, out); }

float m2s_last_lod_blend_ms(const m2s_ctx* c) { return c ? c->last_lod_blend_ms : 0.0f; }

m2s_status m2s_last_lod_blend_stage_ms(const m2s_ctx* c, float out_ms[3]) { return get_array(c, &m2s_ctx::last_lod_blend_stage_ms, out_ms); }

m2s_status m2s_lod_build(m2s_ctx* c, const m2s_lod_build_params* p, uint64_t out_counts[4]) {
    if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
    if (!c || !p) return M2S_ERR_INVALID;
    if (p->n_steps < 1 || p->n_steps > M2S_LOD_MAX_STEPS) return fail(c, M2S_ERR_INVALID, "n_steps outside 1..16");
    for (uint32_t s = 0; s < M2S_LOD_MAX_STEPS; ++s) {
        if (s >= p->n_steps ? p->levels[s] != 0 : p->levels[s] > 10) return fail(c, M2S_ERR_INVALID, "a level above 10, or a level past n_steps that is not 0");
        if (s && s < p->n_steps && p->levels[s] < p->levels[s - 1]) return fail(c, M2S_ERR_INVALID, "the levels decrease");
    }
    if (p->max_group < 2 || p->max_group > 64) return fail(c, M2S_ERR_INVALID, "max_group outside 2..64");
    if (std::isnan(p->min_axis_dot)) return fail(c, M2S_ERR_INVALID, "min_axis_dot is NaN");
    if (p->flags & ~(uint32_t)M2S_MERGE_UNSIGNED_AXIS) return fail(c, M2S_ERR_INVALID, "flags other than M2S_MERGE_UNSIGNED_AXIS");
    M2S_TRY(have_records(c));
    const uint64_t n0 = c->last_stored;
    if (n0 >= kLodMaxNodes) return fail(c, M2S_ERR_CAPACITY, "2^32-1 nodes or more");
    const uint32_t R = c->last_R;
    const bool unsigned_axis = (p->flags & M2S_MERGE_UNSIGNED_AXIS) != 0;   // (every step, the ones that merge nothing included)
    const bool with_sh = c->carry_sh && c->sh_tag.holds(*c, n0);            // pin 4s: the tree owns a plane too
    const uint32_t sh_degree = c->sh_degree;
    const bool gauss = c->merge_model == M2S_MERGE_MODEL_GAUSSIAN;          // pin 4g: every step merges under it (merge_run) and the bounds follow
    const float sigma = c->merge_sigma;
    HIPCHK(c, hipSetDevice(c->device));
    M2S_TRY(c->lod_build_clock.begin(c->err, true));                    // (measured whatever m2s_set_profiling says)
    LodTree& t = c->lod;
    t.end();                                                            // (the tree of an earlier call ends here, whatever follows)
    if (!with_sh) t.drop_sh();
    HIPCHK(c, c->lod_build_clock.mark(SpanMark::Begin, c->stream));
    M2S_TRY(t.reserve(c->err, c->stream, n0 + n0 / 2, 0, with_sh));
    uint64_t first[M2S_LOD_MAX_STEPS + 2] = {};
    uint32_t levels = 1;
    uint64_t skipped = 0;
    first[1] = n0;
    if (n0) {
        HIPCHK(c, hipMemcpyAsync(t.rows<float4>(kLodRecords), c->last_records, n0 * t.row_bytes(kLodRecords), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, lod_link(nullptr, 0, 0, nullptr, t.rows<float4>(kLodRecords), (uint32_t)n0, t.rows<float4>(kLodBounds), gauss, sigma, c->stream));
        if (with_sh) HIPCHK(c, hipMemcpyAsync(t.rows<float>(kLodSh), c->d_sh, n0 * t.row_bytes(kLodSh), hipMemcpyDeviceToDevice, c->stream));
    }
    for (uint32_t s = 0; s < p->n_steps; ++s) {
        const uint64_t below = first[levels - 1], cnt = first[levels] - below;
        M2S_TRY(merge_run(c, p->levels[s], p->max_group, p->min_axis_dot, MergeMode::IfAny, unsigned_axis));
        const uint64_t after = c->last_merge_counts[1];
        if (after == cnt) { ++skipped; continue; }                      // (nothing merged and nothing changed: no level)
        const uint64_t total = first[levels] + after;
        if (total >= kLodMaxNodes) return fail(c, M2S_ERR_CAPACITY, "2^32-1 nodes or more");
        M2S_TRY(t.reserve(c->err, c->stream, total, first[levels], with_sh));
        float4* const level = t.rows<float4>(kLodRecords, first[levels]);
        HIPCHK(c, hipMemcpyAsync(level, c->last_records, after * t.row_bytes(kLodRecords), hipMemcpyDeviceToDevice, c->stream));
        if (with_sh) {                                                  // (the rows pin 5s made for this step: the context's plane by now)
            if (!c->sh_tag.holds(*c, after)) return fail(c, M2S_ERR_HIP, "the merge left no plane of its parents (internal error)");
            HIPCHK(c, hipMemcpyAsync(t.rows<float>(kLodSh, first[levels]), c->d_sh, after * t.row_bytes(kLodSh), hipMemcpyDeviceToDevice, c->stream));
        }
        HIPCHK(c, lod_link(c->d_merge_map, (uint32_t)cnt, (uint32_t)first[levels], t.rows<uint32_t>(kLodParent, below), level, (uint32_t)after,
                           t.rows<float4>(kLodBounds, first[levels]), gauss, sigma, c->stream));
        first[++levels] = total;                                        // (the next step rewrites the map and the pool behind these, stream-ordered)
    }
    HIPCHK(c, lod_link(nullptr, (uint32_t)(first[levels] - first[levels - 1]), 0, t.rows<uint32_t>(kLodParent, first[levels - 1]), nullptr, 0, nullptr, gauss, sigma, c->stream));
    HIPCHK(c, c->lod_build_clock.mark(SpanMark::End, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->lod_build_clock.span(SpanMark::Begin, SpanMark::End, &c->last_lod_build_ms));
    t.commit(levels, first, R, with_sh, sh_degree, gauss ? M2S_MERGE_MODEL_GAUSSIAN : M2S_MERGE_MODEL_FOOTPRINT, sigma);
    if (out_counts) { out_counts[0] = n0; out_counts[1] = first[levels]; out_counts[2] = levels; out_counts[3] = skipped; }
    return M2S_OK;
}

m2s_status m2s_lod_levels(const m2s_ctx* c, uint32_t* out_levels, uint64_t first[M2S_LOD_MAX_STEPS + 2]) {
    if (out_levels) *out_levels = 0;
    if (!c) return M2S_ERR_INVALID;
    if (!c->lod.levels) return M2S_ERR_STATE;
    if (out_levels) *out_levels = c->lod.levels;
    if (first) std::memcpy(first, c->lod.first, sizeof(c->lod.first));
    return M2S_OK;
}

const void* m2s_device_lod(const m2s_ctx* c, uint32_t which) { return c && which <= kLodBounds ? c->lod.plane(which) : nullptr; }

m2s_status m2s_download_lod(m2s_ctx* c, uint32_t which, void* dst, uint64_t capacity_bytes) {
    if (!c) return M2S_ERR_INVALID;
    if (which > 2) return fail(c, M2S_ERR_INVALID, "which outside 0..2");
    if (!c->lod.levels) return fail(c, M2S_ERR_STATE, kNoTreeMsg);
    const uint64_t bytes = c->lod.nodes() * c->lod.row_bytes(which);
    if (capacity_bytes < bytes) return fail(c, M2S_ERR_CAPACITY, "destination holds fewer bytes than the plane");
    if (!bytes) return M2S_OK;
    if (!dst) return fail(c, M2S_ERR_INVALID, "no destination");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->lod.plane(which), bytes, hipMemcpyDeviceToHost));
    return M2S_OK;
}

const void* m2s_device_lod_sh(const m2s_ctx* c) { return c ? c->lod.plane(kLodSh) : nullptr; }

m2s_status m2s_download_lod_sh(m2s_ctx* c, float* dst, uint64_t capacity_rows, uint32_t* out_degree) {
    if (out_degree) *out_degree = 0;
    if (!c) return M2S_ERR_INVALID;
    if (!c->lod.levels) return fail(c, M2S_ERR_STATE, kNoTreeMsg);
    if (!c->lod.has_sh) return fail(c, M2S_ERR_STATE, "the tree has no SH plane (m2s_set_carry_sh and a baked plane at m2s_lod_build)");
    const uint64_t rows = c->lod.nodes();
    if (capacity_rows < rows) return fail(c, M2S_ERR_CAPACITY, "destination holds fewer rows than the plane");
    if (out_degree) *out_degree = c->lod.sh_degree;
    if (!rows) return M2S_OK;
    if (!dst) return fail(c, M2S_ERR_INVALID, "no destination");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->lod.plane(kLodSh), rows * c->lod.row_bytes(kLodSh), hipMemcpyDeviceToHost));
    return M2S_OK;
}

m2s_status m2s_lod_release(m2s_ctx* c) {
    if (!c) return M2S_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->lod.release();
    c->lod_work.release_tree_sized();
    return M2S_OK;
}

float m2s_last_lod_build_ms(const m2s_ctx* c) { return c ? c->last_lod_build_ms : 0.0f; }

m2s_status m2s_lod_select(m2s_ctx* c, const m2s_lod_select_params* p, uint64_t out_counts[4]) {
    if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
    if (!c || !p) return M2S_ERR_INVALID;
    M2S_TRY(lod_select_check(c, p));
    M2S_TRY(lod_ready(c));
    return lod_cut(c, p, out_counts, nullptr, LodVis::None);
}

m2s_status m2s_lod_select_frustum(m2s_ctx* c, const m2s_lod_select_params* p, const m2s_lod_frustum* fr, uint64_t out_counts[4]) {
    if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
    if (!c || !p) return M2S_ERR_INVALID;
    M2S_TRY(lod_select_check(c, p));
    M2S_TRY(lod_frustum_check(c, fr));
    M2S_TRY(lod_ready(c));
    return lod_cut(c, p, out_counts, fr, LodVis::Here);
}

m2s_status m2s_lod_select_budget(m2s_ctx* c, const m2s_lod_budget_params* p, m2s_lod_budget_result* out, uint64_t out_counts[4]) {
    if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
    if (out) std::memset(out, 0, sizeof(*out));
    if (!c || !p) return M2S_ERR_INVALID;
    M2S_TRY(lod_budget_check(c, p));
    M2S_TRY(lod_ready(c));
    return lod_budget(c, p, nullptr, out, out_counts);
}

m2s_status m2s_lod_select_budget_frustum(m2s_ctx* c, const m2s_lod_budget_params* p, const m2s_lod_frustum* fr, m2s_lod_budget_result* out,
                                         uint64_t out_counts[4]) {
    if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
    if (out) std::memset(out, 0, sizeof(*out));
    if (!c || !p) return M2S_ERR_INVALID;
    M2S_TRY(lod_budget_check(c, p));
    M2S_TRY(lod_frustum_check(c, fr));
    M2S_TRY(lod_ready(c));
    return lod_budget(c, p, fr, out, out_counts);
}

m2s_status m2s_lod_select_occluded(m2s_ctx* c, const m2s_lod_select_params* p, const m2s_lod_frustum* fr, const m2s_lod_occluder* oc,
                                   uint64_t out_counts[4]) {
    if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
    if (!c || !p) return M2S_ERR_INVALID;
    M2S_TRY(lod_select_check(c, p));
    M2S_TRY(lod_frustum_check(c, fr));
    M2S_TRY(lod_occluder_check(c, oc));
    M2S_TRY(lod_ready(c));
    M2S_TRY(lod_occluder_state(c, oc));
    return lod_cut(c, p, out_counts, fr, LodVis::Here, oc);
}

m2s_status m2s_lod_select_budget_occluded(m2s_ctx* c, const m2s_lod_budget_params* p, const m2s_lod_frustum* fr, const m2s_lod_occluder* oc,
                                          m2s_lod_budget_result* out, uint64_t out_counts[4]) {
    if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
    if (out) std::memset(out, 0, sizeof(*out));
    if (!c || !p) return M2S_ERR_INVALID;
    M2S_TRY(lod_budget_check(c, p));
    M2S_TRY(lod_frustum_check(c, fr));
    M2S_TRY(lod_occluder_check(c, oc));
    M2S_TRY(lod_ready(c));
    M2S_TRY(lod_occluder_state(c, oc));
    return lod_budget(c, p, fr, out, out_counts, oc);
}

m2s_status m2s_last_lod_occlusion_counts(const m2s_ctx* c, uint64_t out[4]) { return get_array(c, &m2s_ctx::last_lod_occlusion_counts, out); }

m2s_status m2s_last_lod_frustum_counts(const m2s_ctx* c, uint64_t out[2]) { return get_array(c, &m2s_ctx::last_lod_frustum_counts, out); }

float m2s_last_lod_frustum_ms(const m2s_ctx* c) { return c ? c->last_lod_frustum_ms : 0.0f; }

m2s_status m2s_last_lod_budget_stage_ms(const m2s_ctx* c, float out_ms[3]) { return get_array(c, &m2s_ctx::last_lod_budget_stage_ms, out_ms); }

m2s_status m2s_last_lod_level_counts(const m2s_ctx* c, uint64_t out[M2S_LOD_MAX_STEPS + 1]) { return get_array(c, &m2s_ctx::last_lod_level_counts, out); }

m2s_status m2s_last_lod_select_stage_ms(const m2s_ctx* c, float out_ms[3]) { return get_array(c, &m2s_ctx::last_lod_select_stage_ms, out_ms); }

const void* m2s_device_lod_nodes(const m2s_ctx* c) { return c && lod_ids_valid(c) && c->lod_ids_tag.n ? c->lod_work.ids.get() : nullptr; }

m2s_status m2s_download_lod_nodes(m2s_ctx* c, uint32_t* dst, uint64_t capacity, uint64_t* out_n) {
    if (out_n) *out_n = 0;
    if (!c) return M2S_ERR_INVALID;
    if (!lod_ids_valid(c)) return fail(c, M2S_ERR_STATE, "no node indices of the current records (m2s_lod_select; the records changed since)");
    if (out_n) *out_n = c->lod_ids_tag.n;
    if (!dst) return capacity ? fail(c, M2S_ERR_INVALID, "no destination") : M2S_OK;
    if (capacity < c->lod_ids_tag.n) return fail(c, M2S_ERR_CAPACITY, "destination holds fewer entries than there are records");
    if (!c->lod_ids_tag.n) return M2S_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->lod_work.ids, c->lod_ids_tag.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return M2S_OK;
}

}  // extern "C"
