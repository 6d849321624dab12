// m2s_viewer.cpp — the two viewer passes that consume the records: depth sort (RadixSortPass.cpp:8-90) and prepass
// (GaussiansPrepass.cpp:8-56).
#include "m2s_ctx.h"
#include "m2s_ply.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

using namespace m2s;
using namespace m2s_host;

namespace {

// Room for a depth sort of n entries: the keys / permutation words, the radix sort's work area of `temp_bytes` and, with_plane, the
// position plane (without it every sort reads the records: slower, not wrong).
m2s_status reserve_sort(m2s_ctx* c, uint64_t n, size_t temp_bytes, bool with_plane) {
    M2S_TRY(c->d_sort_u32.reserve(c->err, n, 4 * sizeof(uint32_t)));
    M2S_TRY(c->d_sort_temp.reserve(c->err, temp_bytes, 1));
    if (with_plane && c->d_pos_plane.cap() < n) {
        c->pos_plane_tag.clear();
        (void)c->d_pos_plane.try_reserve(n, 16);
    }
    return M2S_OK;
}

}  // namespace

extern "C" {

// RadixSortPass::execute (RadixSortPass.cpp:8-90) on the records of the last conversion.
m2s_status m2s_sort_by_depth(m2s_ctx* c, const float world_to_view[16], uint64_t* out_n) {
    if (!c || !world_to_view) return M2S_ERR_INVALID;
    if (!c->last_records) return fail(c, M2S_ERR_STATE, "no conversion has run and no records were uploaded");
    if (c->records_stale) return fail(c, M2S_ERR_STATE, kStaleMsg);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n = c->last_stored;
    c->sorted_n = 0;
    if (c->sq_src != c->d_sq_src.get()) c->sq_src = nullptr;   // (sources aliasing the permutation words this sort is about to rewrite)
    if (out_n) *out_n = n;
    if (!n) return M2S_OK;
    if (n > 0xFFFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^32-1 records");
    M2S_TRY(c->d_sorted.reserve(c->err, n, sizeof(m2s_gaussian)));
    M2S_TRY(reserve_sort(c, n, sort_temp_bytes((uint32_t)n), true));
    const bool plane_valid = positions_valid(c, n);
    ClockOf<SortMark>& clock = c->sort_clock;
    M2S_TRY(clock.begin(c->err, c->profiling));
    uint32_t* u = c->d_sort_u32;     // keys_in | (unused) | keys_out | vals_out
    HIPCHK(c, sort_by_depth((const float4*)c->last_records, (uint32_t)n, world_to_view, u, u + 2 * n, u + 3 * n, c->d_sort_temp,
                            c->d_sort_temp.cap(), c->d_sorted, c->d_pos_plane, plane_valid, clock.marks(), c->stream,
                            &c->sorted_key_offset, reinterpret_cast<uint32_t*>(&c->h_total[m2s_ctx::kPinnedSortMM])));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->d_pos_plane) c->pos_plane_tag.set(*c, n);
    if (clock.on()) {
        for (int k = 0; k < 3; ++k) HIPCHK(c, clock.span(k, k + 1, &c->last_sort_stage_ms[k]));
        HIPCHK(c, clock.span(SortMark::Start, SortMark::Gathered, &c->last_sort_ms));
    }
    c->sorted_n = n;
    return M2S_OK;
}

const void* m2s_device_sorted_records(const m2s_ctx* c) { return c && c->sorted_n ? c->d_sorted.get() : nullptr; }
// the keys of those records (uint32, ascending): keys_out of the radix sort
// (the sort runs over the bits in which the keys differ, on `key - smallest key`: the smallest key is added back here, once, when
//  somebody asks for the keys — the distributed sort does; a frame's sort + gather does not)
const void* m2s_device_sorted_keys(const m2s_ctx* cc) {
    m2s_ctx* c = const_cast<m2s_ctx*>(cc);
    if (!c || !c->sorted_n) return nullptr;
    uint32_t* keys = c->d_sort_u32 + 2 * c->sorted_n;
    if (c->sorted_key_offset) {
        if (hipSetDevice(c->device) != hipSuccess) return nullptr;
        launch_add_to_keys(keys, (uint32_t)c->sorted_n, c->sorted_key_offset, c->stream);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return nullptr;
        c->sorted_key_offset = 0;
    }
    return keys;
}
uint64_t m2s_num_sorted(const m2s_ctx* c) { return c ? c->sorted_n : 0; }
uint32_t m2s_last_resolution(const m2s_ctx* c) { return c ? c->last_R : 0; }

m2s_status m2s_download_sorted(m2s_ctx* c, m2s_gaussian* dst, uint64_t capacity_records) {
    if (!c) return M2S_ERR_INVALID;
    if (!c->sorted_n) return M2S_OK;
    if (!dst) return fail(c, M2S_ERR_INVALID, "dst is NULL");
    if (capacity_records < c->sorted_n) return fail(c, M2S_ERR_CAPACITY, "dst holds fewer records than were sorted");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_sorted, c->sorted_n * sizeof(m2s_gaussian), hipMemcpyDeviceToHost));
    return M2S_OK;
}

float m2s_last_sort_ms(const m2s_ctx* c) { return c ? c->last_sort_ms : 0.0f; }
m2s_status m2s_last_sort_stage_ms(const m2s_ctx* c, float out_ms[3]) { return get_array(c, &m2s_ctx::last_sort_stage_ms, out_ms); }

// GaussiansPrepass::execute (GaussiansPrepass.cpp:8-56) + the counter read-back that follows it (RadixSortPass.cpp:18-22).
// sorted = m2s_prepass_sorted: the depth sort of RadixSortPass::execute taken FIRST, as a permutation of the records by the depth bits this
// prepass stores; the prepass then reads the records through it and appends its survivors in that order, straight into the sorted-quads buffer.
static m2s_status prepass_impl(m2s_ctx* c, const m2s_prepass_params* p, const void* d_records, uint64_t n, uint64_t* out_visible, bool sorted) {
    if (!c || !p) return M2S_ERR_INVALID;
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    if (!d_records) M2S_TRY(pick_records(c, d_records, n));
    if (p->resolution_target == 0) return fail(c, M2S_ERR_INVALID, "resolution_target is 0");
    if (p->depth_test_mesh == 1 && p->format == 0 && (!p->depth || !p->depth_w || !p->depth_h))
        return fail(c, M2S_ERR_INVALID, "depth_test_mesh is set but no depth image was passed");
    if (n > 0xFFFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^32-1 records");
    HIPCHK(c, hipSetDevice(c->device));
    c->pp_visible = 0;
    c->sq_n = 0;
    c->sq_src = nullptr;
    if (out_visible) *out_visible = 0;
    if (!n) return M2S_OK;
    if (!sorted) M2S_TRY(c->d_quads.reserve(c->err, n, sizeof(m2s_quad)));
    M2S_TRY(c->d_pp_depths.reserve(c->err, n, sizeof(float)));
    const uint32_t* perm = nullptr;
    // the plain prepass has a clock of its own; the sorted one chains its two marks behind the sort's
    M2S_TRY(sorted ? c->sort_clock.begin(c->err, c->profiling) : c->prepass_clock.begin(c->err, c->profiling));
    const StageMarks sort_marks = sorted ? c->sort_clock.marks() : StageMarks();
    const StageMarks pp_marks = sorted ? c->sort_clock.marks(SortMark::Gathered) : c->prepass_clock.marks();
    if (sorted) {   // room for the sorted survivors, the keys / permutation, the radix sort's work area and the position plane
        M2S_TRY(c->d_sorted_quads.reserve(c->err, n, sizeof(m2s_quad)));
        M2S_TRY(reserve_sort(c, n, sort_temp_bytes((uint32_t)n), true));
        c->sorted_n = 0;          // (the key / permutation words are shared with m2s_sort_by_depth: its sorted keys are gone)
    }
    const uint64_t words = (n + 63) / 64 + 1;          // [0] = the arrival-order counter, [1..] = the look-back chain
    // the chain is tagged with the low 16 bits of a launch counter instead of being cleared per launch; cleared when
    // it is (re)allocated and when the tag wraps (see next_epoch)
    bool clear_chain = false;
    M2S_TRY(c->d_pp_chain.reserve(c->err, words, sizeof(unsigned long long), &clear_chain));
    uint32_t epoch = ++c->pp_epoch;
    if (clear_chain || (epoch & 0xFFFFu) == 0)
        HIPCHK(c, hipMemsetAsync(c->d_pp_chain, 0, c->d_pp_chain.cap() * sizeof(unsigned long long), c->stream));
    PrepassK k;
    prepass_prepare(*p, n, &k);
    if (sorted) k.arrival_order = 0;            // the order of the survivors IS the result
    if (p->depth_test_mesh == 1 && p->format == 0) {
        if (p->depth_on_device) k.depth = p->depth;
        else {
            const uint64_t texels = (uint64_t)p->depth_w * p->depth_h;
            M2S_TRY(c->d_pp_depthtex.reserve(c->err, texels, sizeof(float)));
            HIPCHK(c, hipMemcpyAsync(c->d_pp_depthtex, p->depth, texels * sizeof(float), hipMemcpyHostToDevice, c->stream));
            k.depth = c->d_pp_depthtex;
        }
    } else k.depth_test = 0;
    unsigned long long* res = &c->h_total[m2s_ctx::kPinnedPrepass];
    res[0] = 0; res[1] = 0;
    if (k.arrival_order) HIPCHK(c, hipMemsetAsync(c->d_pp_chain, 0, sizeof(unsigned long long), c->stream));
    // Without a depth image the prepass's first test is the frustum test, a function of the position: the sort applies it to the keys
    // (view_project, the prepass's own function), the culled records sort behind the survivors, and the prepass runs over the survivors
    // alone — dense: no compaction, no look-back, no read of a record that is not drawn.  The shader's LAST test (lambda2 < 0, :183) depends
    // on scale and rotation and is not known to the sort: a record that passes the first and fails the last makes the dense launch report a
    // disagreement, and the frame is then repeated as in the `clash` case below — everything sorted, the prepass compacting.
    bool dense = false;
    uint32_t n_run = (uint32_t)n;
    if (sorted) {
        const bool plane_valid = positions_valid(c, n);
        uint32_t* u = c->d_sort_u32;     // keys_in | (unused) | keys_out | vals_out = the permutation
        uint32_t* pinned4 = reinterpret_cast<uint32_t*>(&c->h_total[m2s_ctx::kPinnedSortMM]);
        bool cull = k.depth_test == 0u, clash = false;
        HIPCHK(c, sort_prepass_permutation((const float4*)d_records, (uint32_t)n, k.M, k.V, k.P, cull, u, u + 2 * n, u + 3 * n, c->d_sort_temp, c->d_sort_temp.cap(),
                                           c->d_pos_plane, plane_valid, sort_marks, c->stream, pinned4, &n_run, &clash));
        if (c->d_pos_plane) c->pos_plane_tag.set(*c, n);
        if (cull && clash) {   // a survivor whose depth bits ARE the marker of the culled ones (a NaN with that payload): sort everything, compact in the prepass
            cull = false;
            HIPCHK(c, sort_prepass_permutation((const float4*)d_records, (uint32_t)n, k.M, k.V, k.P, false, u, u + 2 * n, u + 3 * n, c->d_sort_temp, c->d_sort_temp.cap(),
                                               c->d_pos_plane, true, sort_marks, c->stream, pinned4, &n_run, &clash));
        }
        dense = cull;
        perm = u + 3 * n;
        // which record every surviving quad was made from: dense, position i holds record perm[i] and every position survives — the
        // first n_run words of the permutation ARE the sources; compacting, the kernel stores them beside the quads
        if (!dense && n_run) M2S_TRY(c->d_sq_src.reserve(c->err, n, sizeof(uint32_t)));
    }
    uint32_t* src_out = sorted && !dense ? c->d_sq_src.get() : nullptr;
    const uint32_t* status = reinterpret_cast<const uint32_t*>(&res[1]);
    for (;;) {
        HIPCHK(c, pp_marks.mark(0, c->stream));
        if (n_run) HIPCHK(c, launch_prepass(k, (const float4*)d_records, n_run, sorted ? c->d_sorted_quads.get() : c->d_quads.get(), c->d_pp_depths, c->d_pp_chain + 1,
                                            epoch, c->d_pp_chain, &res[0], reinterpret_cast<uint32_t*>(&res[1]), c->stream, perm, dense, src_out));
        HIPCHK(c, pp_marks.mark(1, c->stream));
        if (k.arrival_order) HIPCHK(c, hipMemcpyAsync(&res[0], c->d_pp_chain, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!(dense && status[1] == 2u)) break;
        // A survivor of the sort's frustum test fails the prepass's last test (lambda2 < 0: a needle whose screen-space covariance is
        // numerically of rank 1).  The dense launch wrote a quad for it; the frame is taken again the way a depth image takes it: every
        // record sorted, the prepass compacting through the permutation and storing the sources beside the quads.  The positions are in
        // the plane by now (where there is one), the chain gets an epoch of its own under the rule above, and the stage times read
        // below are those of this second attempt.
        uint32_t* u = c->d_sort_u32;
        bool clash = false;
        res[0] = 0; res[1] = 0;
        HIPCHK(c, sort_prepass_permutation((const float4*)d_records, (uint32_t)n, k.M, k.V, k.P, false, u, u + 2 * n, u + 3 * n, c->d_sort_temp, c->d_sort_temp.cap(),
                                           c->d_pos_plane, true, sort_marks, c->stream, reinterpret_cast<uint32_t*>(&c->h_total[m2s_ctx::kPinnedSortMM]), &n_run,
                                           &clash));
        M2S_TRY(c->d_sq_src.reserve(c->err, n, sizeof(uint32_t)));
        epoch = ++c->pp_epoch;
        if ((epoch & 0xFFFFu) == 0) HIPCHK(c, hipMemsetAsync(c->d_pp_chain, 0, c->d_pp_chain.cap() * sizeof(unsigned long long), c->stream));
        dense = false;
        src_out = c->d_sq_src.get();
    }
    // (only the clock this call opened is read: the other one holds an earlier call's marks)
    if (sorted) {
        const ClockOf<SortMark>& clock = c->sort_clock;
        if (clock.on()) {
            HIPCHK(c, clock.span(SortMark::Gathered, SortMark::Prepassed, &c->last_prepass_ms));
            for (int j = 0; j < 2; ++j) HIPCHK(c, clock.span(j, j + 1, &c->last_sort_stage_ms[j]));
            c->last_sort_stage_ms[2] = c->last_prepass_ms;
            HIPCHK(c, clock.span(SortMark::Start, SortMark::Prepassed, &c->last_sort_ms));
        }
    } else if (c->prepass_clock.on()) {
        HIPCHK(c, c->prepass_clock.span(SpanMark::Begin, SpanMark::End, &c->last_prepass_ms));
    }
    if (status[1]) return fail(c, M2S_ERR_HIP, "prepass: look-back chain timed out");
    if (dense) res[0] = n_run;                  // (the survivors were counted by the sort; the dense prepass appends nothing)
    if (sorted) {
        c->sq_n = res[0];
        c->sq_src = dense ? perm : c->d_sq_src.get();
        c->sq_src_tag.set(*c, n);
    } else c->pp_visible = res[0];
    if (out_visible) *out_visible = res[0];
    return M2S_OK;
}

m2s_status m2s_prepass(m2s_ctx* c, const m2s_prepass_params* p, const void* d_records, uint64_t n, uint64_t* out_visible) {
    return prepass_impl(c, p, d_records, n, out_visible, false);
}

// GaussiansPrepass::execute + RadixSortPass::execute (GaussiansPrepass.cpp:8-56, RadixSortPass.cpp:8-90) of one frame as ONE pass over the
// records: == m2s_prepass (input order) followed by m2s_sort_prepass, byte for byte, in m2s_device_sorted_quads.
m2s_status m2s_prepass_sorted(m2s_ctx* c, const m2s_prepass_params* p, uint64_t* out_visible) {
    return prepass_impl(c, p, nullptr, 0, out_visible, true);
}

const void* m2s_device_quads(const m2s_ctx* c) { return c && c->pp_visible ? c->d_quads.get() : nullptr; }
const void* m2s_device_prepass_depths(const m2s_ctx* c) { return c && c->pp_visible ? c->d_pp_depths.get() : nullptr; }

m2s_status m2s_download_prepass(m2s_ctx* c, m2s_quad* dst_quads, float* dst_depths, uint64_t capacity) {
    if (!c) return M2S_ERR_INVALID;
    if (!c->pp_visible) return M2S_OK;
    if (capacity < c->pp_visible) return fail(c, M2S_ERR_CAPACITY, "destination holds fewer entries than survived the prepass");
    HIPCHK(c, hipSetDevice(c->device));
    if (dst_quads) HIPCHK(c, hipMemcpy(dst_quads, c->d_quads, c->pp_visible * sizeof(m2s_quad), hipMemcpyDeviceToHost));
    if (dst_depths) HIPCHK(c, hipMemcpy(dst_depths, c->d_pp_depths, c->pp_visible * sizeof(float), hipMemcpyDeviceToHost));
    return M2S_OK;
}

float m2s_last_prepass_ms(const m2s_ctx* c) { return c ? c->last_prepass_ms : 0.0f; }

// RadixSortPass::execute (RadixSortPass.cpp:8-90) on what the last m2s_prepass left behind.
m2s_status m2s_sort_prepass(m2s_ctx* c, uint64_t* out_n) {
    if (!c) return M2S_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n = c->pp_visible;          // the atomic counter the reference reads back (RadixSortPass.cpp:18-22)
    c->sq_n = 0;
    c->sq_src = nullptr;
    if (out_n) *out_n = n;
    if (!n) return M2S_OK;
    M2S_TRY(c->d_sorted_quads.reserve(c->err, n, sizeof(m2s_quad)));
    M2S_TRY(reserve_sort(c, n, sort_prepass_temp_bytes((uint32_t)n), false));
    uint32_t* u = c->d_sort_u32;
    ClockOf<SpanMark>& clock = c->sort_prepass_clock;
    M2S_TRY(clock.begin(c->err, c->profiling));
    HIPCHK(c, clock.mark(SpanMark::Begin, c->stream));
    HIPCHK(c, sort_prepass(c->d_pp_depths, c->d_quads, (uint32_t)n, u, u + n, c->d_sort_temp, c->d_sort_temp.cap(), c->d_sorted_quads, c->stream));
    HIPCHK(c, clock.mark(SpanMark::End, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (clock.on()) HIPCHK(c, clock.span(SpanMark::Begin, SpanMark::End, &c->last_sort_prepass_ms));
    c->sq_n = n;
    return M2S_OK;
}

const void* m2s_device_sorted_quads(const m2s_ctx* c) { return c && c->sq_n ? c->d_sorted_quads.get() : nullptr; }
const void* m2s_device_sorted_sources(const m2s_ctx* c) {
    return c && c->sq_n && c->sq_src_tag.holds(*c) ? c->sq_src : nullptr;
}

m2s_status m2s_download_sorted_sources(m2s_ctx* c, uint32_t* dst, uint64_t capacity) {
    if (!c) return M2S_ERR_INVALID;
    const void* src = m2s_device_sorted_sources(c);
    if (!src) return fail(c, M2S_ERR_STATE, "the sorted quads carry no sources (m2s_prepass_sorted, m2s_upload_quad_sources)");
    if (!dst) return fail(c, M2S_ERR_INVALID, "dst is NULL");
    if (capacity < c->sq_n) return fail(c, M2S_ERR_CAPACITY, "dst holds fewer entries than there are sorted quads");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, src, c->sq_n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return M2S_OK;
}

m2s_status m2s_download_sorted_quads(m2s_ctx* c, m2s_quad* dst, uint64_t capacity) {
    if (!c) return M2S_ERR_INVALID;
    if (!c->sq_n) return M2S_OK;
    if (!dst) return fail(c, M2S_ERR_INVALID, "dst is NULL");
    if (capacity < c->sq_n) return fail(c, M2S_ERR_CAPACITY, "dst holds fewer quads than were sorted");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_sorted_quads, c->sq_n * sizeof(m2s_quad), hipMemcpyDeviceToHost));
    return M2S_OK;
}

float m2s_last_sort_prepass_ms(const m2s_ctx* c) { return c ? c->last_sort_prepass_ms : 0.0f; }

}  // extern "C"
