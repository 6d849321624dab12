// m2s_merge.cpp — the merge pass (m2s_merge): host side of m2s_merge.hip.  Order comes from the compact export's helper
// (compact_keys_and_sort, m2s_compact.hip) in the compact export's own buffers; the parents go into the pool the way m2s_prune's survivors
// do (through the staging buffer where the sources live there); what the call does to the context: m2s_recstate.h, Rewrite::Merge —
// MergeWithSh where m2s_set_carry_sh is on and a baked plane of the records exists: k_merge_reduce_sh then reduces the plane too (pin 5s).
// The record model (m2s_set_merge_model, m2s_context.cpp) picks the kernels' instances here: nothing else of the pass knows about it.
// merge_run is the pass behind m2s_merge's argument checks: the steps of m2s_lod_build (m2s_lod.cpp) are calls of it.
#include "m2s_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace m2s;
using namespace m2s_host;

namespace {

bool merge_map_valid(const m2s_ctx* c) { return c->merge_map_tag.holds(*c); }

}  // namespace

namespace m2s_host {

// The body of m2s_merge behind its argument checks (m2s_lod_build runs it once per step): level 0..10, max_group 2..64, no NaN.
// unsigned_axis (M2S_MERGE_UNSIGNED_AXIS) goes to both launches: the heads (pin 2u) and the reduction (pin 5u).
m2s_status merge_run(m2s_ctx* c, uint32_t level, uint32_t max_group, float min_axis_dot, MergeMode mode, bool unsigned_axis) {
    uint64_t n64 = 0;
    M2S_TRY(need_records(c, &n64));
    const uint32_t n = (uint32_t)n64;
    bool dry = mode == MergeMode::Dry || (mode == MergeMode::IfAny && n == 0);
    const uint32_t R = c->last_R;
    HIPCHK(c, hipSetDevice(c->device));
    ClockOf<MergeMark>& clock = c->merge_clock;
    M2S_TRY(clock.begin(c->err, true));            // (measured whatever m2s_set_profiling says)
    // pin 5s: a plane of exactly these n records is reduced with them (decided here: the tag does not survive what follows)
    const bool with_sh = c->carry_sh && c->sh_tag.holds(*c, n);
    // m2s_set_merge_model: pins 2g, 5g, 5sg take the place of 2 / 2u, 5 / 5u, 5s (unsigned_axis then changes nothing)
    const bool gauss = c->merge_model == M2S_MERGE_MODEL_GAUSSIAN;
    M2S_TRY(c->merge_sh_clock.begin(c->err, with_sh));
    c->last_merge_sh_ms = 0.0f;
    uint64_t segments = 0, merged = 0, invalid = 0;
    float ms[3] = { 0, 0, 0 };
    if (n) {
        const uint32_t n_waves = compact_waves(n);
        M2S_TRY(c->d_compact_u32.reserve(c->err, n, 4 * sizeof(uint32_t)));
        M2S_TRY(c->d_compact_waves.reserve(c->err, (uint64_t)n_waves + 1, 8 * sizeof(uint32_t)));
        const size_t temp_bytes = std::max(compact_sort_temp_bytes(n), merge_scan_temp_bytes(n));
        M2S_TRY(c->d_compact_temp.reserve(c->err, temp_bytes, 1));
        M2S_TRY(c->d_merge_u32.reserve(c->err, (uint64_t)n + 1, 7 * sizeof(uint32_t)));
        M2S_TRY(c->d_merge_totals.reserve(c->err, kMergeTotalsWords, sizeof(uint32_t)));
        const uint64_t cap = c->d_compact_u32.cap(), mcap = c->d_merge_u32.cap();
        uint32_t* const u = c->d_compact_u32.get();
        uint32_t* const m = c->d_merge_u32.get();
        uint32_t* const head = c->d_compact_waves.get() + (size_t)n_waves * 8;
        const uint32_t *keys = u + 2 * cap, *perm = u + 3 * cap;
        unsigned long long* const packed = reinterpret_cast<unsigned long long*>(m + 2 * mcap);   // (8 mcap bytes in: aligned)
        unsigned long long* const sums = reinterpret_cast<unsigned long long*>(m + 4 * mcap);
        uint32_t* const seg_start = m + 6 * mcap;
        const float4* plane = m2s_positions_ready(c) ? c->d_pos_plane.get() : nullptr;
        HIPCHK(c, compact_keys_and_sort((const float4*)c->last_records, plane, n, c->d_compact_waves, head, u, u + cap, u + 2 * cap, u + 3 * cap, c->d_compact_temp,
                                        c->d_compact_temp.cap(), clock.marks(), c->stream));
        HIPCHK(c, clock.mark(MergeMark::Segments, c->stream));
        HIPCHK(c, merge_segments((const float4*)c->last_records, keys, perm, n, level, max_group, min_axis_dot, m, m + mcap, packed, sums, seg_start,
                                 c->d_merge_totals, c->d_compact_temp, c->d_compact_temp.cap(), unsigned_axis, gauss, c->stream));
        HIPCHK(c, clock.mark(MergeMark::Segmented, c->stream));
        uint32_t h[kMergeTotalsWords] = {}, skipped = 0;
        HIPCHK(c, hipMemcpyAsync(h, c->d_merge_totals, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&skipped, head + 7, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        segments = h[0];
        invalid = skipped;
        merged = h[1];
        if (segments < 1 || segments > n || invalid > n || merged > segments) return fail(c, M2S_ERR_HIP, "the merge pass's segment count came back inconsistent");
        if (mode == MergeMode::IfAny && segments == n) dry = true;   // (nothing to merge: nothing changes)
        if (!dry) {
            // The parents go into the pool.  Members that live there already cannot be reduced onto themselves by independent lanes: the
            // parents go through the staging buffer and are copied back, stream-ordered (as m2s_prune's survivors).
            const bool in_pool = c->last_records == c->lane[0].records;
            c->merge_map_tag.clear();
            M2S_TRY(c->d_merge_map.reserve(c->err, n, sizeof(uint32_t)));
            if (in_pool) M2S_TRY(c->d_prune_stage.reserve(c->err, segments * sizeof(m2s_gaussian), 1));
            const void* src = c->last_records;
            if (!in_pool) M2S_TRY(ensure_records(c, segments));
            if (with_sh) M2S_TRY(c->d_sh_alt.reserve(c->err, segments, kMergeShLanes * sizeof(float4)));
            float4* dst = in_pool ? c->d_prune_stage.get() : (float4*)c->lane[0].records.get();
            if (gauss) HIPCHK(c, merge_reduce_gauss((const float4*)src, perm, seg_start, c->d_merge_totals, (uint32_t)segments, c->merge_sigma, dst, c->d_merge_map, c->stream));
            else HIPCHK(c, merge_reduce((const float4*)src, perm, seg_start, c->d_merge_totals, (uint32_t)segments, dst, c->d_merge_map, unsigned_axis, c->stream));
            if (with_sh) {
                // Pin 5s.  The members' rows come from d_sh through perm and the parents' rows go into the second buffer, which trades
                // places with d_sh below: no lane lands on a row another still reads, and nothing is copied back.  The weights are the
                // MEMBERS' alpha and scales: in front of the copy that puts the parents where the members were.
                HIPCHK(c, c->merge_sh_clock.mark(SpanMark::Begin, c->stream));
                HIPCHK(c, merge_reduce_sh((const float4*)src, (const float4*)c->d_sh.get(), perm, seg_start, c->d_merge_totals, (uint32_t)segments,
                                          (float4*)c->d_sh_alt.get(), gauss, c->stream));
                HIPCHK(c, c->merge_sh_clock.mark(SpanMark::End, c->stream));
            }
            if (in_pool) HIPCHK(c, hipMemcpyAsync(c->lane[0].records, c->d_prune_stage, segments * sizeof(m2s_gaussian), hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, clock.mark(MergeMark::Reduced, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (with_sh) c->d_sh.swap(c->d_sh_alt);
        }
    } else if (!dry) {
        M2S_TRY(prune_compact_enqueue(c, 0, 0, nullptr, nullptr, false));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->merge_map_tag.clear();
    }
    if (!dry) {
        // (without pin 5s a plane of the members is not a plane of their parents: dropped; with it, no records: an empty plane stays one)
        c->rewritten(c->lane[0].records, segments, R, with_sh ? Rewrite::MergeWithSh : Rewrite::Merge);
        c->merge_map_tag.set(*c, n);
    }
    HIPCHK(c, c->merge_sh_clock.span(SpanMark::Begin, SpanMark::End, &c->last_merge_sh_ms));   // (0 where the reduction did not run)
    // (no records: three zeros; a dry run records no Reduced: [2] is 0)
    HIPCHK(c, clock.span(MergeMark::Start, MergeMark::Sorted, &ms[0]));
    HIPCHK(c, clock.span(MergeMark::Segments, MergeMark::Segmented, &ms[1]));
    HIPCHK(c, clock.span(MergeMark::Segmented, MergeMark::Reduced, &ms[2]));
    c->last_merge_counts[0] = n; c->last_merge_counts[1] = segments; c->last_merge_counts[2] = merged; c->last_merge_counts[3] = invalid;
    std::memcpy(c->last_merge_stage_ms, ms, sizeof(ms));
    return M2S_OK;
}

}  // namespace m2s_host

extern "C" {

m2s_status m2s_merge(m2s_ctx* c, const m2s_merge_params* p, uint64_t out_counts[4]) {
    if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
    if (!c || !p) return M2S_ERR_INVALID;
    if (p->level > 10 || p->max_group < 2 || p->max_group > 64) return fail(c, M2S_ERR_INVALID, "level above 10 or max_group outside 2..64");
    if (std::isnan(p->min_axis_dot)) return fail(c, M2S_ERR_INVALID, "min_axis_dot is NaN");
    // (bit 1 names nothing: callers were promised that flags 2 and 3 are refused, so the second flag is bit 2)
    if ((p->flags & ~(uint32_t)(M2S_MERGE_DRY_RUN | M2S_MERGE_UNSIGNED_AXIS)) || p->reserved[0] != 0 || p->reserved[1] != 0)
        return fail(c, M2S_ERR_INVALID, "unknown flag bits or reserved != 0");
    M2S_TRY(merge_run(c, p->level, p->max_group, p->min_axis_dot, (p->flags & M2S_MERGE_DRY_RUN) ? MergeMode::Dry : MergeMode::Apply,
                      (p->flags & M2S_MERGE_UNSIGNED_AXIS) != 0));
    if (out_counts) std::memcpy(out_counts, c->last_merge_counts, sizeof(c->last_merge_counts));
    return M2S_OK;
}

m2s_status m2s_last_merge_counts(const m2s_ctx* c, uint64_t out[4]) { return get_array(c, &m2s_ctx::last_merge_counts, out); }

m2s_status m2s_last_merge_stage_ms(const m2s_ctx* c, float out_ms[3]) { return get_array(c, &m2s_ctx::last_merge_stage_ms, out_ms); }

float m2s_last_merge_sh_ms(const m2s_ctx* c) { return c ? c->last_merge_sh_ms : 0.0f; }

const void* m2s_device_merge_map(const m2s_ctx* c) { return c && merge_map_valid(c) && c->merge_map_tag.n ? c->d_merge_map.get() : nullptr; }

m2s_status m2s_download_merge_map(m2s_ctx* c, uint32_t* dst, uint64_t capacity, uint64_t* out_n) {
    if (out_n) *out_n = 0;
    if (!c) return M2S_ERR_INVALID;
    if (!merge_map_valid(c)) return fail(c, M2S_ERR_STATE, "no merge map of the current records (m2s_merge; the records changed since)");
    if (out_n) *out_n = c->merge_map_tag.n;
    if (!dst) return capacity ? fail(c, M2S_ERR_INVALID, "no destination") : M2S_OK;
    if (capacity < c->merge_map_tag.n) return fail(c, M2S_ERR_CAPACITY, "destination holds fewer entries than there were records");
    if (!c->merge_map_tag.n) return M2S_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_merge_map, c->merge_map_tag.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return M2S_OK;
}

}  // extern "C"
