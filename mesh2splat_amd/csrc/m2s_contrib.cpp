// m2s_contrib.cpp — the contribution pass (what every record adds to a view's picture) and the pruning of the records nobody sees:
// host side of m2s_contrib.hip.  The binning stages in front of the contribution blend are the splat pass's own (splat_bin, m2s_splat.cpp).
#include "m2s_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace m2s;
using namespace m2s_host;

namespace m2s_host {

m2s_status prune_compact_enqueue(m2s_ctx* c, uint64_t n, uint64_t kept, const uint32_t* flags, const uint32_t* offsets, bool sh, const void* src) {
    if (!n) {
        if (!c->lane[0].records || c->last_records != c->lane[0].records) return ensure_records(c, 1);
        return M2S_OK;
    }
    // The survivors go into the pool.  Records that live there already (or a plane compacted in place) cannot be compacted onto
    // themselves by independent lanes: they go through a staging buffer and are copied back, stream-ordered.
    const bool in_pool = !src && c->last_records == c->lane[0].records;
    const uint64_t stage_bytes = std::max<uint64_t>(in_pool ? kept * sizeof(m2s_gaussian) : 0, sh ? kept * 48 * sizeof(float) : 0);
    if (stage_bytes) M2S_TRY(c->d_prune_stage.reserve(c->err, stage_bytes, 1));
    if (!src) src = c->last_records;
    if (!in_pool) if (m2s_status s = ensure_records(c, std::max<uint64_t>(kept, 1))) return s;
    if (kept) {
        float4* dst = in_pool ? c->d_prune_stage.get() : (float4*)c->lane[0].records.get();
        HIPCHK(c, prune_compact((const float4*)src, flags, offsets, (uint32_t)n, 6, dst, c->stream));
        if (in_pool) HIPCHK(c, hipMemcpyAsync(c->lane[0].records, c->d_prune_stage, kept * sizeof(m2s_gaussian), hipMemcpyDeviceToDevice, c->stream));
        if (sh) {
            HIPCHK(c, prune_compact((const float4*)c->d_sh.get(), flags, offsets, (uint32_t)n, 12, c->d_prune_stage, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->d_sh, c->d_prune_stage, kept * 48 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        }
    }
    return M2S_OK;
}

}  // namespace m2s_host

extern "C" {

m2s_status m2s_upload_quad_sources(m2s_ctx* c, const uint32_t* host_sources, uint64_t n) {
    if (!c || (n && !host_sources)) return M2S_ERR_INVALID;
    if (!c->sq_n || n != c->sq_n) return fail(c, M2S_ERR_INVALID, "the number of sources is not the number of sorted quads");
    for (uint64_t i = 0; i < n; ++i)
        if (host_sources[i] >= c->last_stored) return fail(c, M2S_ERR_INVALID, "a source index is not below the number of records");
    HIPCHK(c, hipSetDevice(c->device));
    c->sq_src = nullptr;
    M2S_TRY(c->d_sq_src.reserve(c->err, n, sizeof(uint32_t)));
    HIPCHK(c, hipMemcpy(c->d_sq_src, host_sources, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->sq_src = c->d_sq_src;
    c->sq_src_tag.set(*c, n);
    return M2S_OK;
}

m2s_status m2s_contrib_begin(m2s_ctx* c) {
    if (!c) return M2S_ERR_INVALID;
    uint64_t n = 0;
    M2S_TRY(need_records(c, &n));
    HIPCHK(c, hipSetDevice(c->device));
    c->contrib_tag.clear();
    M2S_TRY(c->d_contrib.reserve(c->err, std::max<uint64_t>(n, 1), 2 * sizeof(uint32_t)));
    HIPCHK(c, hipMemsetAsync(c->d_contrib, 0, c->d_contrib.cap() * 2 * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->contrib_tag.set(*c, n);
    return M2S_OK;
}

m2s_status m2s_upload_contrib(m2s_ctx* c, const uint32_t* host_wmax, const uint32_t* host_npix, uint64_t n) {
    if (!c) return M2S_ERR_INVALID;
    if (!contrib_valid(c)) return fail(c, M2S_ERR_STATE, "no accumulators of the current records (m2s_contrib_begin)");
    if (n != c->contrib_tag.n) return fail(c, M2S_ERR_INVALID, "the number of words is not the number of records");
    if (host_wmax)
        for (uint64_t i = 0; i < n; ++i)
            if (host_wmax[i] > 0x3F800000u) return fail(c, M2S_ERR_INVALID, "a wmax word is not the bits of a weight in [0, 1]");
    if (!n) return M2S_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (host_wmax) HIPCHK(c, hipMemcpy(c->d_contrib, host_wmax, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (host_npix) HIPCHK(c, hipMemcpy(c->d_contrib + c->d_contrib.cap(), host_npix, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    return M2S_OK;
}

m2s_status m2s_contrib_accumulate(m2s_ctx* c, const m2s_splat_params* p, float count_weight) {
    if (!c || !p) return M2S_ERR_INVALID;
    const int W = p->resolution[0], H = p->resolution[1];
    M2S_TRY(check_resolution(c, W, H));
    if (p->render_mode < 0 || p->render_mode > 6 || p->reserved != 0) return fail(c, M2S_ERR_INVALID, "render mode outside 0..6 or reserved != 0");
    if (p->render_mode == 4) return fail(c, M2S_ERR_INVALID, "render mode 4 (overdraw) has no fragment weight");
    if (!(count_weight >= 0.0f) || !std::isfinite(count_weight)) return fail(c, M2S_ERR_INVALID, "count_weight is negative or not finite");
    if (!c->contrib_tag.is_set()) return fail(c, M2S_ERR_INVALID, "no m2s_contrib_begin");
    if (!contrib_valid(c)) return fail(c, M2S_ERR_INVALID, "the records changed since m2s_contrib_begin");
    if (!c->sq_n) return fail(c, M2S_ERR_INVALID, "no sorted quads (run m2s_prepass_sorted)");
    if (!c->sq_src || !c->sq_src_tag.holds(*c))
        return fail(c, M2S_ERR_INVALID, "the sorted quads carry no sources (they come from m2s_prepass_sorted or m2s_upload_quad_sources)");
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t nq = (uint32_t)c->sq_n;
    SplatBins bins;
    if (m2s_status s = splat_bin(c, c->d_sorted_quads, nq, W, H, &bins)) return s;
    if (bins.pairs)
        HIPCHK(c, contrib_blend((const float4*)c->splat_work.rec.get(), bins.vals, bins.ranges, bins.order, W, H, c->sq_src, count_weight, c->d_contrib,
                                c->d_contrib + c->d_contrib.cap(), c->stream));
    HIPCHK(c, c->bin_clock.mark(BinMark::Blended, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->bin_clock.on()) {
        M2S_TRY(splat_stage_ms(c, c->last_contrib_stage_ms));
        c->last_contrib_ms = (c->last_contrib_stage_ms[0] + c->last_contrib_stage_ms[1]) + c->last_contrib_stage_ms[2];
    }
    return M2S_OK;
}

const void* m2s_device_contrib(const m2s_ctx* c, uint32_t which) {
    return c && which < 2 && contrib_valid(c) ? c->d_contrib + which * c->d_contrib.cap() : nullptr;
}

m2s_status m2s_download_contrib(m2s_ctx* c, uint32_t* dst_wmax, uint32_t* dst_npix, uint64_t capacity) {
    if (!c) return M2S_ERR_INVALID;
    if (!contrib_valid(c)) return fail(c, M2S_ERR_STATE, "no accumulators of the current records (m2s_contrib_begin)");
    const uint64_t n = c->contrib_tag.n;
    if (capacity < n) return fail(c, M2S_ERR_CAPACITY, "destination holds fewer entries than there are records");
    if (!n) return M2S_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (dst_wmax) HIPCHK(c, hipMemcpy(dst_wmax, c->d_contrib, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (dst_npix) HIPCHK(c, hipMemcpy(dst_npix, c->d_contrib + c->d_contrib.cap(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return M2S_OK;
}

float m2s_last_contrib_ms(const m2s_ctx* c) { return c ? c->last_contrib_ms : 0.0f; }

m2s_status m2s_last_contrib_stage_ms(const m2s_ctx* c, float out_ms[3]) { return get_array(c, &m2s_ctx::last_contrib_stage_ms, out_ms); }

m2s_status m2s_prune(m2s_ctx* c, const m2s_prune_params* p, uint64_t* out_kept) {
    if (!c || !p) return M2S_ERR_INVALID;
    if (p->reserved != 0 || std::isnan(p->min_weight)) return fail(c, M2S_ERR_INVALID, "min_weight is NaN or reserved != 0");
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    if (!contrib_valid(c)) return fail(c, M2S_ERR_STATE, "no accumulators of the current records (m2s_contrib_begin, m2s_contrib_accumulate)");
    HIPCHK(c, hipSetDevice(c->device));
    M2S_TRY(c->prune_clock.begin(c->err, c->profiling));
    const uint64_t n = c->last_stored;
    const uint32_t R = c->last_R;
    uint64_t kept = 0, by_w = 0, by_p = 0;
    const bool sh = prune_sh_plane(c, n);
    HIPCHK(c, c->prune_clock.mark(SpanMark::Begin, c->stream));
    if (n) {
        // flags | offsets | two 64-bit counters
        M2S_TRY(c->d_prune_u32.reserve(c->err, n, 2 * sizeof(uint32_t)));
        unsigned long long* counters = nullptr;
        {   // (the counters live behind the scan's work area, 16-byte aligned)
            const uint64_t want = align_up(prune_scan_temp_bytes((uint32_t)n), 16) + 2 * sizeof(unsigned long long);
            M2S_TRY(c->d_prune_temp.reserve(c->err, want, 1));
            counters = reinterpret_cast<unsigned long long*>(c->d_prune_temp + c->d_prune_temp.cap() - 2 * sizeof(unsigned long long));
        }
        uint32_t* flags = c->d_prune_u32;
        uint32_t* offsets = flags + c->d_prune_u32.cap();
        HIPCHK(c, hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), c->stream));
        HIPCHK(c, prune_flags_scan(c->d_contrib, c->d_contrib + c->d_contrib.cap(), (uint32_t)n, p->min_weight, p->min_pixels, flags, offsets, counters,
                                   c->d_prune_temp, c->d_prune_temp.cap() - 2 * sizeof(unsigned long long), c->stream));
        unsigned long long h[2] = { 0, 0 };
        HIPCHK(c, hipMemcpyAsync(h, counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        by_w = h[0]; by_p = h[1];
        kept = n - by_w - by_p;
        M2S_TRY(prune_compact_enqueue(c, n, kept, flags, offsets, sh));
    } else {
        M2S_TRY(prune_compact_enqueue(c, 0, 0, nullptr, nullptr, false));
    }
    HIPCHK(c, c->prune_clock.mark(SpanMark::End, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->prune_clock.on()) HIPCHK(c, c->prune_clock.span(SpanMark::Begin, SpanMark::End, &c->last_prune_ms));
    c->rewritten(c->lane[0].records, kept, R, sh ? Rewrite::PruneWithSh : Rewrite::Prune);
    c->last_prune_counts[0] = n; c->last_prune_counts[1] = kept; c->last_prune_counts[2] = by_w; c->last_prune_counts[3] = by_p;
    if (out_kept) *out_kept = kept;
    return M2S_OK;
}

m2s_status m2s_last_prune_counts(const m2s_ctx* c, uint64_t out[4]) { return get_array(c, &m2s_ctx::last_prune_counts, out); }

float m2s_last_prune_ms(const m2s_ctx* c) { return c ? c->last_prune_ms : 0.0f; }

}  // extern "C"
