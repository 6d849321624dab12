// m2s_refit.cpp — the colour refit (m2s_refit_begin / _accumulate / _apply): host side of m2s_refit.hip.  The binning stages in front of
// the refit blend are the splat pass's own (splat_bin, m2s_splat.cpp); what the apply does to the context: m2s_recstate.h, Rewrite::RefitApply.
#include "m2s_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace m2s;
using namespace m2s_host;

namespace {

bool refit_valid(const m2s_ctx* c) { return c->refit_tag.holds(*c, c->last_stored); }
long long* refit_num(const m2s_ctx* c) { return reinterpret_cast<long long*>(c->d_refit.get()); }
unsigned long long* refit_den(const m2s_ctx* c) { return c->d_refit + 3 * c->d_refit.cap(); }
const char* const kNoRefitMsg = "no accumulators of the current records (m2s_refit_begin)";

}  // namespace

extern "C" {

m2s_status m2s_refit_begin(m2s_ctx* c) {
    if (!c) return M2S_ERR_INVALID;
    uint64_t n = 0;
    M2S_TRY(need_records(c, &n));
    HIPCHK(c, hipSetDevice(c->device));
    c->refit_tag.clear();
    M2S_TRY(c->d_refit.reserve(c->err, std::max<uint64_t>(n, 1), 4 * sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->d_refit, 0, c->d_refit.cap() * 4 * sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->refit_tag.set(*c, n);
    return M2S_OK;
}

m2s_status m2s_refit_accumulate(m2s_ctx* c, const m2s_refit_params* p, const void* d_target, const void* d_render, uint64_t out_counts[2]) {
    if (!c || !p) return M2S_ERR_INVALID;
    const int W = p->resolution[0], H = p->resolution[1];
    M2S_TRY(check_resolution(c, W, H));
    if (p->min_cover < 1 || p->min_cover > 255 || p->reserved != 0) return fail(c, M2S_ERR_INVALID, "min_cover outside 1..255 or reserved != 0");
    if (!c->refit_tag.is_set()) return fail(c, M2S_ERR_INVALID, "no m2s_refit_begin");
    if (!refit_valid(c)) return fail(c, M2S_ERR_INVALID, "the records changed since m2s_refit_begin");
    if (!c->sq_n) return fail(c, M2S_ERR_INVALID, "no sorted quads (run m2s_prepass_sorted)");
    if (!c->sq_src || !c->sq_src_tag.holds(*c))
        return fail(c, M2S_ERR_INVALID, "the sorted quads carry no sources (they come from m2s_prepass_sorted or m2s_upload_quad_sources)");
    if (!d_target) {
        if (c->mr_w != W || c->mr_h != H) return fail(c, M2S_ERR_STATE, "no mesh G-buffer of this resolution exists (run m2s_mesh_render)");
        d_target = c->d_mr_gbuf.ptr[2];
    }
    if (!d_render) {
        if (c->gbuf_w != W || c->gbuf_h != H) return fail(c, M2S_ERR_STATE, "no G-buffer of this resolution exists (run m2s_splat)");
        d_render = c->d_gbuf.ptr[2];
    }
    HIPCHK(c, hipSetDevice(c->device));
    SplatBins bins;
    if (m2s_status s = splat_bin(c, c->d_sorted_quads, (uint32_t)c->sq_n, W, H, &bins)) return s;
    // (without pairs the kernel still runs: it counts the participating pixels; d_totals[3] is zero behind splat_bin)
    BinWork& w = c->splat_work;
    HIPCHK(c, refit_blend((const float4*)w.rec.get(), bins.vals, bins.ranges, bins.order, W, H, c->sq_src, (const uint32_t*)d_target,
                          (const uint32_t*)d_render, p->min_cover, refit_num(c), refit_den(c), w.d_totals + 3, c->stream));
    HIPCHK(c, c->bin_clock.mark(BinMark::Blended, c->stream));
    HIPCHK(c, hipMemcpyAsync(w.h_totals + 3, w.d_totals + 3, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->bin_clock.on()) M2S_TRY(splat_stage_ms(c, c->last_refit_stage_ms));
    if (out_counts) { out_counts[0] = w.h_totals[3]; out_counts[1] = bins.pairs; }
    return M2S_OK;
}

const void* m2s_device_refit(const m2s_ctx* c, uint32_t which) {
    if (!c || which > 1 || !refit_valid(c)) return nullptr;
    return which ? (const void*)refit_den(c) : (const void*)refit_num(c);
}

m2s_status m2s_download_refit(m2s_ctx* c, int64_t* dst_num, uint64_t* dst_den, uint64_t capacity) {
    if (!c) return M2S_ERR_INVALID;
    if (!refit_valid(c)) return fail(c, M2S_ERR_STATE, kNoRefitMsg);
    const uint64_t n = c->refit_tag.n;
    if (capacity < n) return fail(c, M2S_ERR_CAPACITY, "destination holds fewer entries than there are records");
    if (!n) return M2S_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (dst_num) HIPCHK(c, hipMemcpy(dst_num, refit_num(c), n * 3 * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (dst_den) HIPCHK(c, hipMemcpy(dst_den, refit_den(c), n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return M2S_OK;
}

m2s_status m2s_upload_refit(m2s_ctx* c, const int64_t* host_num, const uint64_t* host_den, uint64_t n) {
    if (!c) return M2S_ERR_INVALID;
    if (!refit_valid(c)) return fail(c, M2S_ERR_STATE, kNoRefitMsg);
    if (n != c->refit_tag.n) return fail(c, M2S_ERR_INVALID, "the number of entries is not the number of records");
    if (!n) return M2S_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (host_num) HIPCHK(c, hipMemcpy(refit_num(c), host_num, n * 3 * sizeof(int64_t), hipMemcpyHostToDevice));
    if (host_den) HIPCHK(c, hipMemcpy(refit_den(c), host_den, n * sizeof(uint64_t), hipMemcpyHostToDevice));
    return M2S_OK;
}

m2s_status m2s_refit_apply(m2s_ctx* c, const m2s_refit_apply_params* p, uint64_t out_counts[4]) {
    if (!c || !p) return M2S_ERR_INVALID;
    if (!std::isfinite(p->step) || !std::isfinite(p->min_weight_sum) || p->min_weight_sum < 0.0f || p->reserved[0] != 0 || p->reserved[1] != 0)
        return fail(c, M2S_ERR_INVALID, "step is not finite, min_weight_sum is negative or not finite, or reserved != 0");
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    if (!refit_valid(c)) return fail(c, M2S_ERR_STATE, kNoRefitMsg);
    HIPCHK(c, hipSetDevice(c->device));
    M2S_TRY(c->refit_apply_clock.begin(c->err, c->profiling));
    M2S_TRY(c->d_refit_counts.reserve(c->err, 3, sizeof(unsigned long long)));
    const uint64_t n = c->last_stored;
    const uint32_t R = c->last_R;
    const double dq = (double)p->min_weight_sum * 65536.0;
    const unsigned long long D = dq >= 9223372036854775808.0 ? ~0ull : (unsigned long long)std::llrint(dq);
    unsigned long long h[3] = { 0, 0, 0 };
    HIPCHK(c, c->refit_apply_clock.mark(SpanMark::Begin, c->stream));
    if (n) {
        // the update happens in the pool: records that live elsewhere (uploaded, adopted, a second lane's) are copied there first
        if (c->last_records != c->lane[0].records) {
            const void* src = c->last_records;
            M2S_TRY(ensure_records(c, n));
            HIPCHK(c, hipMemcpyAsync(c->lane[0].records, src, n * sizeof(m2s_gaussian), hipMemcpyDeviceToDevice, c->stream));
        }
        HIPCHK(c, hipMemsetAsync(c->d_refit_counts, 0, 3 * sizeof(unsigned long long), c->stream));
        HIPCHK(c, refit_apply((float4*)c->lane[0].records.get(), refit_num(c), refit_den(c), (uint32_t)n, (double)p->step, D, c->d_refit_counts,
                              c->stream));
        HIPCHK(c, hipMemcpyAsync(h, c->d_refit_counts, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    } else {
        M2S_TRY(prune_compact_enqueue(c, 0, 0, nullptr, nullptr, false));
    }
    HIPCHK(c, c->refit_apply_clock.mark(SpanMark::End, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->refit_apply_clock.on()) HIPCHK(c, c->refit_apply_clock.span(SpanMark::Begin, SpanMark::End, &c->last_refit_apply_ms));
    c->rewritten(c->lane[0].records, n, R, Rewrite::RefitApply);   // (a plane of these records was baked from the old albedo: dropped)
    if (out_counts) { out_counts[0] = n; out_counts[1] = h[0]; out_counts[2] = h[1]; out_counts[3] = h[2]; }
    return M2S_OK;
}

m2s_status m2s_last_refit_stage_ms(const m2s_ctx* c, float out_ms[3]) { return get_array(c, &m2s_ctx::last_refit_stage_ms, out_ms); }

float m2s_last_refit_apply_ms(const m2s_ctx* c) { return c ? c->last_refit_apply_ms : 0.0f; }

}  // extern "C"
