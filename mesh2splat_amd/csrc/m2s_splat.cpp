// m2s_splat.cpp — the splat pass (GaussianSplattingPass.cpp:50-95) on the sorted quads: host side of m2s_splat.hip.
#include "m2s_ctx.h"

#include <algorithm>
#include <cstring>

using namespace m2s;
using namespace m2s_host;

namespace m2s_host {

m2s_status splat_bin(m2s_ctx* c, const void* d_quads, uint32_t nq, int W, int H, SplatBins* out) {
    BinWork& w = c->splat_work;
    M2S_TRY(w.reserve_totals(c->err, 4, 4 * sizeof(unsigned long long)));
    const int tiles_x = (W + kSplatTile - 1) / kSplatTile, tiles_y = (H + kSplatTile - 1) / kSplatTile;
    const uint32_t n_tiles = (uint32_t)(tiles_x * tiles_y);
    HIPCHK(c, hipMemsetAsync(w.d_totals, 0, 4 * sizeof(unsigned long long), c->stream));
    ClockOf<BinMark>& clock = c->bin_clock;
    M2S_TRY(clock.begin(c->err, c->profiling));
    uint64_t pairs = 0;
    *out = SplatBins();
    if (nq) {
        // ---- setup: records, tile counts, their scan; the number of pairs read back once (the pair buffers are sized from it)
        M2S_TRY(w.reserve_items(c->err, nq, kSplatRecBytes));
        M2S_TRY(w.reserve_temp(c->err, splat_scan_temp_bytes(nq)));
        HIPCHK(c, clock.mark(BinMark::Setup, c->stream));
        HIPCHK(c, splat_setup((const float4*)d_quads, nq, W, H, (float4*)w.rec.get(), w.cnt, w.off, w.temp, w.temp.cap(), w.d_totals, c->stream));
        HIPCHK(c, clock.mark(BinMark::SetupEnd, c->stream));
        HIPCHK(c, hipMemcpyAsync(w.h_totals, w.d_totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        pairs = w.h_totals[0];
        out->skipped = w.h_totals[1];
        if (pairs > 0x7FFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^31-1 (tile, quad) pairs");
    }
    HIPCHK(c, clock.mark(BinMark::Pairs, c->stream));
    out->pairs = pairs;
    if (pairs) {
        BinWork::Pairs pr;
        M2S_TRY(w.reserve_pairs(c->err, pairs, &pr));
        M2S_TRY(c->d_splat_tiles.reserve(c->err, n_tiles, 5 * sizeof(uint32_t)));
        M2S_TRY(w.reserve_temp(c->err, splat_sort_temp_bytes((uint32_t)pairs, n_tiles)));
        const uint64_t tc = c->d_splat_tiles.cap();
        uint2* rg = reinterpret_cast<uint2*>(c->d_splat_tiles.get());
        uint32_t* len = c->d_splat_tiles + 2 * tc;
        uint32_t* len_sorted = len + tc;
        uint32_t* ord = len_sorted + tc;
        HIPCHK(c, splat_pairs((const float4*)w.rec.get(), w.cnt, w.off, nq, tiles_x, pr.keys_in, pr.vals_in, c->stream));
        HIPCHK(c, clock.mark(BinMark::Paired, c->stream));
        HIPCHK(c, splat_group(pr.keys_in, pr.vals_in, pr.keys_out, pr.vals_out, (uint32_t)pairs, n_tiles, rg, len, len_sorted, ord, w.temp,
                              w.temp.cap(), c->stream));
        out->vals = pr.vals_out; out->ranges = rg; out->order = ord;
    } else HIPCHK(c, clock.mark(BinMark::Paired, c->stream));   // (no pairs: both spans close around nothing, small and not 0, as they always have)
    HIPCHK(c, clock.mark(BinMark::Grouped, c->stream));
    return M2S_OK;
}

m2s_status splat_stage_ms(m2s_ctx* c, float out[3]) {
    const ClockOf<BinMark>& clock = c->bin_clock;
    float a = 0, b = 0, g = 0, bl = 0;
    HIPCHK(c, clock.span(BinMark::Setup, BinMark::SetupEnd, &a));      // (0 without quads: no setup ran)
    HIPCHK(c, clock.span(BinMark::Pairs, BinMark::Paired, &b));
    HIPCHK(c, clock.span(BinMark::Paired, BinMark::Grouped, &g));
    HIPCHK(c, clock.span(BinMark::Grouped, BinMark::Blended, &bl));
    out[0] = a + b; out[1] = g; out[2] = bl;
    return M2S_OK;
}

}  // namespace m2s_host

extern "C" {

m2s_status m2s_upload_quads(m2s_ctx* c, const m2s_quad* host_quads, uint64_t n) {
    if (!c || (n && !host_quads)) return M2S_ERR_INVALID;
    if (n > 0xFFFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^32-1 quads");
    HIPCHK(c, hipSetDevice(c->device));
    c->sq_n = 0;
    c->sq_src = nullptr;
    if (!n) return M2S_OK;
    M2S_TRY(c->d_sorted_quads.reserve(c->err, n, sizeof(m2s_quad)));
    HIPCHK(c, hipMemcpy(c->d_sorted_quads, host_quads, n * sizeof(m2s_quad), hipMemcpyHostToDevice));
    c->sq_n = n;
    return M2S_OK;
}

// GaussianSplattingPass::execute: clear, then one instanced draw of the sorted quads with the pass's blend state.
m2s_status m2s_splat(m2s_ctx* c, const m2s_splat_params* p, const void* d_quads, uint64_t n, uint64_t* out_skipped) {
    if (!c || !p) return M2S_ERR_INVALID;
    const int W = p->resolution[0], H = p->resolution[1];
    M2S_TRY(check_resolution(c, W, H));
    if (p->render_mode < 0 || p->render_mode > 6 || p->reserved != 0) return fail(c, M2S_ERR_INVALID, "render mode outside 0..6 or reserved != 0");
    if (!d_quads) {
        if (!c->sq_n) return fail(c, M2S_ERR_INVALID, "no sorted quads (run m2s_sort_prepass / m2s_prepass_sorted / m2s_upload_quads, or pass d_quads)");
        d_quads = c->d_sorted_quads;
        n = c->sq_n;
    }
    if (n > 0xFFFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^32-1 quads");
    HIPCHK(c, hipSetDevice(c->device));
    if (out_skipped) *out_skipped = 0;
    c->gbuf_w = c->gbuf_h = 0;
    for (uint64_t& v : c->last_splat_counts) v = 0;
    const uint64_t px = (uint64_t)W * (uint64_t)H;
    M2S_TRY(c->d_gbuf.reserve(c->err, px));
    const uint32_t nq = (uint32_t)n;
    SplatBins bins;
    const m2s_status bs = splat_bin(c, d_quads, nq, W, H, &bins);
    c->last_splat_counts[2] = bins.skipped;
    if (out_skipped) *out_skipped = bins.skipped;
    if (bs != M2S_OK) return bs;
    const uint64_t pairs = bins.pairs;
    const uint32_t* vals = bins.vals;
    const uint2* ranges = bins.ranges;
    const uint32_t* order = bins.order;
    // ---- blend: every tile writes its 16 x 16 pixels of all five planes once (tiles without quads write the cleared values)
    BinWork& w = c->splat_work;
    HIPCHK(c, splat_blend((const float4*)w.rec.get(), vals, ranges, order, W, H, p->render_mode, c->d_gbuf.ptr, w.d_totals + 2, c->stream));
    HIPCHK(c, c->bin_clock.mark(BinMark::Blended, c->stream));
    HIPCHK(c, hipMemcpyAsync(w.h_totals + 2, w.d_totals + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->last_splat_counts[0] = pairs;
    c->last_splat_counts[1] = w.h_totals[2];
    if (c->bin_clock.on()) {
        M2S_TRY(splat_stage_ms(c, c->last_splat_stage_ms));
        c->last_splat_ms = (c->last_splat_stage_ms[0] + c->last_splat_stage_ms[1]) + c->last_splat_stage_ms[2];
    }
    c->gbuf_w = W;
    c->gbuf_h = H;
    return M2S_OK;
}

const void* m2s_device_gbuffer(const m2s_ctx* c, uint32_t attachment) {
    return c && c->gbuf_w && attachment < 5 ? c->d_gbuf.ptr[attachment] : nullptr;
}

m2s_status m2s_download_gbuffer(m2s_ctx* c, uint32_t attachment, void* dst, uint64_t capacity_bytes) {
    if (!c || attachment >= 5 || !dst) return M2S_ERR_INVALID;
    if (!c->gbuf_w) return fail(c, M2S_ERR_STATE, "no splat has run");
    const uint64_t bytes = (uint64_t)c->gbuf_w * (uint64_t)c->gbuf_h * ((attachment == 2 || attachment == 4) ? 4 : 8);
    if (capacity_bytes < bytes) return fail(c, M2S_ERR_CAPACITY, "destination smaller than the attachment");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_gbuf.ptr[attachment], bytes, hipMemcpyDeviceToHost));
    return M2S_OK;
}

float m2s_last_splat_ms(const m2s_ctx* c) { return c ? c->last_splat_ms : 0.0f; }

m2s_status m2s_last_splat_stage_ms(const m2s_ctx* c, float out_ms[3]) { return get_array(c, &m2s_ctx::last_splat_stage_ms, out_ms); }

m2s_status m2s_last_splat_counts(const m2s_ctx* c, uint64_t out[3]) { return get_array(c, &m2s_ctx::last_splat_counts, out); }

}  // extern "C"
