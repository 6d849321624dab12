// m2s_score.cpp — the fidelity score (m2s_score_frames): host side of m2s_score.hip.
#include "m2s_ctx.h"

#include <cstring>

using namespace m2s;
using namespace m2s_host;

extern "C" {

m2s_status m2s_score_frames(m2s_ctx* c, const m2s_score_params* p, const void* d_a, const void* d_b, const void* d_cover_a, const void* d_cover_b,
                            m2s_score_result* out) {
    if (!c || !p || !out) return M2S_ERR_INVALID;
    const int W = p->resolution[0], H = p->resolution[1];
    M2S_TRY(check_resolution(c, W, H));
    if (p->mask_mode > 3) return fail(c, M2S_ERR_INVALID, "mask mode outside 0..3");
    if (p->flags & ~(uint32_t)(M2S_SCORE_NO_COVER | M2S_SCORE_WANT_MAP)) return fail(c, M2S_ERR_INVALID, "unknown flag");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(c, M2S_ERR_INVALID, "reserved != 0");
    c->score_map_w = c->score_map_h = 0;
    const bool cover = !(p->flags & M2S_SCORE_NO_COVER), want_map = (p->flags & M2S_SCORE_WANT_MAP) != 0;
    if (!d_a) {
        if (c->mesh_frame_w != W || c->mesh_frame_h != H) return fail(c, M2S_ERR_STATE, "no mesh frame of this resolution exists (run m2s_relight_mesh)");
        d_a = c->d_mesh_frame;
    }
    if (!d_b) {
        if (c->frame_w != W || c->frame_h != H) return fail(c, M2S_ERR_STATE, "no frame of this resolution exists (run m2s_relight)");
        d_b = c->d_frame;
    }
    if (cover && !d_cover_a) {
        if (c->mr_w != W || c->mr_h != H) return fail(c, M2S_ERR_STATE, "no mesh G-buffer of this resolution exists (run m2s_mesh_render)");
        d_cover_a = c->d_mr_gbuf.ptr[2];
    }
    if (cover && !d_cover_b) {
        if (c->gbuf_w != W || c->gbuf_h != H) return fail(c, M2S_ERR_STATE, "no G-buffer of this resolution exists (run m2s_splat)");
        d_cover_b = c->d_gbuf.ptr[2];
    }
    HIPCHK(c, hipSetDevice(c->device));
    constexpr size_t kWords = (size_t)kScoreShards * kScoreCounters;
    M2S_TRY(c->d_score_acc.reserve(c->err, kWords, sizeof(unsigned long long)));
    M2S_TRY(c->h_score.ensure(c->err, kWords * sizeof(unsigned long long)));
    M2S_TRY(c->score_clock.begin(c->err, c->profiling));
    if (want_map) M2S_TRY(c->d_score_map.reserve(c->err, (uint64_t)W * (uint64_t)H, 4));
    ScoreK k;
    k.W = W; k.H = H;
    k.mask_mode = p->mask_mode;
    k.tiles_x = score_tiles(W);
    HIPCHK(c, hipMemsetAsync(c->d_score_acc, 0, kWords * sizeof(unsigned long long), c->stream));
    HIPCHK(c, c->score_clock.mark(SpanMark::Begin, c->stream));
    HIPCHK(c, launch_score(k, (const uint32_t*)d_a, (const uint32_t*)d_b, cover ? (const uint32_t*)d_cover_a : nullptr,
                           cover ? (const uint32_t*)d_cover_b : nullptr, want_map ? c->d_score_map.get() : nullptr, c->d_score_acc, c->stream));
    HIPCHK(c, c->score_clock.mark(SpanMark::End, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_score, c->d_score_acc, kWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->score_clock.on()) HIPCHK(c, c->score_clock.span(SpanMark::Begin, SpanMark::End, &c->last_score_ms));
    // the shards are integers: their sum (max_abs: their maximum) does not depend on which workgroup added where
    unsigned long long t[kScoreCounters] = {};
    for (int s = 0; s < kScoreShards; ++s)
        for (int i = 0; i < kScoreCounters; ++i) {
            const unsigned long long v = c->h_score[s * kScoreCounters + i];
            if (i >= kScoreMaxFirst && i <= kScoreMaxLast) t[i] = v > t[i] ? v : t[i];
            else t[i] += v;
        }
    std::memset(out, 0, sizeof(*out));
    out->pixels = t[0];
    for (int i = 0; i < 4; ++i) out->cover[i] = t[1 + i];
    for (int i = 0; i < 3; ++i) { out->sse[i] = t[5 + i]; out->sad[i] = t[8 + i]; out->max_abs[i] = (uint32_t)t[11 + i]; }
    out->windows = t[14];
    out->ssim_q32 = (int64_t)t[15];
    if (want_map) { c->score_map_w = W; c->score_map_h = H; }
    return M2S_OK;
}

const void* m2s_device_score_map(const m2s_ctx* c) { return c && c->score_map_w ? c->d_score_map.get() : nullptr; }

m2s_status m2s_download_score_map(m2s_ctx* c, void* dst, uint64_t capacity_bytes) {
    if (!c || !dst) return M2S_ERR_INVALID;
    if (!c->score_map_w) return fail(c, M2S_ERR_STATE, "the last m2s_score_frames kept no error map (M2S_SCORE_WANT_MAP)");
    const uint64_t bytes = (uint64_t)c->score_map_w * (uint64_t)c->score_map_h * 4;
    if (capacity_bytes < bytes) return fail(c, M2S_ERR_CAPACITY, "destination smaller than the map");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_score_map, bytes, hipMemcpyDeviceToHost));
    return M2S_OK;
}

float m2s_last_score_ms(const m2s_ctx* c) { return c ? c->last_score_ms : 0.0f; }

}  // extern "C"
