// m2s_light.cpp — the shadow pass (GaussianShadowPass.cpp:83-236) and the deferred relighting pass (GaussianRelightingPass.cpp:136-143):
// host side of m2s_light.hip.
#include "m2s_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace m2s;
using namespace m2s_host;

namespace {

constexpr int kPinnedBases = 8;     // shadow_work.h_totals: [0..2] totals | 8 x u32 bases from word 8 | 96 floats of view matrices from word 16
constexpr int kPinnedViews = 16;
constexpr size_t kPinnedBytes = kPinnedViews * 8 + 96 * sizeof(float);

m2s_status ensure_light_common(m2s_ctx* c) {
    M2S_TRY(c->shadow_work.reserve_totals(c->err, 4, kPinnedBytes));
    return c->d_sh_views.reserve(c->err, 96 + 8, sizeof(float));
}

// The six cameras of the light (GaussianShadowPass.cpp:91-108: glm::lookAt(light, light + axis, up)) and the 90 degree / aspect 1
// glm::perspective, in double, rounded to float, column-major.  `light + axis - light` is taken as the axis itself, so the rotation
// part is an exact signed permutation and the translation the (exactly representable) negated, permuted light position;
// 1 / tan(45 degrees) is 1.
void shadow_cameras(const float light[3], float near_p, float far_p, float views[96], float proj[16]) {
    static const double F[6][3] = { { 1, 0, 0 }, { -1, 0, 0 }, { 0, 1, 0 }, { 0, -1, 0 }, { 0, 0, 1 }, { 0, 0, -1 } };
    static const double UP[6][3] = { { 0, -1, 0 }, { 0, -1, 0 }, { 0, 0, 1 }, { 0, 0, -1 }, { 0, -1, 0 }, { 0, -1, 0 } };
    const double eye[3] = { light[0], light[1], light[2] };
    for (int fc = 0; fc < 6; ++fc) {
        const double* f = F[fc];
        const double* up = UP[fc];
        const double s[3] = { f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0] };
        const double u[3] = { s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0] };
        double m[16] = { 0 };
        m[15] = 1;
        for (int k = 0; k < 3; ++k) { m[k * 4 + 0] = s[k]; m[k * 4 + 1] = u[k]; m[k * 4 + 2] = -f[k]; }
        m[12] = -((s[0] * eye[0] + s[1] * eye[1]) + s[2] * eye[2]);
        m[13] = -((u[0] * eye[0] + u[1] * eye[1]) + u[2] * eye[2]);
        m[14] = (f[0] * eye[0] + f[1] * eye[1]) + f[2] * eye[2];
        for (int k = 0; k < 16; ++k) views[fc * 16 + k] = (float)(m[k] + 0.0);      // (+ 0.0: no negative zeros in the matrix)
    }
    const double n = near_p, f = far_p;
    for (int k = 0; k < 16; ++k) proj[k] = 0.0f;
    proj[0] = 1.0f;
    proj[5] = 1.0f;
    proj[10] = (float)(-(f + n) / (f - n));
    proj[11] = -1.0f;
    proj[14] = (float)(-(2.0 * f * n) / (f - n));
}

m2s_status check_light(m2s_ctx* c, const m2s_light_params* lp, int* S_out) {
    const int64_t S = lp->shadow_resolution ? (int64_t)lp->shadow_resolution : 1024;
    if (S < 1 || S > 4096) return fail(c, M2S_ERR_INVALID, "shadow resolution outside 1..4096");
    if (lp->render_mode < 0 || lp->render_mode > 6 || lp->reserved != 0) return fail(c, M2S_ERR_INVALID, "render mode outside 0..6 or reserved != 0");
    *S_out = (int)S;
    return M2S_OK;
}

// Stage B over `total` quads in c->d_shadow_quads (the six lists back to back, fb: where each starts) into the cleared cube.
m2s_status shadow_stage_b(m2s_ctx* c, const m2s_light_params* lp, int S, uint32_t total, const ShadowBases& fb, uint64_t* out_skipped, float* b_ms,
                          float* r_ms) {
    ClockOf<ShadowMark>& clock = c->shadow_clock;      // (opened by the caller)
    // ---- stage B: setup, the number of (tile, quad) pairs read back once (the pair buffers are sized from it)
    BinWork& w = c->shadow_work;
    M2S_TRY(w.reserve_items(c->err, total, 48));
    M2S_TRY(w.reserve_temp(c->err, shadow_temp_bytes(1, total, 1)));
    const float4* rec = (const float4*)w.rec.get();
    HIPCHK(c, clock.mark(ShadowMark::Setup, c->stream));
    HIPCHK(c, shadow_setup(c->d_shadow_quads, total, fb, S, lp->light_position, lp->near_far[1], (float4*)w.rec.get(), w.cnt, w.off, w.temp,
                           w.temp.cap(), w.d_totals, c->stream));
    HIPCHK(c, clock.mark(ShadowMark::SetupEnd, c->stream));
    HIPCHK(c, hipMemcpyAsync(w.h_totals, w.d_totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t pairs = w.h_totals[0];
    c->last_shadow_counts[8] = w.h_totals[1];
    if (out_skipped) *out_skipped = w.h_totals[1];
    if (pairs > 0x7FFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^31-1 (tile, quad) pairs");
    if (pairs) {
        BinWork::Pairs pr;
        M2S_TRY(w.reserve_pairs(c->err, pairs, &pr));
        M2S_TRY(w.reserve_temp(c->err, shadow_temp_bytes(1, 1, (uint32_t)pairs)));
        HIPCHK(c, clock.mark(ShadowMark::Bin, c->stream));
        HIPCHK(c, shadow_bin(rec, w.cnt, w.off, total, S, pr.keys_in, pr.vals_in, pr.keys_out, pr.vals_out, (uint32_t)pairs, w.temp, w.temp.cap(),
                             c->stream));
        HIPCHK(c, clock.mark(ShadowMark::Binned, c->stream));
        HIPCHK(c, shadow_raster(rec, pr.keys_out, pr.vals_out, (uint32_t)pairs, S, c->d_shadow_cube, w.d_totals + 2, c->stream));
        HIPCHK(c, clock.mark(ShadowMark::Rastered, c->stream));
        HIPCHK(c, hipMemcpyAsync(w.h_totals + 2, w.d_totals + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->last_shadow_counts[6] = pairs;
        c->last_shadow_counts[7] = w.h_totals[2];
    }
    float x = 0, y = 0, z = 0;                         // (0 where the stage did not run, or the clock is off)
    HIPCHK(c, clock.span(ShadowMark::Bin, ShadowMark::Binned, &x));
    HIPCHK(c, clock.span(ShadowMark::Binned, ShadowMark::Rastered, &y));
    HIPCHK(c, clock.span(ShadowMark::Setup, ShadowMark::SetupEnd, &z));
    *b_ms += x; *r_ms += y;
    *b_ms += z;
    return M2S_OK;
}

}  // namespace

extern "C" {

// GaussianShadowPass::execute: the compute prepass through the six cameras of the light, then the six depth-only draws.
m2s_status m2s_shadow(m2s_ctx* c, const m2s_prepass_params* pp, const m2s_light_params* lp, const void* d_records, uint64_t n,
                      uint64_t out_per_face[6], uint64_t* out_skipped) {
    if (!c || !pp || !lp) return M2S_ERR_INVALID;
    if (c->slot_count) return fail(c, M2S_ERR_STATE, kInFlightMsg);
    int S = 0;
    if (m2s_status s = check_light(c, lp, &S)) return s;
    M2S_TRY(check_resolution(c, pp->resolution[0], pp->resolution[1], "renderer resolution"));
    if (pp->resolution_target == 0) return fail(c, M2S_ERR_INVALID, "resolution_target is 0");
    M2S_TRY(pick_records(c, d_records, n));
    HIPCHK(c, hipSetDevice(c->device));
    if (m2s_status s = ensure_light_common(c)) return s;
    if (out_per_face) for (int f = 0; f < 6; ++f) out_per_face[f] = 0;
    if (out_skipped) *out_skipped = 0;
    c->shadow_S = 0;
    c->shadow_lists = false;
    for (uint32_t& b : c->shadow_base) b = 0;
    for (uint64_t& v : c->last_shadow_counts) v = 0;
    const uint64_t texels = 6ull * (uint64_t)S * (uint64_t)S;
    M2S_TRY(c->d_shadow_cube.reserve(c->err, texels, sizeof(float)));
    ClockOf<ShadowMark>& clock = c->shadow_clock;
    M2S_TRY(clock.begin(c->err, c->profiling));
    HIPCHK(c, shadow_clear(c->d_shadow_cube, S, c->stream));                      // glClear(GL_DEPTH_BUFFER_BIT), six times
    HIPCHK(c, hipMemsetAsync(c->shadow_work.d_totals, 0, 4 * sizeof(unsigned long long), c->stream));
    const uint32_t nr = (uint32_t)n;
    uint32_t total = 0;
    float a_ms = 0, b_ms = 0, r_ms = 0;
    if (nr) {
        // ---- stage A
        PrepassK k;
        prepass_prepare(*pp, n, &k);
        BinWork& w = c->shadow_work;
        float* h_views = reinterpret_cast<float*>(w.h_totals + kPinnedViews);
        shadow_cameras(lp->light_position, lp->near_far[0], lp->near_far[1], h_views, k.P);
        const uint32_t nb = shadow_blocks(nr);
        const uint64_t words = 6ull * nb + 1;
        M2S_TRY(c->d_sh_tab.reserve(c->err, words, 2 * sizeof(uint32_t)));
        uint32_t* cnt = c->d_sh_tab;
        uint32_t* off = c->d_sh_tab + c->d_sh_tab.cap();
        M2S_TRY(w.reserve_temp(c->err, shadow_temp_bytes((uint32_t)words, 1, 1)));
        uint32_t* d_bases = reinterpret_cast<uint32_t*>(c->d_sh_views + 96);
        HIPCHK(c, hipMemcpyAsync(c->d_sh_views, h_views, 96 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, clock.mark(ShadowMark::Count, c->stream));
        HIPCHK(c, shadow_count(k, c->d_sh_views, lp->light_position, (const float4*)d_records, nr, cnt, off, w.temp, w.temp.cap(), d_bases, c->stream));
        HIPCHK(c, clock.mark(ShadowMark::Counted, c->stream));
        uint32_t* h_bases = reinterpret_cast<uint32_t*>(w.h_totals + kPinnedBases);
        HIPCHK(c, hipMemcpyAsync(h_bases, d_bases, 7 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        total = h_bases[6];
        ShadowBases fb;
        for (int f = 0; f < 7; ++f) fb.b[f] = h_bases[f];
        if (total) {
            M2S_TRY(c->d_shadow_quads.reserve(c->err, total, 48));
            HIPCHK(c, clock.mark(ShadowMark::Emit, c->stream));
            HIPCHK(c, shadow_emit(k, c->d_sh_views, lp->light_position, (const float4*)d_records, nr, off, c->d_shadow_quads, c->stream));
            HIPCHK(c, clock.mark(ShadowMark::Emitted, c->stream));
            if (m2s_status st = shadow_stage_b(c, lp, S, total, fb, out_skipped, &b_ms, &r_ms)) return st;
        }
        float x = 0, y = 0;
        HIPCHK(c, clock.span(ShadowMark::Emit, ShadowMark::Emitted, &x));
        HIPCHK(c, clock.span(ShadowMark::Count, ShadowMark::Counted, &y));
        a_ms += x;
        a_ms += y;
        for (int f = 0; f < 7; ++f) c->shadow_base[f] = fb.b[f];
        for (int f = 0; f < 6; ++f) {
            c->last_shadow_counts[f] = fb.b[f + 1] - fb.b[f];
            if (out_per_face) out_per_face[f] = c->last_shadow_counts[f];
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (clock.on()) {
        c->last_shadow_stage_ms[0] = a_ms; c->last_shadow_stage_ms[1] = b_ms; c->last_shadow_stage_ms[2] = r_ms;
        c->last_shadow_ms = a_ms + b_ms + r_ms;
    }
    c->shadow_S = S;
    c->shadow_lists = true;
    return M2S_OK;
}

// Stage B alone on quad lists made elsewhere: the counterpart of m2s_upload_quads + m2s_splat for the shadow pass.
m2s_status m2s_shadow_from_quads(m2s_ctx* c, const m2s_light_params* lp, const m2s_shadow_quad* host_quads, const uint64_t per_face[6],
                                 uint64_t* out_skipped) {
    if (!c || !lp || !per_face) return M2S_ERR_INVALID;
    int S = 0;
    if (m2s_status s = check_light(c, lp, &S)) return s;
    uint64_t total = 0;
    ShadowBases fb;
    for (int f = 0; f < 6; ++f) {
        if (per_face[f] > 0xFFFFFFFFull || total + per_face[f] > 0xFFFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^32-1 quads");
        fb.b[f] = (uint32_t)total;
        total += per_face[f];
    }
    fb.b[6] = (uint32_t)total;
    if (total && !host_quads) return fail(c, M2S_ERR_INVALID, "host_quads is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    if (m2s_status s = ensure_light_common(c)) return s;
    if (out_skipped) *out_skipped = 0;
    c->shadow_S = 0;
    c->shadow_lists = false;
    for (uint32_t& b : c->shadow_base) b = 0;
    for (uint64_t& v : c->last_shadow_counts) v = 0;
    M2S_TRY(c->d_shadow_cube.reserve(c->err, 6ull * (uint64_t)S * (uint64_t)S, sizeof(float)));
    M2S_TRY(c->shadow_clock.begin(c->err, c->profiling));
    HIPCHK(c, shadow_clear(c->d_shadow_cube, S, c->stream));
    HIPCHK(c, hipMemsetAsync(c->shadow_work.d_totals, 0, 4 * sizeof(unsigned long long), c->stream));
    float b_ms = 0, r_ms = 0;
    if (total) {
        M2S_TRY(c->d_shadow_quads.reserve(c->err, total, 48));
        HIPCHK(c, hipMemcpyAsync(c->d_shadow_quads, host_quads, total * 48, hipMemcpyHostToDevice, c->stream));
        if (m2s_status s = shadow_stage_b(c, lp, S, (uint32_t)total, fb, out_skipped, &b_ms, &r_ms)) return s;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->shadow_clock.on()) {
        c->last_shadow_stage_ms[0] = 0; c->last_shadow_stage_ms[1] = b_ms; c->last_shadow_stage_ms[2] = r_ms;
        c->last_shadow_ms = b_ms + r_ms;
    }
    for (int f = 0; f < 7; ++f) c->shadow_base[f] = fb.b[f];
    for (int f = 0; f < 6; ++f) c->last_shadow_counts[f] = per_face[f];
    c->shadow_S = S;
    c->shadow_lists = true;
    return M2S_OK;
}

const void* m2s_device_shadow_cubemap(const m2s_ctx* c) { return c && c->shadow_S ? c->d_shadow_cube.get() : nullptr; }

m2s_status m2s_download_shadow_cubemap(m2s_ctx* c, float* dst, uint64_t capacity_floats) {
    if (!c || !dst) return M2S_ERR_INVALID;
    if (!c->shadow_S) return fail(c, M2S_ERR_STATE, "no shadow cube exists");
    const uint64_t texels = 6ull * (uint64_t)c->shadow_S * (uint64_t)c->shadow_S;
    if (capacity_floats < texels) return fail(c, M2S_ERR_CAPACITY, "destination smaller than the cube");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_shadow_cube, texels * sizeof(float), hipMemcpyDeviceToHost));
    return M2S_OK;
}

m2s_status m2s_download_shadow_quads(m2s_ctx* c, uint32_t face, m2s_shadow_quad* dst, uint64_t capacity) {
    if (!c || face >= 6) return M2S_ERR_INVALID;
    if (!c->shadow_lists) return fail(c, M2S_ERR_STATE, "no shadow pass has run");
    const uint64_t first = c->shadow_base[face], cnt = c->shadow_base[face + 1] - first;
    if (!cnt) return M2S_OK;
    if (!dst) return fail(c, M2S_ERR_INVALID, "dst is NULL");
    if (capacity < cnt) return fail(c, M2S_ERR_CAPACITY, "dst holds fewer quads than the face's list");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, (const char*)c->d_shadow_quads.get() + first * 48, cnt * 48, hipMemcpyDeviceToHost));
    return M2S_OK;
}

m2s_status m2s_upload_shadow_cubemap(m2s_ctx* c, const float* host, uint32_t S) {
    if (!c || !host) return M2S_ERR_INVALID;
    if (S < 1 || S > 4096) return fail(c, M2S_ERR_INVALID, "shadow resolution outside 1..4096");
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t texels = 6ull * S * S;
    c->shadow_S = 0;
    c->shadow_lists = false;
    M2S_TRY(c->d_shadow_cube.reserve(c->err, texels, sizeof(float)));
    HIPCHK(c, hipMemcpy(c->d_shadow_cube, host, texels * sizeof(float), hipMemcpyHostToDevice));
    c->shadow_S = (int32_t)S;
    return M2S_OK;
}

m2s_status m2s_upload_gbuffer(m2s_ctx* c, const void* const planes[5], int32_t W, int32_t H) {
    if (!c || !planes) return M2S_ERR_INVALID;
    M2S_TRY(check_resolution(c, W, H));
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t px = (uint64_t)W * (uint64_t)H;
    c->gbuf_w = c->gbuf_h = 0;
    M2S_TRY(c->d_gbuf.reserve(c->err, px));
    for (int k = 0; k < 5; ++k) {
        const size_t bytes = px * ((k == 2 || k == 4) ? 4 : 8);
        if (planes[k]) HIPCHK(c, hipMemcpy(c->d_gbuf.ptr[k], planes[k], bytes, hipMemcpyHostToDevice));
        else HIPCHK(c, hipMemset(c->d_gbuf.ptr[k], 0, bytes));
    }
    c->gbuf_w = W;
    c->gbuf_h = H;
    return M2S_OK;
}

// GaussianRelightingPass::execute: one full-screen draw of gaussianSplattingDeferredPS.glsl; split: the branch with the split screen.
static m2s_status relight_checks(m2s_ctx* c, const m2s_light_params* lp, int32_t gw, int32_t gh) {
    int S = 0;
    if (m2s_status s = check_light(c, lp, &S)) return s;
    if (!gw) return fail(c, M2S_ERR_INVALID, "no G-buffer exists (run m2s_splat or m2s_upload_gbuffer)");
    if (!c->shadow_S) return fail(c, M2S_ERR_INVALID, "no shadow cube exists (run m2s_shadow or m2s_upload_shadow_cubemap)");
    if (lp->resolution[0] != gw || lp->resolution[1] != gh) return fail(c, M2S_ERR_INVALID, "resolution is not the G-buffer's");
    if (lp->shadow_resolution && (int32_t)lp->shadow_resolution != c->shadow_S) return fail(c, M2S_ERR_INVALID, "shadow resolution is not the cube's");
    return M2S_OK;
}

static RelightK relight_uniforms(const m2s_ctx* c, const m2s_light_params* lp, int32_t W, int32_t H) {
    RelightK k;
    for (int i = 0; i < 3; ++i) { k.light[i] = lp->light_position[i]; k.cam[i] = lp->camera_position[i]; k.color[i] = lp->light_color[i]; }
    k.intensity = lp->light_intensity;
    k.far_plane = lp->near_far[1];
    k.mode = lp->render_mode;
    k.W = W; k.H = H; k.S = c->shadow_S;
    return k;
}

static m2s_status relight(m2s_ctx* c, const m2s_light_params* lp, bool split, float split_position) {
    if (!c || !lp) return M2S_ERR_INVALID;
    if (split && !(split_position >= 0.0f && split_position <= 1.0f)) return fail(c, M2S_ERR_INVALID, "split position outside 0..1");
    if (m2s_status s = relight_checks(c, lp, c->gbuf_w, c->gbuf_h)) return s;
    if (split && (c->mr_w != c->gbuf_w || c->mr_h != c->gbuf_h)) return fail(c, M2S_ERR_STATE, "no mesh G-buffer of the G-buffer's resolution exists (run m2s_mesh_render)");
    HIPCHK(c, hipSetDevice(c->device));
    if (m2s_status s = ensure_light_common(c)) return s;
    const uint64_t px = (uint64_t)c->gbuf_w * (uint64_t)c->gbuf_h;
    c->frame_w = c->frame_h = 0;
    c->frame_has_counts = false;
    M2S_TRY(c->d_frame.reserve(c->err, px, 4));
    M2S_TRY(c->d_shadow_counts.reserve(c->err, px, 1));
    const RelightK k = relight_uniforms(c, lp, c->gbuf_w, c->gbuf_h);
    const bool counts = lp->want_shadow_counts != 0 && lp->render_mode == 6;
    M2S_TRY(c->relight_clock.begin(c->err, c->profiling));
    HIPCHK(c, c->relight_clock.mark(SpanMark::Begin, c->stream));
    const int split_x = split ? (int)(split_position * (float)c->gbuf_w) : 0;      // static_cast<int>(splitScreenPosition * w)
    const int div_x = std::max(0, split_x - 1);                                      // dividerWidth / 2 == 1
    HIPCHK(c, launch_relight(k, c->d_gbuf.ptr, c->d_shadow_cube, c->d_frame, counts ? c->d_shadow_counts.get() : nullptr, c->stream,
                             split ? c->d_mr_gbuf.ptr : nullptr, split_x, div_x));
    HIPCHK(c, c->relight_clock.mark(SpanMark::End, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->relight_clock.on()) HIPCHK(c, c->relight_clock.span(SpanMark::Begin, SpanMark::End, &c->last_relight_ms));
    c->frame_w = c->gbuf_w;
    c->frame_h = c->gbuf_h;
    c->frame_has_counts = counts;
    return M2S_OK;
}

m2s_status m2s_relight(m2s_ctx* c, const m2s_light_params* lp) { return relight(c, lp, false, 0.0f); }
m2s_status m2s_relight_split(m2s_ctx* c, const m2s_light_params* lp, float split_position) { return relight(c, lp, true, split_position); }

// The same draw over the MESH G-buffer, every pixel, into the second frame buffer: the reference image of m2s_score_frames.  The
// frame and the shadow counts of m2s_relight are not touched.
m2s_status m2s_relight_mesh(m2s_ctx* c, const m2s_light_params* lp) {
    if (!c || !lp) return M2S_ERR_INVALID;
    if (!c->mr_w) return fail(c, M2S_ERR_STATE, "no mesh G-buffer exists (run m2s_mesh_render)");
    if (m2s_status s = relight_checks(c, lp, c->mr_w, c->mr_h)) return s;
    HIPCHK(c, hipSetDevice(c->device));
    if (m2s_status s = ensure_light_common(c)) return s;
    c->mesh_frame_w = c->mesh_frame_h = 0;
    M2S_TRY(c->d_mesh_frame.reserve(c->err, (uint64_t)c->mr_w * (uint64_t)c->mr_h, 4));
    const RelightK k = relight_uniforms(c, lp, c->mr_w, c->mr_h);
    M2S_TRY(c->relight_clock.begin(c->err, c->profiling));
    HIPCHK(c, c->relight_clock.mark(SpanMark::Begin, c->stream));
    HIPCHK(c, launch_relight(k, c->d_mr_gbuf.ptr, c->d_shadow_cube, c->d_mesh_frame, nullptr, c->stream));
    HIPCHK(c, c->relight_clock.mark(SpanMark::End, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->relight_clock.on()) HIPCHK(c, c->relight_clock.span(SpanMark::Begin, SpanMark::End, &c->last_relight_ms));
    c->mesh_frame_w = c->mr_w;
    c->mesh_frame_h = c->mr_h;
    return M2S_OK;
}

const void* m2s_device_frame(const m2s_ctx* c) { return c && c->frame_w ? c->d_frame.get() : nullptr; }

m2s_status m2s_download_frame(m2s_ctx* c, void* dst, uint64_t capacity_bytes) {
    if (!c || !dst) return M2S_ERR_INVALID;
    if (!c->frame_w) return fail(c, M2S_ERR_STATE, "no relight has run");
    const uint64_t bytes = (uint64_t)c->frame_w * (uint64_t)c->frame_h * 4;
    if (capacity_bytes < bytes) return fail(c, M2S_ERR_CAPACITY, "destination smaller than the frame");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_frame, bytes, hipMemcpyDeviceToHost));
    return M2S_OK;
}

const void* m2s_device_mesh_frame(const m2s_ctx* c) { return c && c->mesh_frame_w ? c->d_mesh_frame.get() : nullptr; }

m2s_status m2s_download_mesh_frame(m2s_ctx* c, void* dst, uint64_t capacity_bytes) {
    if (!c || !dst) return M2S_ERR_INVALID;
    if (!c->mesh_frame_w) return fail(c, M2S_ERR_STATE, "no m2s_relight_mesh has run");
    const uint64_t bytes = (uint64_t)c->mesh_frame_w * (uint64_t)c->mesh_frame_h * 4;
    if (capacity_bytes < bytes) return fail(c, M2S_ERR_CAPACITY, "destination smaller than the frame");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_mesh_frame, bytes, hipMemcpyDeviceToHost));
    return M2S_OK;
}

m2s_status m2s_download_shadow_counts(m2s_ctx* c, uint8_t* dst, uint64_t capacity_bytes) {
    if (!c || !dst) return M2S_ERR_INVALID;
    if (!c->frame_w || !c->frame_has_counts) return fail(c, M2S_ERR_STATE, "the last relight kept no shadow counts (want_shadow_counts, render mode 6)");
    const uint64_t bytes = (uint64_t)c->frame_w * (uint64_t)c->frame_h;
    if (capacity_bytes < bytes) return fail(c, M2S_ERR_CAPACITY, "destination smaller than the plane");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_shadow_counts, bytes, hipMemcpyDeviceToHost));
    return M2S_OK;
}

float m2s_last_shadow_ms(const m2s_ctx* c) { return c ? c->last_shadow_ms : 0.0f; }
m2s_status m2s_last_shadow_stage_ms(const m2s_ctx* c, float out_ms[3]) { return get_array(c, &m2s_ctx::last_shadow_stage_ms, out_ms); }
m2s_status m2s_last_shadow_counts(const m2s_ctx* c, uint64_t out[9]) { return get_array(c, &m2s_ctx::last_shadow_counts, out); }
float m2s_last_relight_ms(const m2s_ctx* c) { return c ? c->last_relight_ms : 0.0f; }

}  // extern "C"
