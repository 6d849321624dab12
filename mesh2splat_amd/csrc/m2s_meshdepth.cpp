// m2s_meshdepth.cpp — the mesh depth prepass (DepthPrepass.cpp:8-50): host side of m2s_meshdepth.hip; the stages it shares with the
// visibility stage of the mesh render pass (mesh_raster; m2s_meshrender.cpp).
#include "m2s_ctx.h"

#include <algorithm>
#include <cstring>

using namespace m2s;
using namespace m2s_host;

namespace {

// glm's mat4 * mat4 (type_mat4x4.inl): column j of the result = ((A[0] b0 + A[1] b1) + A[2] b2) + A[3] b3 with b = column j of B,
// every operation rounded to fp32 (this file is compiled without contraction)
void mat4_mul(const float* A, const float* B, float* R) {
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i)
            R[j * 4 + i] = ((A[0 + i] * B[j * 4 + 0] + A[4 + i] * B[j * 4 + 1]) + A[8 + i] * B[j * 4 + 2]) + A[12 + i] * B[j * 4 + 3];
}

}  // namespace

namespace m2s_host {

void mesh_pvm(const float* proj, const float* view, const float* model, float* out) {
    float pv[16];
    mat4_mul(proj, view, pv);          // GLSL multiplies left to right: (P V) M
    mat4_mul(pv, model, out);
}

m2s_status mesh_raster(m2s_ctx* c, const MeshDepthK& k, bool vis, void* image, float ms[3]) {
    BinWork& w = c->md_work;
    M2S_TRY(w.reserve_totals(c->err, 8, 8 * sizeof(unsigned long long)));
    ClockOf<MeshMark>& clock = c->md_clock;
    M2S_TRY(clock.begin(c->err, c->profiling));
    unsigned long long* const h_md = w.h_totals;
    for (int i = 0; i < 8; ++i) h_md[i] = 0;
    ms[0] = ms[1] = ms[2] = 0.0f;
    const int W = k.W, H = k.H;
    const uint32_t n = c->scene.n_tri;
    M2S_TRY(c->d_md_deferred.reserve(c->err, std::max<uint64_t>(n, 1), sizeof(uint32_t)));
    HIPCHK(c, clock.mark(MeshMark::Start, c->stream));
    if (vis) HIPCHK(c, meshvis_clear((unsigned long long*)image, W, H, c->stream));
    else HIPCHK(c, meshdepth_clear((float*)image, W, H, c->stream));       // glClear(GL_DEPTH_BUFFER_BIT): part of the pass
    HIPCHK(c, hipMemsetAsync(w.d_totals, 0, 8 * sizeof(unsigned long long), c->stream));
    if (n) {
        if (vis) HIPCHK(c, meshvis_setup(k, c->scene, (unsigned long long*)image, c->d_md_deferred, w.d_totals, c->stream));
        else HIPCHK(c, meshdepth_setup(k, c->scene, (float*)image, c->d_md_deferred, w.d_totals, c->stream));
    }
    HIPCHK(c, clock.mark(MeshMark::SetupEnd, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_md, w.d_totals, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t nd = h_md[5];
    uint64_t pairs = 0;
    if (nd) {
        const uint64_t slots = nd * kMdSlotsPerTriangle;
        M2S_TRY(w.reserve_items(c->err, slots, 48));
        M2S_TRY(w.reserve_temp(c->err, meshdepth_temp_bytes((uint32_t)slots, 1)));
        const float4* rec = (const float4*)w.rec.get();
        HIPCHK(c, clock.mark(MeshMark::Deferred, c->stream));
        HIPCHK(c, meshdepth_deferred(k, c->scene, c->d_md_deferred, (uint32_t)nd, (float4*)w.rec.get(), w.cnt, w.off, w.temp, w.temp.cap(), w.d_totals,
                                     c->stream, vis));
        HIPCHK(c, hipMemcpyAsync(h_md, w.d_totals, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        pairs = h_md[3];
        if (pairs > 0x7FFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^31-1 (tile, triangle) pairs");
        if (pairs) {
            BinWork::Pairs pr;
            M2S_TRY(w.reserve_pairs(c->err, pairs, &pr));
            M2S_TRY(w.reserve_temp(c->err, meshdepth_temp_bytes(1, (uint32_t)pairs)));
            HIPCHK(c, meshdepth_bin(k, rec, w.cnt, w.off, (uint32_t)nd, pr.keys_in, pr.vals_in, pr.keys_out, pr.vals_out, (uint32_t)pairs, w.temp,
                                    w.temp.cap(), c->stream));
            HIPCHK(c, clock.mark(MeshMark::Binned, c->stream));
            if (vis) HIPCHK(c, meshvis_raster(k, rec, pr.keys_out, pr.vals_out, (uint32_t)pairs, (unsigned long long*)image, w.d_totals, c->stream));
            else HIPCHK(c, meshdepth_raster(k, rec, pr.keys_out, pr.vals_out, (uint32_t)pairs, (float*)image, w.d_totals, c->stream));
            HIPCHK(c, clock.mark(MeshMark::Rastered, c->stream));
            HIPCHK(c, hipMemcpyAsync(h_md, w.d_totals, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        } else if (clock.on()) {   // deferred triangles without pairs: the clipper ran, its span is closed here
            HIPCHK(c, clock.mark(MeshMark::Binned, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    // (nothing deferred: [1] and [2] are 0; no pairs: [2] is)
    HIPCHK(c, clock.span(MeshMark::Start, MeshMark::SetupEnd, &ms[0]));
    HIPCHK(c, clock.span(MeshMark::Deferred, MeshMark::Binned, &ms[1]));
    HIPCHK(c, clock.span(MeshMark::Binned, MeshMark::Rastered, &ms[2]));
    return M2S_OK;
}

}  // namespace m2s_host

extern "C" {

// DepthPrepass::execute: the opaque meshes through the frame's camera, depth only, GL_LESS, into a cleared image.
m2s_status m2s_mesh_depth(m2s_ctx* c, const m2s_mesh_depth_params* p, uint64_t out_counts[5]) {
    if (!c || !p) return M2S_ERR_INVALID;
    const int W = p->resolution[0], H = p->resolution[1];
    M2S_TRY(check_resolution(c, W, H));
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(c, M2S_ERR_INVALID, "reserved != 0");
    if (!c->has_scene) return fail(c, M2S_ERR_STATE, "no scene has been uploaded");
    HIPCHK(c, hipSetDevice(c->device));
    c->md_w = c->md_h = 0;
    for (uint64_t& v : c->last_md_counts) v = 0;
    if (out_counts) for (int k = 0; k < 5; ++k) out_counts[k] = 0;
    MeshDepthK k;
    mesh_pvm(p->view_to_clip, p->world_to_view, p->model_to_world, k.PVM);
    k.W = W; k.H = H;
    k.inplace = c->md_inplace < 0 ? kMdInplace : c->md_inplace;
    M2S_TRY(c->d_md_image.reserve(c->err, (uint64_t)W * (uint64_t)H, sizeof(float)));
    float ms[3] = { 0, 0, 0 };
    if (m2s_status s = mesh_raster(c, k, false, c->d_md_image, ms)) return s;
    if (c->profiling) {
        std::memcpy(c->last_md_stage_ms, ms, sizeof ms);
        c->last_md_ms = ms[0] + ms[1] + ms[2];
    }
    for (int i = 0; i < 5; ++i) c->last_md_counts[i] = c->md_work.h_totals[i];
    if (out_counts) for (int i = 0; i < 5; ++i) out_counts[i] = c->last_md_counts[i];
    c->md_w = W;
    c->md_h = H;
    return M2S_OK;
}

const void* m2s_device_mesh_depth(const m2s_ctx* c) { return c && c->md_w ? c->d_md_image.get() : nullptr; }

m2s_status m2s_download_mesh_depth(m2s_ctx* c, float* dst, uint64_t capacity_floats) {
    if (!c || !dst) return M2S_ERR_INVALID;
    if (!c->md_w) return fail(c, M2S_ERR_STATE, "no mesh depth image exists");
    const uint64_t texels = (uint64_t)c->md_w * (uint64_t)c->md_h;
    if (capacity_floats < texels) return fail(c, M2S_ERR_CAPACITY, "destination smaller than the image");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_md_image, texels * sizeof(float), hipMemcpyDeviceToHost));
    return M2S_OK;
}

float m2s_last_mesh_depth_ms(const m2s_ctx* c) { return c ? c->last_md_ms : 0.0f; }
m2s_status m2s_last_mesh_depth_stage_ms(const m2s_ctx* c, float out_ms[3]) { return get_array(c, &m2s_ctx::last_md_stage_ms, out_ms); }
m2s_status m2s_last_mesh_depth_counts(const m2s_ctx* c, uint64_t out[5]) { return get_array(c, &m2s_ctx::last_md_counts, out); }

m2s_status m2s_debug_set_mesh_depth_inplace(m2s_ctx* c, int32_t max_box) {
    if (!c) return M2S_ERR_INVALID;
    if (max_box < -1 || max_box > 8192) return fail(c, M2S_ERR_INVALID, "max_box outside -1..8192");
    c->md_inplace = max_box;
    return M2S_OK;
}

}  // extern "C"
