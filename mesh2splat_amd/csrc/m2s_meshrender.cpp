// m2s_meshrender.cpp — the mesh render pass (MeshRenderPass.cpp:8-73): host side of m2s_meshrender.hip.  The visibility stage runs
// through mesh_raster (m2s_meshdepth.cpp) with the mesh depth prepass's work buffers.
#include "m2s_ctx.h"

#include <algorithm>
#include <cstring>

using namespace m2s;
using namespace m2s_host;

namespace {

// mat3(transpose(inverse(M))) in float64 from the fp32 matrix (column-major), rounded to fp32: out[col * 3 + row].
// inverse = adjugate / det, so element (row r, col c) of the inverse's transpose is cofactor(r, c) / det.
void normal_matrix(const float* Mf, float* out) {
    double m[4][4];       // m[r][c]
    for (int c = 0; c < 4; ++c) for (int r = 0; r < 4; ++r) m[r][c] = (double)Mf[c * 4 + r];
    auto minor3 = [&](int rr, int cc) {
        int R[3], C[3];
        for (int i = 0, k = 0; i < 4; ++i) if (i != rr) R[k++] = i;
        for (int i = 0, k = 0; i < 4; ++i) if (i != cc) C[k++] = i;
        return m[R[0]][C[0]] * (m[R[1]][C[1]] * m[R[2]][C[2]] - m[R[1]][C[2]] * m[R[2]][C[1]])
             - m[R[0]][C[1]] * (m[R[1]][C[0]] * m[R[2]][C[2]] - m[R[1]][C[2]] * m[R[2]][C[0]])
             + m[R[0]][C[2]] * (m[R[1]][C[0]] * m[R[2]][C[1]] - m[R[1]][C[1]] * m[R[2]][C[0]]);
    };
    double cof[4][4], det = 0.0;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) cof[r][c] = (((r + c) & 1) ? -1.0 : 1.0) * minor3(r, c);
    for (int c = 0; c < 4; ++c) det += m[0][c] * cof[0][c];
    for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) out[c * 3 + r] = (float)(cof[r][c] / det);
}

}  // namespace

extern "C" {

// MeshRenderPass::execute: every mesh through the frame's camera, GL_LESS, back faces culled, into the mesh G-buffer.
m2s_status m2s_mesh_render(m2s_ctx* c, const m2s_mesh_render_params* p, uint64_t out_counts[6]) {
    if (!c || !p) return M2S_ERR_INVALID;
    const int W = p->resolution[0], H = p->resolution[1];
    M2S_TRY(check_resolution(c, W, H));
    if (p->render_mode < 0 || p->render_mode > 6) return fail(c, M2S_ERR_INVALID, "render mode outside 0..6");
    if (p->reserved != 0) return fail(c, M2S_ERR_INVALID, "reserved != 0");
    if (!c->has_scene) return fail(c, M2S_ERR_STATE, "no scene has been uploaded");
    HIPCHK(c, hipSetDevice(c->device));
    M2S_TRY(c->mr_clock.begin(c->err, c->profiling));
    c->mr_w = c->mr_h = 0;
    for (uint64_t& v : c->last_mr_counts) v = 0;
    if (out_counts) for (int k = 0; k < 6; ++k) out_counts[k] = 0;
    const uint64_t px = (uint64_t)W * (uint64_t)H;
    M2S_TRY(c->d_mr_vis.reserve(c->err, px, sizeof(unsigned long long)));
    M2S_TRY(c->d_mr_gbuf.reserve(c->err, px));
    MeshDepthK k;
    mesh_pvm(p->view_to_clip, p->world_to_view, p->model_to_world, k.PVM);      // the depth pass's transform: the two passes' depths agree bit for bit
    k.W = W; k.H = H;
    k.inplace = c->md_inplace < 0 ? kMdInplace : c->md_inplace;
    float ms[4] = { 0, 0, 0, 0 };
    if (m2s_status s = mesh_raster(c, k, true, c->d_mr_vis, ms)) return s;
    MeshRenderK r;
    std::memcpy(r.PVM, k.PVM, sizeof r.PVM);
    std::memcpy(r.M, p->model_to_world, sizeof r.M);
    std::memcpy(r.V, p->world_to_view, sizeof r.V);
    normal_matrix(p->model_to_world, r.N);
    r.near_far[0] = p->near_far[0]; r.near_far[1] = p->near_far[1];
    r.W = W; r.H = H; r.mode = p->render_mode;
    HIPCHK(c, c->mr_clock.mark(SpanMark::Begin, c->stream));
    HIPCHK(c, meshrender_shade(r, c->scene, c->d_mr_vis, c->d_mr_gbuf.ptr, c->stream));
    HIPCHK(c, c->mr_clock.mark(SpanMark::End, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->mr_clock.on()) {
        HIPCHK(c, c->mr_clock.span(SpanMark::Begin, SpanMark::End, &ms[3]));
        std::memcpy(c->last_mr_stage_ms, ms, sizeof ms);
        c->last_mr_ms = (ms[0] + ms[1]) + (ms[2] + ms[3]);
    }
    for (int i = 0; i < 5; ++i) c->last_mr_counts[i] = c->md_work.h_totals[i];
    c->last_mr_counts[5] = c->md_work.h_totals[6];
    if (out_counts) for (int i = 0; i < 6; ++i) out_counts[i] = c->last_mr_counts[i];
    c->mr_w = W;
    c->mr_h = H;
    return M2S_OK;
}

const void* m2s_device_mesh_gbuffer(const m2s_ctx* c, uint32_t attachment) { return c && c->mr_w && attachment < 5 ? c->d_mr_gbuf.ptr[attachment] : nullptr; }

m2s_status m2s_download_mesh_gbuffer(m2s_ctx* c, uint32_t attachment, void* dst, uint64_t capacity_bytes) {
    if (!c || !dst || attachment >= 5) return M2S_ERR_INVALID;
    if (!c->mr_w) return fail(c, M2S_ERR_STATE, "no mesh G-buffer exists");
    const uint64_t bytes = (uint64_t)c->mr_w * (uint64_t)c->mr_h * ((attachment == 2 || attachment == 4) ? 4 : 8);
    if (capacity_bytes < bytes) return fail(c, M2S_ERR_CAPACITY, "destination smaller than the plane");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_mr_gbuf.ptr[attachment], bytes, hipMemcpyDeviceToHost));
    return M2S_OK;
}

m2s_status m2s_download_mesh_visibility(m2s_ctx* c, uint64_t* dst, uint64_t capacity_pixels) {
    if (!c || !dst) return M2S_ERR_INVALID;
    if (!c->mr_w) return fail(c, M2S_ERR_STATE, "no mesh G-buffer exists");
    const uint64_t px = (uint64_t)c->mr_w * (uint64_t)c->mr_h;
    if (capacity_pixels < px) return fail(c, M2S_ERR_CAPACITY, "destination smaller than the image");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(dst, c->d_mr_vis, px * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return M2S_OK;
}

float m2s_last_mesh_render_ms(const m2s_ctx* c) { return c ? c->last_mr_ms : 0.0f; }
m2s_status m2s_last_mesh_render_stage_ms(const m2s_ctx* c, float out_ms[4]) { return get_array(c, &m2s_ctx::last_mr_stage_ms, out_ms); }
m2s_status m2s_last_mesh_render_counts(const m2s_ctx* c, uint64_t out[6]) { return get_array(c, &m2s_ctx::last_mr_counts, out); }

}  // extern "C"
