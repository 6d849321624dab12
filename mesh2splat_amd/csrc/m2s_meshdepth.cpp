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
    if (!c->h_md) HIPCHK(c, hipHostMalloc((void**)&c->h_md, 8 * sizeof(unsigned long long), hipHostMallocDefault));
    if (!c->d_md_totals) HIPCHK(c, hipMalloc((void**)&c->d_md_totals, 8 * sizeof(unsigned long long)));
    for (hipEvent_t& e : c->md_ev) if (!e) HIPCHK(c, hipEventCreate(&e));
    for (int i = 0; i < 8; ++i) c->h_md[i] = 0;
    ms[0] = ms[1] = ms[2] = 0.0f;
    const int W = k.W, H = k.H;
    const uint32_t n = c->scene.n_tri;
    if (m2s_status s = grow_buffer(c, c->d_md_deferred, c->md_tri_cap, std::max<uint64_t>(n, 1), sizeof(uint32_t))) return s;
    hipEvent_t* ev = c->md_ev;
    const bool prof = c->profiling;
    if (prof) HIPCHK(c, hipEventRecord(ev[0], c->stream));
    if (vis) HIPCHK(c, meshvis_clear((unsigned long long*)image, W, H, c->stream));
    else HIPCHK(c, meshdepth_clear((float*)image, W, H, c->stream));       // glClear(GL_DEPTH_BUFFER_BIT): part of the pass
    HIPCHK(c, hipMemsetAsync(c->d_md_totals, 0, 8 * sizeof(unsigned long long), c->stream));
    if (n) {
        if (vis) HIPCHK(c, meshvis_setup(k, c->scene, (unsigned long long*)image, c->d_md_deferred, c->d_md_totals, c->stream));
        else HIPCHK(c, meshdepth_setup(k, c->scene, (float*)image, c->d_md_deferred, c->d_md_totals, c->stream));
    }
    if (prof) HIPCHK(c, hipEventRecord(ev[1], c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_md, c->d_md_totals, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t nd = c->h_md[5];
    uint64_t pairs = 0;
    if (nd) {
        const uint64_t slots = nd * kMdSlotsPerTriangle;
        if (c->md_slot_cap < slots) {
            for (void* q : { c->d_md_rec, (void*)c->d_md_cnt, (void*)c->d_md_off }) if (q) (void)hipFree(q);
            c->d_md_rec = nullptr; c->d_md_cnt = nullptr; c->d_md_off = nullptr;
            c->md_slot_cap = 0;
            HIPCHK(c, hipMalloc(&c->d_md_rec, (size_t)slots * 48));
            HIPCHK(c, hipMalloc((void**)&c->d_md_cnt, (size_t)slots * sizeof(uint32_t)));
            HIPCHK(c, hipMalloc((void**)&c->d_md_off, (size_t)slots * sizeof(unsigned long long)));
            c->md_slot_cap = slots;
        }
        if (m2s_status s = grow_buffer(c, c->d_md_temp, c->md_temp_cap, meshdepth_temp_bytes((uint32_t)slots, 1), 1)) return s;
        if (prof) HIPCHK(c, hipEventRecord(ev[2], c->stream));
        HIPCHK(c, meshdepth_deferred(k, c->scene, c->d_md_deferred, (uint32_t)nd, (float4*)c->d_md_rec, c->d_md_cnt, c->d_md_off, c->d_md_temp,
                                     c->md_temp_cap, c->d_md_totals, c->stream, vis));
        HIPCHK(c, hipMemcpyAsync(c->h_md, c->d_md_totals, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        pairs = c->h_md[3];
        if (pairs > 0x7FFFFFFFull) return fail(c, M2S_ERR_CAPACITY, "more than 2^31-1 (tile, triangle) pairs");
        if (pairs) {
            if (m2s_status s = grow_buffer(c, c->d_md_pairs, c->md_pairs_cap, pairs, 4 * sizeof(uint32_t))) return s;
            if (m2s_status s = grow_buffer(c, c->d_md_temp, c->md_temp_cap, meshdepth_temp_bytes(1, (uint32_t)pairs), 1)) return s;
            const uint64_t pc = c->md_pairs_cap;
            uint32_t* keys_in = c->d_md_pairs;
            uint32_t* vals_in = keys_in + pc;
            uint32_t* keys_out = vals_in + pc;
            uint32_t* vals_out = keys_out + pc;
            HIPCHK(c, meshdepth_bin(k, (const float4*)c->d_md_rec, c->d_md_cnt, c->d_md_off, (uint32_t)nd, keys_in, vals_in, keys_out, vals_out, (uint32_t)pairs,
                                    c->d_md_temp, c->md_temp_cap, c->stream));
            if (prof) HIPCHK(c, hipEventRecord(ev[3], c->stream));
            if (vis) HIPCHK(c, meshvis_raster(k, (const float4*)c->d_md_rec, keys_out, vals_out, (uint32_t)pairs, (unsigned long long*)image, c->d_md_totals, c->stream));
            else HIPCHK(c, meshdepth_raster(k, (const float4*)c->d_md_rec, keys_out, vals_out, (uint32_t)pairs, (float*)image, c->d_md_totals, c->stream));
            if (prof) HIPCHK(c, hipEventRecord(ev[4], c->stream));
            HIPCHK(c, hipMemcpyAsync(c->h_md, c->d_md_totals, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (prof) {
                HIPCHK(c, hipEventElapsedTime(&ms[1], ev[2], ev[3]));
                HIPCHK(c, hipEventElapsedTime(&ms[2], ev[3], ev[4]));
            }
        } else if (prof) {
            HIPCHK(c, hipEventRecord(ev[3], c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipEventElapsedTime(&ms[1], ev[2], ev[3]));
        }
    }
    if (prof) HIPCHK(c, hipEventElapsedTime(&ms[0], ev[0], ev[1]));
    return M2S_OK;
}

}  // namespace m2s_host

extern "C" {

// DepthPrepass::execute: the opaque meshes through the frame's camera, depth only, GL_LESS, into a cleared image.
m2s_status m2s_mesh_depth(m2s_ctx* c, const m2s_mesh_depth_params* p, uint64_t out_counts[5]) {
    if (!c || !p) return M2S_ERR_INVALID;
    const int W = p->resolution[0], H = p->resolution[1];
    if (W < 1 || W > 8192 || H < 1 || H > 8192) return fail(c, M2S_ERR_INVALID, "resolution outside 1..8192");
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
    if (m2s_status s = grow_buffer(c, c->d_md_image, c->md_image_cap, (uint64_t)W * (uint64_t)H, sizeof(float))) return s;
    float ms[3] = { 0, 0, 0 };
    if (m2s_status s = mesh_raster(c, k, false, c->d_md_image, ms)) return s;
    if (c->profiling) {
        std::memcpy(c->last_md_stage_ms, ms, sizeof ms);
        c->last_md_ms = ms[0] + ms[1] + ms[2];
    }
    for (int i = 0; i < 5; ++i) c->last_md_counts[i] = c->h_md[i];
    if (out_counts) for (int i = 0; i < 5; ++i) out_counts[i] = c->last_md_counts[i];
    c->md_w = W;
    c->md_h = H;
    return M2S_OK;
}

const void* m2s_device_mesh_depth(const m2s_ctx* c) { return c && c->md_w ? c->d_md_image : nullptr; }

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
m2s_status m2s_last_mesh_depth_stage_ms(const m2s_ctx* c, float out_ms[3]) {
    if (!c || !out_ms) return M2S_ERR_INVALID;
    std::memcpy(out_ms, c->last_md_stage_ms, sizeof(c->last_md_stage_ms));
    return M2S_OK;
}
m2s_status m2s_last_mesh_depth_counts(const m2s_ctx* c, uint64_t out[5]) {
    if (!c || !out) return M2S_ERR_INVALID;
    for (int k = 0; k < 5; ++k) out[k] = c->last_md_counts[k];
    return M2S_OK;
}

m2s_status m2s_debug_set_mesh_depth_inplace(m2s_ctx* c, int32_t max_box) {
    if (!c) return M2S_ERR_INVALID;
    if (max_box < -1 || max_box > 8192) return fail(c, M2S_ERR_INVALID, "max_box outside -1..8192");
    c->md_inplace = max_box;
    return M2S_OK;
}

}  // extern "C"
