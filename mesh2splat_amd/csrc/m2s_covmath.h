// m2s_covmath.h — the covariance arithmetic the viewer's two per-Gaussian compute shaders share: gaussianSplattingPrepassCS.glsl:94-110,
// :154-190 (k_prepass, m2s_prepass.hip) and the same lines of gaussianPointShadowMappingCS.glsl:96-112, :160-196 (k_shadow_quads,
// m2s_light.hip: the prepass seen from the six cameras of the light).  fp32, the shader's operation order, one rounding per operation.
// One definition, so that the shadow pass sizes and culls a Gaussian exactly as the prepass would through the same camera.
#pragma once
#include "m2s_device.h"

#pragma clang fp contract(off)

namespace m2s {

struct M3 { float c[3][3]; };   // c[col][row], like the shader's mat3

// mat3 * mat3 in the shader's (glm's) association: a0r*b_c0 + a1r*b_c1 + a2r*b_c2, left to right
__device__ __forceinline__ M3 m3_mul(const M3& a, const M3& b) {
    M3 r;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 3; ++i) r.c[c][i] = a.c[0][i] * b.c[c][0] + a.c[1][i] * b.c[c][1] + a.c[2][i] * b.c[c][2];
    return r;
}
__device__ __forceinline__ M3 m3_transpose(const M3& a) {
    M3 r;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 3; ++i) r.c[c][i] = a.c[i][c];
    return r;
}
__device__ __forceinline__ float min_glsl(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float max_glsl(float a, float b) { return (a < b) ? b : a; }

// :94-110  scale (u_stdDev, the model scale as written), castQuatToMat3 * inverse(mat3(u_modelToWorld)), computeCov3D.
// rot: the rotation matrix after :102-108 (the prepass takes a format-1 normal from it).
__device__ __forceinline__ M3 gaussian_cov3d(const PrepassK& k, float4 gscl, float4 grot, M3& rot) {
    const float multiplier = (k.format == 0u || k.format == 3u) ? k.std_dev : 1.0f;   // :94
    // :95-96  modelScale = (|M[0]|, |M[0]|, |M[1]|) as written; k.ms2 = its square (uniform, prepared on the host)
    const float scale[3] = { (gscl.x * multiplier) * k.ms2[0], (gscl.y * multiplier) * k.ms2[1], (gscl.z * multiplier) * k.ms2[2] };

    // :100  castQuatToMat3 on the stored vec4
    {
        const float x = grot.x, y = grot.y, z = grot.z, w = grot.w;
        rot.c[0][0] = 1.f - 2.f * (z * z + w * w);
        rot.c[0][1] = 2.f * (y * z - x * w);
        rot.c[0][2] = 2.f * (y * w + x * z);
        rot.c[1][0] = 2.f * (y * z + x * w);
        rot.c[1][1] = 1.f - 2.f * (y * y + w * w);
        rot.c[1][2] = 2.f * (z * w - x * y);
        rot.c[2][0] = 2.f * (y * w - x * z);
        rot.c[2][1] = 2.f * (z * w + x * y);
        rot.c[2][2] = 1.f - 2.f * (y * y + z * z);
    }
    M3 mri;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 3; ++i) mri.c[c][i] = k.mr_inv[c * 3 + i];
    rot = m3_mul(rot, mri);                                                      // :102-108
    M3 cov3d;                                                                    // :110  computeCov3D
    {
        M3 sm;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 3; ++i) sm.c[c][i] = (c == i) ? scale[c] : 0.0f;
        const M3 mm = m3_mul(sm, rot);
        cov3d = m3_mul(m3_transpose(mm), mm);
    }

    return cov3d;
}

// What :154-190 leave behind: the 2 x 2 covariance with the 0.3 low-pass on its diagonal, its eigenvalues (the caller culls on
// lambda2 < 0, :183) and the two quad axes in NDC of a res[0] x res[1] window.
struct Cov2D { float c00, c01, c10, c11, lambda1, lambda2; float4 quad_scale; };
// V, P: u_worldToView (the camera's; the shadow pass: the face's) and u_viewToClip, column-major; vs: the view-space position.
__device__ __forceinline__ void project_cov(const float* V, const float* P, const float* res, const float* near_far, float4 vs, const M3& cov3d,
                                            Cov2D& o) {
    const float p00 = P[0], p11 = P[5], p32 = P[14];
    const float tz_sq = vs.z * vs.z;                                             // :154-159
    const float jsx = -(p00 * res[0]) / (2.0f * vs.z);
    const float jsy = -(p11 * res[1]) / (2.0f * vs.z);
    const float jtx = (p00 * vs.x * res[0]) / (2.0f * tz_sq);
    const float jty = (p11 * vs.y * res[1]) / (2.0f * tz_sq);
    const float jtz = ((near_far[1] - near_far[0]) * p32) / (2.0f * tz_sq);
    M3 J, W;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 3; ++i) { J.c[c][i] = 0.0f; W.c[c][i] = V[c * 4 + i]; }   // :161-165
    J.c[0][0] = jsx; J.c[1][1] = jsy; J.c[2][0] = jtx; J.c[2][1] = jty; J.c[2][2] = jtz;
    const M3 JW = m3_mul(J, W);
    const M3 Vp = m3_mul(m3_mul(JW, cov3d), m3_transpose(JW));                   // :168
    float c00 = Vp.c[0][0];
    const float c01 = Vp.c[0][1], c10 = Vp.c[1][0];
    float c11 = Vp.c[1][1];                                                      // :170
    c00 += 0.3f;                                                                 // :173-174
    c11 += 0.3f;
    const float mid = c00 + c11;
    const float da = c00 - c11, db = 2.0f * c01;
    const float delta = sqrtf(da * da + db * db);                                // :178
    const float lambda1 = 0.5f * (mid + delta), lambda2 = 0.5f * (mid - delta);

    const float dvy = (-c00 + c01 + lambda1) / (c01 - c11 + lambda1);            // :185
    const float inv_len = 1.0f / sqrtf(1.0f * 1.0f + dvy * dvy);
    const float dx = 1.0f * inv_len, dy = dvy * inv_len;
    const float major_r = min_glsl(3.0f * sqrtf(lambda1), 1024.0f), minor_r = min_glsl(3.0f * sqrtf(lambda2), 1024.0f);
    const float hx = res[0] * 0.5f, hy = res[1] * 0.5f;                      // :186-190
    o.quad_scale = make_float4((major_r * dx) / hx, (major_r * dy) / hy, (minor_r * dy) / hx, (minor_r * (-dx)) / hy);
    o.c00 = c00; o.c01 = c01; o.c10 = c10; o.c11 = c11; o.lambda1 = lambda1; o.lambda2 = lambda2;
}

}  // namespace m2s
