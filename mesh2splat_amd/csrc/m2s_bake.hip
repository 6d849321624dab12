// m2s_bake.hip — the point light baked into the spherical harmonics of the standard 3DGS .ply (m2s_bake_light, m2s_sh_shade_records;
// the pin is in include/m2s.h, tests/bake_ref.py restates it in numpy).
//   k_bake_sh    one lane per record: the deferred shader of k_relight (mode 6) with the Gaussian's own world position, normal, albedo,
//                roughness and metallic, evaluated for every view direction of a fixed quadrature table and projected onto the 16
//                harmonics.  Everything that does not depend on the view direction (albedo^2.2, L, n.l, attenuation, F0, the light
//                term of GeometrySmith, the 20 shadow taps) is computed once in front of the loop.  The loop counter is wave-uniform, so
//                the 20 floats of a direction (d, w, w B_0..15) arrive through scalar loads and sit in SGPRs; the 48 accumulators are
//                VGPRs.  The record's 48 coefficients leave through LDS (row stride 49 words: the per-lane column writes and the
//                row-major reads are both free of bank conflicts) as 16-byte non-temporal stores, consecutive lanes on consecutive
//                addresses: a wave writes its 12 KB in twelve 1 KB instructions.
//   k_sh_shade   one lane per record: a copy of the record whose colour is what a standard 3DGS viewer shows of the coefficients from
//                a camera position.
#include "m2s_device.h"
#include "m2s_devfn.h"
#include "m2s_lightmath.h"
#include "m2s_shbasis.h"
#include "m2s_viewmath.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr int kBakeLanes = 64;        // records per workgroup (one wave)
constexpr int kBakeStride = 49;       // LDS words per record: 48 coefficients + 1 (odd: lane l's word j lives in bank (49 l + j) mod 64)

__global__ void __launch_bounds__(kBakeLanes) k_bake_sh(const BakeK k, const float4* __restrict__ rec, uint32_t n, const float* __restrict__ tab,
                                                        const float* __restrict__ cube, float4* __restrict__ plane, uint8_t* __restrict__ counts) {
    __shared__ float s_out[kBakeLanes * kBakeStride];
    const uint32_t lane = threadIdx.x;
    const uint32_t first = blockIdx.x * (uint32_t)kBakeLanes;          // (n <= 2^32 - 1 and first < n: no overflow)
    const uint32_t i = first + lane;
    float acc[3][16];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[c][j] = 0.0f;
    if (lane < n - first) {
        const float4* g = rec + (size_t)i * 6;
        const float4 gpos = g[0], gcol = g[1], gnrm = g[3], gpbr = g[5];
        const float4 ws = m4_mul(k.M, gpos.x, gpos.y, gpos.z, 1.0f);                      // gaussianSplattingPrepassCS.glsl:67
        const float4 nw = m4_mul(k.MinvT, gnrm.x, gnrm.y, gnrm.z, 1.0f);                  // :119-120 (the vec4's w is 1, as written)
        float N0 = nw.x, N1 = nw.y, N2 = nw.z;
        normalize3(N0, N1, N2);
        // ---- the shadow factor, once per record: decision arithmetic
        uint32_t count = 0;
        if (k.use_shadows) count = shadow_taps(cube, k.S, ws.x, ws.y, ws.z, k.light[0], k.light[1], k.light[2], k.far_plane);
        if (counts) counts[i] = (uint8_t)count;
        const float shadow = (float)count / 20.0f;
        // ---- what does not depend on V (gaussianSplattingDeferredPS.glsl:130-164 in k_relight's order)
        const float roughness = gpbr.y, metallic = k.viewer_metallic ? 0.0f : gpbr.x;
        float a[3] = { fminf(fmaxf(gcol.x, 0.0f), 1.0f), fminf(fmaxf(gcol.y, 0.0f), 1.0f), fminf(fmaxf(gcol.z, 0.0f), 1.0f) };
        a[0] = pow_fast(a[0], 2.2f); a[1] = pow_fast(a[1], 2.2f); a[2] = pow_fast(a[2], 2.2f);
        float L0 = k.light[0] - ws.x, L1 = k.light[1] - ws.y, L2 = k.light[2] - ws.z;
        const float d2 = dot3(L0, L1, L2, L0, L1, L2);
        const float d = __builtin_amdgcn_sqrtf(d2);
        normalize3(L0, L1, L2);
        const float attenuation = 1.0f / (d * d);
        const float r[3] = { (k.color[0] * k.intensity) * attenuation, (k.color[1] * k.intensity) * attenuation, (k.color[2] * k.intensity) * attenuation };
        const float im = 1.0f - metallic;
        const float F0[3] = { 0.04f * im + a[0] * metallic, 0.04f * im + a[1] * metallic, 0.04f * im + a[2] * metallic };
        const float ar = roughness * roughness, aa = ar * ar;
        const float nl = max0(dot3(N0, N1, N2, L0, L1, L2));
        const float rr = roughness + 1.0f, kk = (rr * rr) / 8.0f;
        const float Gl = nl / (nl * (1.0f - kk) + kk);
        const float lit = 1.0f - shadow;
        const float ig = 1.0f / 2.2f;
        const float amb[3] = { 0.3f * a[0], 0.3f * a[1], 0.3f * a[2] };
        for (uint32_t t = 0; t < k.n_dirs; ++t) {                                          // wave-uniform: the table row is scalar
            const float* row = tab + (size_t)t * 20;
            const float V0 = -row[0], V1 = -row[1], V2 = -row[2];
            float H0 = V0 + L0, H1 = V1 + L1, H2 = V2 + L2;
            normalize3(H0, H1, H2);
            const float hv = max0(dot3(H0, H1, H2, V0, V1, V2));
            const float fc = fminf(fmaxf(1.0f - hv, 0.0f), 1.0f);
            const float f5 = pow_fast(fc, 5.0f);
            const float nh = max0(dot3(N0, N1, N2, H0, H1, H2));
            float den = (nh * nh) * (aa - 1.0f) + 1.0f;
            den = ((22.0f / 7.0f) * den) * den;
            const float NDF = aa / den;
            const float nv = max0(dot3(N0, N1, N2, V0, V1, V2));
            const float G = Gl * (nv / (nv * (1.0f - kk) + kk));
            const float ng = NDF * G;
            const float denominator = (4.0f * nv) * nl + 0.0001f;
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float F = F0[c] + (1.0f - F0[c]) * f5;
                const float s = (ng * F) / denominator;
                const float kD = (1.0f - F) * im;
                const float Lo = ((((kD * a[c]) / 22.0f) / 7.0f + s) * r[c]) * nl * lit;
                float col = amb[c] + Lo;
                col = pow_fast(col / (col + 1.0f), ig);
                v[c] = col - 0.5f;
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float wb = row[4 + j];
                acc[0][j] = acc[0][j] + wb * v[0];
                acc[1][j] = acc[1][j] + wb * v[1];
                acc[2][j] = acc[2][j] + wb * v[2];
            }
        }
    }
    // ---- f_dc[3], then f_rest channel-major, coefficients above the degree +0.0
    float* mine = s_out + lane * kBakeStride;
#pragma unroll
    for (int c = 0; c < 3; ++c) mine[c] = acc[c][0];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 1; j < 16; ++j) mine[3 + 15 * c + (j - 1)] = (uint32_t)j < k.n_coef ? acc[c][j] : 0.0f;
    __syncthreads();
    const uint32_t left = n - first;
    const uint32_t words4 = (left < (uint32_t)kBakeLanes ? left : (uint32_t)kBakeLanes) * 12u;    // float4 words this workgroup owns
    float4* out = plane + (size_t)first * 12;
#pragma unroll
    for (int it = 0; it < 12; ++it) {
        const uint32_t t = (uint32_t)it * kBakeLanes + lane;
        if (t < words4) {
            const float* src = s_out + (t / 12u) * kBakeStride + (t % 12u) * 4u;
            nt_store(out + t, make_float4(src[0], src[1], src[2], src[3]));
        }
    }
}

__global__ void __launch_bounds__(256) k_sh_shade(const ShadeK k, const float4* __restrict__ rec, const float4* __restrict__ sh, uint32_t n,
                                                  float4* __restrict__ dst) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4* g = rec + (size_t)i * 6;
    const float4 gpos = g[0], gcol = g[1];
    const float4 ws = m4_mul(k.M, gpos.x, gpos.y, gpos.z, 1.0f);
    float x = ws.x - k.cam[0], y = ws.y - k.cam[1], z = ws.z - k.cam[2];
    normalize3(x, y, z);
    float B[16];
    sh_basis<float>(x, y, z, B);
    float cf[48];
    const float4* s4 = sh + (size_t)i * 12;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const float4 v = s4[q];
        cf[4 * q] = v.x; cf[4 * q + 1] = v.y; cf[4 * q + 2] = v.z; cf[4 * q + 3] = v.w;
    }
    float col[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float s = 0.5f + cf[c] * B[0];
#pragma unroll
        for (int j = 1; j < 16; ++j) s = s + cf[3 + 15 * c + (j - 1)] * B[j];
        col[c] = max0(s);
    }
    float4* o = dst + (size_t)i * 6;
    o[0] = gpos;
    o[1] = make_float4(col[0], col[1], col[2], gcol.w);
    o[2] = g[2]; o[3] = g[3]; o[4] = g[4]; o[5] = g[5];
}

}  // namespace

hipError_t launch_bake_sh(const BakeK& k, const float4* rec, uint32_t n, const float* table, const float* cube, float* plane, uint8_t* counts,
                          hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_bake_sh, dim3((n + kBakeLanes - 1u) / kBakeLanes), dim3(kBakeLanes), 0, st, k, rec, n, table, cube, (float4*)plane, counts);
    return hipGetLastError();
}

hipError_t launch_sh_shade(const ShadeK& k, const float4* rec, const float* sh, uint32_t n, float4* dst, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_sh_shade, dim3((n + 255u) / 256u), dim3(256), 0, st, k, rec, (const float4*)sh, n, dst);
    return hipGetLastError();
}

}  // namespace m2s
