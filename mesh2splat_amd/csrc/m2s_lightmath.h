// m2s_lightmath.h — what the deferred shader (gaussianSplattingDeferredPS.glsl) is made of, shared by the two kernels that evaluate
// it: k_relight (m2s_light.hip, per pixel) and k_bake_sh (m2s_bake.hip, per Gaussian and view direction).  One definition, so that the
// baked light takes the cube texel, the 20 taps and the fast-math flavour of the frame's.
//   decision arithmetic (cube_fetch, shadow_taps): IEEE fp32 operation by operation, correctly rounded root and division
//   value arithmetic (pow_fast, normalize3): fp32 with the device's fast log2 / exp2 / reciprocal square root
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#pragma clang fp contract(off)

namespace m2s {

// value arithmetic: the device's fast log2 / exp2 / reciprocal square root
__device__ __forceinline__ float pow_fast(float x, float y) { return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x)); }
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
    const float r = __builtin_amdgcn_rsqf(dot3(x, y, z, x, y, z));
    x *= r; y *= r; z *= r;
}
__device__ __forceinline__ float max0(float v) { return v > 0.0f ? v : (v == v ? 0.0f : v); }      // max(v, 0.0) with NaN kept

// texture(u_shadowCubemap, v).r: OpenGL 4.6 table 8.19, GL_NEAREST, clamp to edge; a NaN coordinate reads texel 0 of face 5
__device__ __forceinline__ float cube_fetch(const float* __restrict__ cube, int S, float x, float y, float z) {
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    int face;
    float sc, tc, ma;
    if (ax >= ay && ax >= az) { ma = ax; if (x < 0.0f) { face = 1; sc = z; tc = -y; } else { face = 0; sc = -z; tc = -y; } }
    else if (ay >= az) { ma = ay; if (y < 0.0f) { face = 3; sc = x; tc = -z; } else { face = 2; sc = x; tc = z; } }
    else { ma = az; if (z < 0.0f) { face = 5; sc = -x; tc = -y; } else { face = 4; sc = x; tc = -y; } }
    const float s = 0.5f * (sc / ma + 1.0f), t = 0.5f * (tc / ma + 1.0f);
    const size_t SS = (size_t)S * (size_t)S;
    if (s != s || t != t) return cube[5 * SS];
    const float fs = floorf(s * (float)S), ft = floorf(t * (float)S), hi = (float)(S - 1);
    const int i = (int)fminf(fmaxf(fs, 0.0f), hi), j = (int)fminf(fmaxf(ft, 0.0f), hi);
    return cube[(size_t)face * SS + (size_t)j * (size_t)S + (size_t)i];
}

// computeShadowFactor (:70-99) up to the division by 20: how many of the 20 taps round normalize(p - light) are shadowed
__device__ __forceinline__ uint32_t shadow_taps(const float* __restrict__ cube, int S, float p0, float p1, float p2, float lx, float ly, float lz,
                                                float far_plane) {
    uint32_t count = 0;
    const float dx = p0 - lx, dy = p1 - ly, dz = p2 - lz;
    const float cur = sqrtf((dx * dx + dy * dy) + dz * dz);
    const float sx = dx / cur, sy = dy / cur, sz = dz / cur;
    const float lhs = cur - 0.05f;
    // sampleOffsetDirections
    constexpr int8_t OFF[20][3] = { { 1, 1, 1 }, { 1, -1, 1 }, { -1, -1, 1 }, { -1, 1, 1 }, { 1, 1, -1 }, { 1, -1, -1 }, { -1, -1, -1 }, { -1, 1, -1 },
                                    { 1, 1, 0 }, { 1, -1, 0 }, { -1, -1, 0 }, { -1, 1, 0 }, { 1, 0, 1 }, { -1, 0, 1 }, { 1, 0, -1 }, { -1, 0, -1 },
                                    { 0, 1, 1 }, { 0, -1, 1 }, { 0, -1, -1 }, { 0, 1, -1 } };
#pragma unroll
    for (int i = 0; i < 20; ++i) {
        const float vx = sx + (float)OFF[i][0] * 0.025f, vy = sy + (float)OFF[i][1] * 0.025f, vz = sz + (float)OFF[i][2] * 0.025f;
        const float closest = cube_fetch(cube, S, vx, vy, vz) * far_plane;
        count += lhs > closest ? 1u : 0u;
    }
    return count;
}

}  // namespace m2s
