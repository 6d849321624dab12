// m2s_compactmath.h — the arithmetic of the compact .ply (include/m2s.h "compact export"): ONE statement of every rounding, clamp and
// bit position, compiled into the host writer (m2s_compact_host.cpp), the device kernels (m2s_compact.hip) and the reader's decoder, so
// that the device's bytes equal the host's by construction.  fp32, one rounding per operation, no contraction; `/` and sqrtf are IEEE on
// both sides.  The logarithm is NOT here: the callers pass log-scales in (the C library's logf on the host, logf_glibc on the device).
// Self-contained (no HIP header needed): a plain host compiler builds the writer and the reader for the fuzzer.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIP__)
#define M2S_HD __host__ __device__ inline
#else
#define M2S_HD inline
#endif
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace m2s_compact {

constexpr uint32_t kChunkRows = 256;
constexpr uint32_t kInvalidKey = 1u << 30;          // behind every 30-bit Morton key
constexpr float kShC0 = 0.28209479177387814f;

M2S_HD uint32_t f2u(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
M2S_HD float u2f(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }
M2S_HD bool finite(float v) { return (f2u(v) & 0x7F800000u) != 0x7F800000u; }

// The order every min / max of the format is taken in: the floats as a line, -0 below +0 (and a NaN of the baked plane beyond the
// infinity of its sign) — an unsigned integer per float, so that the result does not depend on the order of the reduction.
M2S_HD uint32_t ord(float v) { const uint32_t u = f2u(v); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
M2S_HD float unord(uint32_t k) { return u2f((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
constexpr uint32_t kOrdMinNeutral = 0xFFFFFFFFu, kOrdMaxNeutral = 0u;

// 1. valid records: position.xyz, color.rgba, scale.xyz, rotation finite; scale.xyz >= 0; n2 finite and > 0
M2S_HD float quat_n2(const float* q) { return ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]; }
M2S_HD bool valid(const float* pos, const float* col, const float* scl, const float* rot) {
    bool ok = finite(pos[0]) && finite(pos[1]) && finite(pos[2]) && finite(col[0]) && finite(col[1]) && finite(col[2]) && finite(col[3]) &&
              finite(scl[0]) && finite(scl[1]) && finite(scl[2]) && finite(rot[0]) && finite(rot[1]) && finite(rot[2]) && finite(rot[3]);
    ok = ok && scl[0] >= 0.0f && scl[1] >= 0.0f && scl[2] >= 0.0f;
    const float n2 = quat_n2(rot);
    return ok && finite(n2) && n2 > 0.0f;
}

// 3. key
M2S_HD uint32_t axis_cell(float p, float bmin, float bmax) {
    const float ext = bmax - bmin;
    if (!(ext > 0.0f)) return 0u;
    const float f = floorf(((p - bmin) / ext) * 1024.0f);
    return f >= 1023.0f ? 1023u : f > 0.0f ? (uint32_t)f : 0u;        // (NaN — an extent beyond the largest float — gives 0)
}
M2S_HD uint32_t part1by2(uint32_t x) {
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}
M2S_HD uint32_t morton_key(const float* p, const float* bmin, const float* bmax) {
    return part1by2(axis_cell(p[0], bmin[0], bmax[0])) | (part1by2(axis_cell(p[1], bmin[1], bmax[1])) << 1) |
           (part1by2(axis_cell(p[2], bmin[2], bmax[2])) << 2);
}

// 5. row values
M2S_HD float clamp_log_scale(float l) {               // min(max(l, -20), 20); l is never NaN for a valid record and a finite multiplier > 0
    const float a = l < -20.0f ? -20.0f : l;
    return a > 20.0f ? 20.0f : a;
}
M2S_HD float sh_dc_colour(float dc) { return dc * kShC0 + 0.5f; }

// 7. packing
M2S_HD uint32_t unorm(float v, uint32_t t) {          // t = 2^b - 1; a NaN packs as 0
    const float x = floorf(v * (float)t + 0.5f);
    return x > 0.0f ? (x < (float)t ? (uint32_t)x : t) : 0u;
}
M2S_HD float nrm(float v, float lo, float hi) { return (hi - lo < 0.00001f) ? 0.0f : (v - lo) / (hi - lo); }
M2S_HD uint32_t pack_11_10_11(const float* v, const float* lo, const float* hi) {
    return (unorm(nrm(v[0], lo[0], hi[0]), 2047u) << 21) | (unorm(nrm(v[1], lo[1], hi[1]), 1023u) << 11) | unorm(nrm(v[2], lo[2], hi[2]), 2047u);
}
M2S_HD uint32_t pack_colour(const float* c, const float* lo, const float* hi, float alpha) {
    return (unorm(nrm(c[0], lo[0], hi[0]), 255u) << 24) | (unorm(nrm(c[1], lo[1], hi[1]), 255u) << 16) | (unorm(nrm(c[2], lo[2], hi[2]), 255u) << 8) |
           unorm(alpha, 255u);
}
M2S_HD uint32_t pack_rotation(const float* rot) {     // rot = (w, x, y, z) as stored in the record
    const float len = sqrtf(quat_n2(rot));
    float a0 = rot[0] / len, a1 = rot[1] / len, a2 = rot[2] / len, a3 = rot[3] / len;
    uint32_t L = 0;
    float big = fabsf(a0);
    if (fabsf(a1) > big) { big = fabsf(a1); L = 1; }
    if (fabsf(a2) > big) { big = fabsf(a2); L = 2; }
    if (fabsf(a3) > big) { big = fabsf(a3); L = 3; }
    const float aL = L == 0 ? a0 : L == 1 ? a1 : L == 2 ? a2 : a3;
    if (aL < 0.0f) { a0 = -a0; a1 = -a1; a2 = -a2; a3 = -a3; }
    uint32_t w = L;
    if (L != 0) w = (w << 10) | unorm(a0 * 0.70710678f + 0.5f, 1023u);
    if (L != 1) w = (w << 10) | unorm(a1 * 0.70710678f + 0.5f, 1023u);
    if (L != 2) w = (w << 10) | unorm(a2 * 0.70710678f + 0.5f, 1023u);
    if (L != 3) w = (w << 10) | unorm(a3 * 0.70710678f + 0.5f, 1023u);
    return w;
}

// 8. SH element: K = (d + 1)^2 - 1 coefficients per channel; word of coefficient i (1..K) of channel c in the plane's float[48] row
M2S_HD uint32_t sh_coefficients(uint32_t degree) { return (degree + 1u) * (degree + 1u) - 1u; }
M2S_HD uint32_t sh_plane_word(uint32_t c, uint32_t i) { return 3u + 15u * c + i - 1u; }
M2S_HD uint32_t sh_byte(float v) {                    // a NaN packs as 0
    const float x = truncf((v / 8.0f + 0.5f) * 256.0f);
    return x > 0.0f ? (x < 255.0f ? (uint32_t)x : 255u) : 0u;
}

// ---- decoder (m2s_read_ply) ----
M2S_HD float lerp_unorm(uint32_t q, uint32_t t, float lo, float hi) { return lo + ((float)q / (float)t) * (hi - lo); }
M2S_HD void unpack_rotation(uint32_t w, float* rot) {
    const uint32_t L = w >> 30;
    float v[3], s = 0.0f;
    for (int k = 0; k < 3; ++k) {
        v[k] = ((float)((w >> (10 * (2 - k))) & 1023u) / 1023.0f - 0.5f) / 0.70710678f;
        s += v[k] * v[k];
    }
    const float m = sqrtf(1.0f - s > 0.0f ? 1.0f - s : 0.0f);
    int k = 0;
    for (uint32_t i = 0; i < 4; ++i) rot[i] = i == L ? m : v[k++];
}

}  // namespace m2s_compact
