// m2s_merge.hip — device side of the merge pass (include/m2s.h "merge pass"): neighbouring records are replaced by their
// moment-matched parent.  Order (validity, box, Morton keys, stable sort) is the compact export's own — compact_keys_and_sort,
// m2s_compact.hip — and everything behind it is here: the run flags over the sorted sequence, two rocPRIM scans that turn them into
// segments, and the reduction of every segment into one 96-byte record.  Segmentation is integer logic and exact fp32 (no contraction);
// the parent is fp64 throughout, one lane per segment walking its members in sorted order: no floating-point atomics, the same bits
// from run to run.  Under M2S_MERGE_MODEL_GAUSSIAN (m2s_set_merge_model) the heads, the reduction and the SH weights are the
// instances of pins 2g, 5g, 5sg: k_merge_heads<true, true>, k_merge_reduce_gauss, k_merge_reduce_sh<true>.
#include <rocprim/device/device_scan.hpp>

#include "m2s_compactmath.h"
#include "m2s_device.h"

#pragma clang fp contract(off)

namespace m2s {

namespace mc = m2s_compact;

// castQuatToMat3's third row (m2s_covmath.h: rot.c[0][2], c[1][2], c[2][2]) of the stored vec4, its own fp32 expressions
__device__ __forceinline__ void quat_axis3(float4 q, float& a0, float& a1, float& a2) {
    const float x = q.x, y = q.y, z = q.z, w = q.w;
    a0 = 2.f * (y * w + x * z);
    a1 = 2.f * (z * w - x * y);
    a2 = 1.f - 2.f * (y * y + z * z);
}

// ... its first and second rows (rot.c[0][0], c[1][0], c[2][0] and rot.c[0][1], c[1][1], c[2][1]), likewise
__device__ __forceinline__ void quat_axis1(float4 q, float& a0, float& a1, float& a2) {
    const float x = q.x, y = q.y, z = q.z, w = q.w;
    a0 = 1.f - 2.f * (z * z + w * w);
    a1 = 2.f * (y * z + x * w);
    a2 = 2.f * (y * w - x * z);
}
__device__ __forceinline__ void quat_axis2(float4 q, float& a0, float& a1, float& a2) {
    const float x = q.x, y = q.y, z = q.z, w = q.w;
    a0 = 2.f * (y * z - x * w);
    a1 = 1.f - 2.f * (y * y + w * w);
    a2 = 2.f * (z * w + x * y);
}

// Pin 2g: the row of the smallest |scale[k]|, the lower k on a tie (a flat record: its r_3, pin 2's own axis)
__device__ __forceinline__ void gauss_axis(float4 scl, float4 q, float& a0, float& a1, float& a2) {
    const float s0 = fabsf(scl.x), s1 = fabsf(scl.y), s2 = fabsf(scl.z);
    const float s01 = s1 < s0 ? s1 : s0;
    if (s2 < s01) quat_axis3(q, a0, a1, a2);
    else if (s1 < s0) quat_axis2(q, a0, a1, a2);
    else quat_axis1(q, a0, a1, a2);
}

// Pin 2.  flag[j] = j where sorted position j starts a run, else 0 (the inclusive maximum of the flags is every position's run start).
// kUnsigned (M2S_MERGE_UNSIGNED_AXIS, pin 2u): the same d, its sign dropped before the comparison.
// kGauss (M2S_MERGE_MODEL_GAUSSIAN, pin 2g; always with kUnsigned): the axes are those of the smallest scales, not the third rows.
template <bool kUnsigned, bool kGauss = false>
__global__ void __launch_bounds__(kBlock) k_merge_heads(const float4* __restrict__ rec, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                        uint32_t n, uint32_t shift, float min_axis_dot, uint32_t* __restrict__ flag) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    bool head = j == 0;
    if (!head) {
        const uint32_t k1 = keys[j], k0 = keys[j - 1];
        head = k1 == mc::kInvalidKey || k0 == mc::kInvalidKey || (k1 >> shift) != (k0 >> shift);
        if (!head) {
            float a0, a1, a2, b0, b1, b2;
            if constexpr (kGauss) {
                const float4 *ga = rec + (size_t)perm[j] * 6, *gb = rec + (size_t)perm[j - 1] * 6;
                gauss_axis(ga[2], ga[4], a0, a1, a2);
                gauss_axis(gb[2], gb[4], b0, b1, b2);
            } else {
                quat_axis3(rec[(size_t)perm[j] * 6 + 4], a0, a1, a2);
                quat_axis3(rec[(size_t)perm[j - 1] * 6 + 4], b0, b1, b2);
            }
            const float d = ((a0 * b0) + a1 * b1) + a2 * b2;
            head = !((kUnsigned ? fabsf(d) : d) >= min_axis_dot);
        }
    }
    flag[j] = head ? j : 0u;
}

// Pin 3.  Position j starts a segment where it is a whole number of max_group members behind its run's start.  packed[j] = that flag,
// and in the upper half whether the segment it starts has a second member (the next position starts none): one 64-bit sum then gives
// the segment ids and counts the segments of two members or more, without an atomic.  Neither half can carry: both sums are <= n < 2^32.
__global__ void __launch_bounds__(kBlock) k_merge_cuts(const uint32_t* __restrict__ run_start, uint32_t n, uint32_t max_group,
                                                       unsigned long long* __restrict__ packed) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const bool h = (j - run_start[j]) % max_group == 0u;
    const bool hn = j + 1 == n || (j + 1 - run_start[j + 1]) % max_group == 0u;
    packed[j] = (unsigned long long)h | ((unsigned long long)(h && !hn) << 32);
}

// seg_start[s] = first sorted position of segment s, seg_start[segments] = n; totals = { segments, segments of two members or more }
__global__ void __launch_bounds__(kBlock) k_merge_starts(const unsigned long long* __restrict__ packed, const unsigned long long* __restrict__ sums, uint32_t n,
                                                         uint32_t* __restrict__ seg_start, uint32_t* __restrict__ totals) {
    const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const unsigned long long in = packed[j], ex = sums[j];
    const uint32_t h = (uint32_t)in, s = (uint32_t)ex;
    if (h) seg_start[s] = j;
    if (j + 1 == n) {
        seg_start[s + h] = n;
        totals[0] = s + h;
        totals[1] = (uint32_t)(ex >> 32) + (uint32_t)(in >> 32);
    }
}

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ D3 operator*(double s, D3 a) { return { s * a.x, s * a.y, s * a.z }; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
__device__ __forceinline__ D3 d3(float4 v) { return { (double)v.x, (double)v.y, (double)v.z }; }

// the three rows of castQuatToMat3 of the stored vec4, in fp64
__device__ __forceinline__ void quat_rows(float4 q, D3& r1, D3& r2, D3& r3) {
    const double x = q.x, y = q.y, z = q.z, w = q.w;
    r1 = { 1.0 - 2.0 * (z * z + w * w), 2.0 * (y * z + x * w), 2.0 * (y * w - x * z) };
    r2 = { 2.0 * (y * z - x * w), 1.0 - 2.0 * (y * y + w * w), 2.0 * (z * w + x * y) };
    r3 = { 2.0 * (y * w + x * z), 2.0 * (z * w - x * y), 1.0 - 2.0 * (y * y + z * z) };
}

// v minus its component along the unit vector nb, normalised; false where less than 1e-6 of its length is left
__device__ __forceinline__ bool tangent_of(D3 v, D3 nb, D3& t) {
    const D3 p = v - dot(v, nb) * nb;
    const double l2 = dot(p, p);
    if (!(l2 >= 1e-12 * dot(v, v)) || !(l2 > 0.0)) return false;
    t = (1.0 / sqrt(l2)) * p;
    return true;
}

// Pins 4 - 6.  Lane s = segment s: members perm[seg_start[s]] .. perm[seg_start[s + 1] - 1], at most 64.  Two walks: the weights' sum,
// the centroid and the plane first (the moments are taken about the one and in the other), then everything else.  The second walk finds its records in L2.
// kUnsigned (pin 5u): the first walk turns every member's r_3 onto the side of the oriented r_3 of the member before it, then sums it.
template <bool kUnsigned>
__global__ void __launch_bounds__(kBlock) k_merge_reduce(const float4* __restrict__ rec, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ seg_start,
                                                         const uint32_t* __restrict__ totals, float4* __restrict__ out, uint32_t* __restrict__ map) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= totals[0]) return;
    const uint32_t a = seg_start[s], b = seg_start[s + 1];
    const uint32_t first = perm[a];
    const float4* g1 = rec + (size_t)first * 6;
    float4* o = out + (size_t)s * 6;
    map[first] = s;
    if (b - a == 1u) {
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = g1[k];
        return;
    }
    const float4 pos1 = g1[0], scl1 = g1[2], nrm1 = g1[3], rot1 = g1[4], pbr1 = g1[5];
    const D3 p1 = d3(pos1);
    // walk 1: W, the centroid and the plane's normal, for both weightings (the area, and 1 where the areas add up to nothing)
    double W = 0.0;
    D3 sw = { 0, 0, 0 }, s1 = { 0, 0, 0 }, nsum = { 0, 0, 0 }, n1 = { 0, 0, 0 };
    [[maybe_unused]] D3 prev = { 0, 0, 0 };   // o_{i-1}; zero in front of the first member, which therefore never flips
    for (uint32_t j = a; j < b; ++j) {
        const uint32_t i = perm[j];
        const float4* g = rec + (size_t)i * 6;
        const float4 scl = g[2];
        const D3 d = d3(g[0]) - p1;
        D3 q1, q2, q3;
        quat_rows(g[4], q1, q2, q3);
        if constexpr (kUnsigned) {
            if (dot(q3, prev) < 0.0) q3 = { -q3.x, -q3.y, -q3.z };   // (false for a zero and for a NaN: no flip)
            prev = q3;
        }
        const double w = (double)scl.x * (double)scl.y;
        W += w;
        sw = sw + w * d;
        s1 = s1 + d;
        nsum = nsum + w * q3;
        n1 = n1 + q3;
        map[i] = s;
    }
    const bool unit = W == 0.0;
    if (unit) { W = (double)(b - a); sw = s1; nsum = n1; }
    const D3 mu = (1.0 / W) * sw;
    D3 r1, r2, r3;
    quat_rows(rot1, r1, r2, r3);
    double l2 = dot(nsum, nsum);
    if (!(l2 > 0.0) || !isfinite(l2)) { nsum = r3; l2 = dot(r3, r3); }
    D3 nb = { 0.0, 0.0, 1.0 };
    if (l2 > 0.0 && isfinite(l2)) nb = (1.0 / sqrt(l2)) * nsum;
    D3 t1;
    if (!tangent_of(r1, nb, t1) && !tangent_of(r2, nb, t1)) t1 = r1;
    const D3 t2 = cross(nb, t1);
    // walk 2: the in-plane moments about the centroid, alpha, colour, normal, pbr
    double ma = 0.0, mb = 0.0, mcc = 0.0, swa = 0.0;
    D3 cwa = { 0, 0, 0 }, cw = { 0, 0, 0 }, ns = { 0, 0, 0 };
    double pb0 = 0.0, pb1 = 0.0;
    for (uint32_t j = a; j < b; ++j) {
        const float4* g = rec + (size_t)perm[j] * 6;
        const float4 col = g[1], scl = g[2], nrm = g[3], pbr = g[5];
        D3 q1, q2, q3;
        quat_rows(g[4], q1, q2, q3);
        const double w = unit ? 1.0 : (double)scl.x * (double)scl.y;
        const double kx = (double)scl.x * (double)scl.x / 12.0, ky = (double)scl.y * (double)scl.y / 12.0;
        const D3 e = (d3(g[0]) - p1) - mu;
        const double u1 = dot(t1, q1), u2 = dot(t1, q2), v1 = dot(t2, q1), v2 = dot(t2, q2), du = dot(t1, e), dv = dot(t2, e);
        ma += w * ((kx * u1 * u1 + ky * u2 * u2) + du * du);
        mb += w * ((kx * u1 * v1 + ky * u2 * v2) + du * dv);
        mcc += w * ((kx * v1 * v1 + ky * v2 * v2) + dv * dv);
        const double wa = w * (double)col.w;
        swa += wa;
        cwa = cwa + wa * d3(col);
        cw = cw + w * d3(col);
        ns = ns + w * d3(nrm);
        pb0 += w * (double)pbr.x;
        pb1 += w * (double)pbr.y;
    }
    ma /= W; mb /= W; mcc /= W;
    const double dd = sqrt((ma - mcc) * (ma - mcc) + 4.0 * mb * mb);
    const double lam1 = ((ma + mcc) + dd) / 2.0;
    const double lam2 = fmax(((ma + mcc) - dd) / 2.0, 0.0);
    D3 e1 = t1;
    if (dd != 0.0) {
        double ex = mb, ey = lam1 - ma;
        const double fx = lam1 - mcc, fy = mb;
        if (fx * fx + fy * fy > ex * ex + ey * ey) { ex = fx; ey = fy; }
        const double il = 1.0 / sqrt(ex * ex + ey * ey);
        e1 = (ex * il) * t1 + (ey * il) * t2;
    }
    const D3 e2 = cross(nb, e1);
    // quat_cast (m2s_devfn.h: geo_flat) of the matrix with columns e1, e2, nb, in fp64; stored (w, x, y, z), first float >= 0
    double qw, qx, qy, qz;
    {
        const double m00 = e1.x, m01 = e1.y, m02 = e1.z, m10 = e2.x, m11 = e2.y, m12 = e2.z, m20 = nb.x, m21 = nb.y, m22 = nb.z;
        const double fx = m00 - m11 - m22, fy = m11 - m00 - m22, fz = m22 - m00 - m11, fw = m00 + m11 + m22;
        int bi = 0;
        double fb = fw;
        if (fx > fb) { fb = fx; bi = 1; }
        if (fy > fb) { fb = fy; bi = 2; }
        if (fz > fb) { fb = fz; bi = 3; }
        const double bv = sqrt(fb + 1.0) * 0.5, mult = 0.25 / bv;
        const double d0 = m12 - m21, d1 = m20 - m02, d2 = m01 - m10, s0 = m01 + m10, s1_ = m20 + m02, s2 = m12 + m21;
        if (bi == 0) { qw = bv; qx = d0 * mult; qy = d1 * mult; qz = d2 * mult; }
        else if (bi == 1) { qw = d0 * mult; qx = bv; qy = s0 * mult; qz = s1_ * mult; }
        else if (bi == 2) { qw = d1 * mult; qx = s0 * mult; qy = bv; qz = s2 * mult; }
        else { qw = d2 * mult; qx = s1_ * mult; qy = s2 * mult; qz = bv; }
        if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
    }
    const double nl2 = dot(ns, ns);
    const bool nok = nl2 > 0.0 && isfinite(nl2);
    const double ni = nok ? 1.0 / sqrt(nl2) : 0.0;
    const D3 rgb = swa != 0.0 ? (1.0 / swa) * cwa : (1.0 / W) * cw;
    o[0] = make_float4((float)(p1.x + mu.x), (float)(p1.y + mu.y), (float)(p1.z + mu.z), pos1.w);
    o[1] = make_float4((float)rgb.x, (float)rgb.y, (float)rgb.z, (float)(swa / W));
    o[2] = make_float4((float)sqrt(12.0 * lam1), (float)sqrt(12.0 * lam2), scl1.z, scl1.w);
    o[3] = nok ? make_float4((float)(ns.x * ni), (float)(ns.y * ni), (float)(ns.z * ni), nrm1.w) : make_float4(0.0f, 0.0f, 0.0f, nrm1.w);
    o[4] = make_float4((float)qw, (float)qx, (float)qy, (float)qz);
    o[5] = make_float4((float)(pb0 / W), (float)(pb1 / W), pbr1.z, pbr1.w);
}

// k_merge_reduce's quat_cast of the matrix with columns c0, c1, c2, the same operations (k_merge_reduce keeps its own text: its
// instances stay the code they were)
__device__ __forceinline__ void quat_cast_wxyz(D3 c0, D3 c1, D3 c2, double& qw, double& qx, double& qy, double& qz) {
    const double m00 = c0.x, m01 = c0.y, m02 = c0.z, m10 = c1.x, m11 = c1.y, m12 = c1.z, m20 = c2.x, m21 = c2.y, m22 = c2.z;
    const double fx = m00 - m11 - m22, fy = m11 - m00 - m22, fz = m22 - m00 - m11, fw = m00 + m11 + m22;
    int bi = 0;
    double fb = fw;
    if (fx > fb) { fb = fx; bi = 1; }
    if (fy > fb) { fb = fy; bi = 2; }
    if (fz > fb) { fb = fz; bi = 3; }
    const double bv = sqrt(fb + 1.0) * 0.5, mult = 0.25 / bv;
    const double d0 = m12 - m21, d1 = m20 - m02, d2 = m01 - m10, s0 = m01 + m10, s1_ = m20 + m02, s2 = m12 + m21;
    if (bi == 0) { qw = bv; qx = d0 * mult; qy = d1 * mult; qz = d2 * mult; }
    else if (bi == 1) { qw = d0 * mult; qx = bv; qy = s0 * mult; qz = s1_ * mult; }
    else if (bi == 2) { qw = d1 * mult; qx = s0 * mult; qy = bv; qz = s2 * mult; }
    else { qw = d2 * mult; qx = s1_ * mult; qy = s2 * mult; qz = bv; }
    if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
}

// Pin 5g: the product of the two largest of |s1|, |s2|, |s3| (exact in fp64: two 24-bit significands), |sx sy| for a flat record
__device__ __forceinline__ double gauss_area(double s1, double s2, double s3) {
    const double a1 = fabs(s1), a2 = fabs(s2), a3 = fabs(s3);
    const double lo = fmin(fmin(a1, a2), a3);
    return lo == a3 ? a1 * a2 : lo == a2 ? a1 * a3 : a2 * a3;
}

// One rotation of pin 5g's cyclic Jacobi iteration on the pair (p, q) of a symmetric 3 x 3 matrix, r the third index: app, aqq, apq
// and the two elements arp, arq beside them; (v0p, v0q), (v1p, v1q), (v2p, v2q) are columns p and q of the eigenvector matrix.
// Nothing happens where apq is already 0.  An apq so small that theta (or its square) overflows gives t = 0: apq is dropped.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q, double& v1p,
                                              double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    const double x0 = v0p, y0 = v0q, x1 = v1p, y1 = v1q, x2 = v2p, y2 = v2q;
    v0p = c * x0 - s * y0; v0q = s * x0 + c * y0;
    v1p = c * x1 - s * y1; v1q = s * x1 + c * y1;
    v2p = c * x2 - s * y2; v2q = s * x2 + c * y2;
}

constexpr int kJacobiSweeps = 16;   // (pin 5g; a 3 x 3 matrix is diagonal to the last bit after 5 - 7)

// Pins 4, 5g, 6 (M2S_MERGE_MODEL_GAUSSIAN).  Lane s = segment s, as k_merge_reduce: two walks over at most 64 members, fp64, no atomics.
// Walk 1: the weights' sum and the centroid; walk 2: the six elements of the full moment M about it, alpha, colour, normal, pbr.  Then the
// eigenpairs of M by cyclic Jacobi rotations, the three pairs written out and every element a named scalar: nothing is indexed, nothing
// goes to scratch.  sigma: what a stored scale is multiplied with to be a standard deviation in the units of the positions.
__global__ void __launch_bounds__(kBlock) k_merge_reduce_gauss(const float4* __restrict__ rec, const uint32_t* __restrict__ perm,
                                                               const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ totals, float sigma_f,
                                                               float4* __restrict__ out, uint32_t* __restrict__ map) {
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= totals[0]) return;
    const uint32_t a = seg_start[s], b = seg_start[s + 1];
    const uint32_t first = perm[a];
    const float4* g1 = rec + (size_t)first * 6;
    float4* o = out + (size_t)s * 6;
    map[first] = s;
    if (b - a == 1u) {
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = g1[k];
        return;
    }
    const float4 pos1 = g1[0], scl1 = g1[2], nrm1 = g1[3], pbr1 = g1[5];
    const D3 p1 = d3(pos1);
    const double sigma = (double)sigma_f, sigma2 = sigma * sigma;
    // walk 1: W and the centroid, for both weightings (the area, and 1 where the areas add up to nothing)
    double W = 0.0;
    D3 sw = { 0, 0, 0 }, s1 = { 0, 0, 0 };
    for (uint32_t j = a; j < b; ++j) {
        const uint32_t i = perm[j];
        const float4* g = rec + (size_t)i * 6;
        const float4 scl = g[2];
        const D3 d = d3(g[0]) - p1;
        const double w = gauss_area((double)scl.x, (double)scl.y, (double)scl.z);
        W += w;
        sw = sw + w * d;
        s1 = s1 + d;
        map[i] = s;
    }
    const bool unit = W == 0.0;
    if (unit) { W = (double)(b - a); sw = s1; }
    const D3 mu = (1.0 / W) * sw;
    // walk 2: M = sum w (C + e e^T) / W with C = sigma^2 sum_k s_k^2 r_k r_k^T, and the averaged fields
    double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0, swa = 0.0;
    D3 cwa = { 0, 0, 0 }, cw = { 0, 0, 0 }, ns = { 0, 0, 0 };
    double pb0 = 0.0, pb1 = 0.0;
    for (uint32_t j = a; j < b; ++j) {
        const float4* g = rec + (size_t)perm[j] * 6;
        const float4 col = g[1], scl = g[2], nrm = g[3], pbr = g[5];
        D3 q1, q2, q3;
        quat_rows(g[4], q1, q2, q3);
        const double w = unit ? 1.0 : gauss_area((double)scl.x, (double)scl.y, (double)scl.z);
        const double k1 = (double)scl.x * (double)scl.x, k2 = (double)scl.y * (double)scl.y, k3 = (double)scl.z * (double)scl.z;
        const D3 e = (d3(g[0]) - p1) - mu;
        m00 += w * (sigma2 * ((k1 * q1.x * q1.x + k2 * q2.x * q2.x) + k3 * q3.x * q3.x) + e.x * e.x);
        m01 += w * (sigma2 * ((k1 * q1.x * q1.y + k2 * q2.x * q2.y) + k3 * q3.x * q3.y) + e.x * e.y);
        m02 += w * (sigma2 * ((k1 * q1.x * q1.z + k2 * q2.x * q2.z) + k3 * q3.x * q3.z) + e.x * e.z);
        m11 += w * (sigma2 * ((k1 * q1.y * q1.y + k2 * q2.y * q2.y) + k3 * q3.y * q3.y) + e.y * e.y);
        m12 += w * (sigma2 * ((k1 * q1.y * q1.z + k2 * q2.y * q2.z) + k3 * q3.y * q3.z) + e.y * e.z);
        m22 += w * (sigma2 * ((k1 * q1.z * q1.z + k2 * q2.z * q2.z) + k3 * q3.z * q3.z) + e.z * e.z);
        const double wa = w * (double)col.w;
        swa += wa;
        cwa = cwa + wa * d3(col);
        cw = cw + w * d3(col);
        ns = ns + w * d3(nrm);
        pb0 += w * (double)pbr.x;
        pb1 += w * (double)pbr.y;
    }
    m00 /= W; m01 /= W; m02 /= W; m11 /= W; m12 /= W; m22 /= W;
    // the eigenpairs: column k of (v00 v01 v02; v10 v11 v12; v20 v21 v22) belongs to the diagonal element k
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        if (m01 == 0.0 && m02 == 0.0 && m12 == 0.0) break;
        jacobi_rotate(m00, m11, m01, m02, m12, v00, v01, v10, v11, v20, v21);   // (0, 1); the third index is 2
        jacobi_rotate(m00, m22, m02, m01, m12, v00, v02, v10, v12, v20, v22);   // (0, 2); the third index is 1
        jacobi_rotate(m11, m22, m12, m01, m02, v01, v02, v11, v12, v21, v22);   // (1, 2); the third index is 0
    }
    double l1 = fmax(m00, 0.0), l2 = fmax(m11, 0.0), l3 = fmax(m22, 0.0);
    D3 e1 = { v00, v10, v20 }, e2 = { v01, v11, v21 }, e3 = { v02, v12, v22 };
    // descending, the lower original index first on a tie: three strict compare-and-swaps of neighbours
    if (l2 > l1) { const double t = l1; l1 = l2; l2 = t; const D3 v = e1; e1 = e2; e2 = v; }
    if (l3 > l2) { const double t = l2; l2 = l3; l3 = t; const D3 v = e2; e2 = e3; e3 = v; }
    if (l2 > l1) { const double t = l1; l1 = l2; l2 = t; const D3 v = e1; e1 = e2; e2 = v; }
    e3 = cross(e1, e2);
    const double sc1 = sqrt(l1) / sigma, sc2 = sqrt(l2) / sigma, sc3 = sqrt(l3) / sigma;
    double qw, qx, qy, qz;
    quat_cast_wxyz(e1, e2, e3, qw, qx, qy, qz);
    const double nl2 = dot(ns, ns);
    const bool nok = nl2 > 0.0 && isfinite(nl2);
    const double ni = nok ? 1.0 / sqrt(nl2) : 0.0;
    const D3 rgb = swa != 0.0 ? (1.0 / swa) * cwa : (1.0 / W) * cw;
    // alpha-weighted area is conserved: sum a_i alpha_i (0 under the unit weights: every area is 0) over the parent's own area
    const double ap = sc1 * sc2;
    const double alpha = ap > 0.0 && isfinite(ap) ? fmin(1.0, (unit ? 0.0 : swa) / ap) : swa / W;
    o[0] = make_float4((float)(p1.x + mu.x), (float)(p1.y + mu.y), (float)(p1.z + mu.z), pos1.w);
    o[1] = make_float4((float)rgb.x, (float)rgb.y, (float)rgb.z, (float)alpha);
    o[2] = make_float4((float)sc1, (float)sc2, (float)sc3, scl1.w);
    o[3] = nok ? make_float4((float)(ns.x * ni), (float)(ns.y * ni), (float)(ns.z * ni), nrm1.w) : make_float4(0.0f, 0.0f, 0.0f, nrm1.w);
    o[4] = make_float4((float)qw, (float)qx, (float)qy, (float)qz);
    o[5] = make_float4((float)(pb0 / W), (float)(pb1 / W), pbr1.z, pbr1.w);
}

// Pin 5s: one walk over the members of a segment for one float4 column q of the SH plane.  kUnit: every weight is 1 (the areas add up to nothing).
// kGauss (pin 5sg): the weight is pin 5g's area, not sx sy.
// Every product and sum is fp64 in member order, without contraction.  The twelve lanes of a segment read the same alpha and scale words.
template <bool kUnit, bool kGauss>
__device__ __forceinline__ void merge_sh_walk(const float* __restrict__ rec, const float4* __restrict__ sh, const uint32_t* __restrict__ perm, uint32_t a,
                                              uint32_t b, uint32_t q, double& W, double& A, double (&sa)[4], double (&sw)[4]) {
    W = 0.0; A = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { sa[k] = 0.0; sw[k] = 0.0; }
    uint32_t i = perm[a];
    for (uint32_t j = a; j < b; ++j) {
        const uint32_t nxt = j + 1 < b ? perm[j + 1] : i;      // (the next member's index is on its way while this one's rows are)
        const float* g = rec + (size_t)i * 24;
        const float4 v = sh[(size_t)i * kMergeShLanes + q];
        const double w = kUnit ? 1.0 : kGauss ? gauss_area((double)g[8], (double)g[9], (double)g[10]) : (double)g[8] * (double)g[9];
        const double wa = w * (double)g[7];
        W += w;
        A += wa;
        sa[0] += wa * (double)v.x; sa[1] += wa * (double)v.y; sa[2] += wa * (double)v.z; sa[3] += wa * (double)v.w;
        sw[0] += w * (double)v.x; sw[1] += w * (double)v.y; sw[2] += w * (double)v.z; sw[3] += w * (double)v.w;
        i = nxt;
    }
}

// Pin 5s.  A row of the plane is twelve float4: lane t = (segment t / 12, column t % 12), no lane idle but the tail of the last
// workgroup.  Twelve against sixteen with four idle: a quarter fewer waves for the same bytes, at the price of a division by 12 per lane
// and of segments that straddle two waves, which costs nothing here — the lanes share no state.  A wave reads whole 192-byte rows
// through perm, 5 1/3 of them per load.  No atomics, a fixed order: the same bits from run to run.  out is not the memory sh points into.
// kGauss: the weights of pin 5sg.
template <bool kGauss>
__global__ void __launch_bounds__(kBlock) k_merge_reduce_sh(const float4* __restrict__ rec, const float4* __restrict__ sh, const uint32_t* __restrict__ perm,
                                                            const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ totals,
                                                            float4* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t s = (uint32_t)(t / kMergeShLanes), q = (uint32_t)(t - (uint64_t)s * kMergeShLanes);
    if (t / kMergeShLanes >= (uint64_t)totals[0]) return;
    const uint32_t a = seg_start[s], b = seg_start[s + 1];
    float4* o = out + (size_t)s * kMergeShLanes + q;
    if (b - a == 1u) {
        *o = sh[(size_t)perm[a] * kMergeShLanes + q];
        return;
    }
    double W, A, sa[4], sw[4];
    merge_sh_walk<false, kGauss>((const float*)rec, sh, perm, a, b, q, W, A, sa, sw);
    if (W == 0.0) merge_sh_walk<true, kGauss>((const float*)rec, sh, perm, a, b, q, W, A, sa, sw);   // (pin 5's own test; rare: a second walk, no second set of sums)
    const bool by_alpha = A != 0.0;
    const double den = by_alpha ? A : W;
    *o = make_float4((float)((by_alpha ? sa[0] : sw[0]) / den), (float)((by_alpha ? sa[1] : sw[1]) / den), (float)((by_alpha ? sa[2] : sw[2]) / den),
                     (float)((by_alpha ? sa[3] : sw[3]) / den));
}

size_t merge_scan_temp_bytes(uint32_t n) {
    size_t a = 0, b = 0;
    (void)rocprim::inclusive_scan(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, rocprim::maximum<uint32_t>(), (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, b, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, (size_t)n,
                                  rocprim::plus<unsigned long long>(), (hipStream_t)0);
    return a > b ? a : b;
}

hipError_t merge_segments(const float4* rec, const uint32_t* keys, const uint32_t* perm, uint32_t n, uint32_t level, uint32_t max_group, float min_axis_dot,
                          uint32_t* flag, uint32_t* run_start, unsigned long long* packed, unsigned long long* sums, uint32_t* seg_start, uint32_t* totals,
                          void* temp, size_t temp_bytes, bool unsigned_axis, bool gauss, hipStream_t st) {
    if (!n) return hipErrorInvalidValue;
    const dim3 grid((n + kBlock - 1) / kBlock);
    if (gauss) hipLaunchKernelGGL((k_merge_heads<true, true>), grid, dim3(kBlock), 0, st, rec, keys, perm, n, 3u * level, min_axis_dot, flag);
    else if (unsigned_axis) hipLaunchKernelGGL(k_merge_heads<true>, grid, dim3(kBlock), 0, st, rec, keys, perm, n, 3u * level, min_axis_dot, flag);
    else hipLaunchKernelGGL(k_merge_heads<false>, grid, dim3(kBlock), 0, st, rec, keys, perm, n, 3u * level, min_axis_dot, flag);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = rocprim::inclusive_scan(temp, temp_bytes, (const uint32_t*)flag, run_start, (size_t)n, rocprim::maximum<uint32_t>(), st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_merge_cuts, grid, dim3(kBlock), 0, st, (const uint32_t*)run_start, n, max_group, packed);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = rocprim::exclusive_scan(temp, temp_bytes, (const unsigned long long*)packed, sums, 0ull, (size_t)n, rocprim::plus<unsigned long long>(), st)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_merge_starts, grid, dim3(kBlock), 0, st, (const unsigned long long*)packed, (const unsigned long long*)sums, n, seg_start, totals);
    return hipGetLastError();
}

hipError_t merge_reduce(const float4* rec, const uint32_t* perm, const uint32_t* seg_start, const uint32_t* totals, uint32_t segments, float4* out,
                        uint32_t* map, bool unsigned_axis, hipStream_t st) {
    if (!segments) return hipSuccess;
    const dim3 grid((segments + kBlock - 1) / kBlock);
    if (unsigned_axis) hipLaunchKernelGGL(k_merge_reduce<true>, grid, dim3(kBlock), 0, st, rec, perm, seg_start, totals, out, map);
    else hipLaunchKernelGGL(k_merge_reduce<false>, grid, dim3(kBlock), 0, st, rec, perm, seg_start, totals, out, map);
    return hipGetLastError();
}

hipError_t merge_reduce_gauss(const float4* rec, const uint32_t* perm, const uint32_t* seg_start, const uint32_t* totals, uint32_t segments, float sigma,
                              float4* out, uint32_t* map, hipStream_t st) {
    if (!segments) return hipSuccess;
    const dim3 grid((segments + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_merge_reduce_gauss, grid, dim3(kBlock), 0, st, rec, perm, seg_start, totals, sigma, out, map);
    return hipGetLastError();
}

hipError_t merge_reduce_sh(const float4* rec, const float4* sh, const uint32_t* perm, const uint32_t* seg_start, const uint32_t* totals, uint32_t segments,
                           float4* out, bool gauss, hipStream_t st) {
    if (!segments) return hipSuccess;
    const uint64_t lanes = (uint64_t)segments * kMergeShLanes;
    const dim3 grid((uint32_t)((lanes + kBlock - 1) / kBlock));      // (below 2^28 workgroups for any 32-bit segment count)
    if (gauss) hipLaunchKernelGGL(k_merge_reduce_sh<true>, grid, dim3(kBlock), 0, st, rec, sh, perm, seg_start, totals, out);
    else hipLaunchKernelGGL(k_merge_reduce_sh<false>, grid, dim3(kBlock), 0, st, rec, sh, perm, seg_start, totals, out);
    return hipGetLastError();
}

}  // namespace m2s
