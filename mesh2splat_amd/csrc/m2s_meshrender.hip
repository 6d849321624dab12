// m2s_meshrender.hip — the shading stage of the mesh render pass (MeshRenderPass.cpp:8-73, meshRender{VS,PS}.glsl): the source mesh
// drawn into a second five-target G-buffer, which m2s_relight_split puts left of the split screen's divider.  The visibility stage is
// the mesh depth prepass's kernels with a 64-bit payload (m2s_meshdepth.hip, kVis): it leaves, per pixel, (bits of z) << 32 | global
// index of the triangle GL_LESS would have kept.  The semantics are the ones include/m2s.h pins (m2s_mesh_render);
// tests/meshrender_ref.py restates them in numpy.
//
//   k_mr_shade   one lane per pixel.  An empty pixel writes zeros to the five planes (the pass's clear).  Any other loads the winner's
//                three corners, recomputes their clip positions (the visibility stage's function: same bits), and takes the
//                barycentrics of the ORIGINAL triangle in homogeneous form, in fp64 — a clipped triangle needs no piece, and a sub-pixel
//                one does not cancel.  The same function at the centres of (x + 1, y) and (x, y + 1) gives the UV differences a helper
//                invocation would see; lod_from_grad and the conversion's software sampler take it from there.  The vertex shader's
//                varyings are recomputed per corner (three corners per pixel: 36 B of positions, 24 B of UV and 84 B of normals and
//                tangents, all from L2 for neighbouring pixels of one triangle).
#include "m2s_devfn.h"
#include "m2s_viewmath.h"

#pragma clang fp contract(off)

namespace m2s {

namespace {

constexpr uint32_t kOne = 0x3F800000u;

__device__ __forceinline__ uint32_t half_bits(float v) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)v); }      // RNE, overflow to inf
__device__ __forceinline__ uint2 half4(float x, float y, float z, float w) {
    return make_uint2(half_bits(x) | (half_bits(y) << 16), half_bits(z) | (half_bits(w) << 16));
}
__device__ __forceinline__ uint32_t q8(float c) { return c == c ? (uint32_t)rintf(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f) : 0u; }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
// value arithmetic: v * rsq(|v|^2) with the device's fast reciprocal square root
__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
    const float r = fast_rsq((x * x + y * y) + z * z);
    x *= r; y *= r; z *= r;
}
// glm's mat3 * vec3
__device__ __forceinline__ void m3_mul(const float* m, float x, float y, float z, float& ox, float& oy, float& oz) {
    ox = (m[0] * x + m[3] * y) + m[6] * z;
    oy = (m[1] * x + m[4] * y) + m[7] * z;
    oz = (m[2] * x + m[5] * y) + m[8] * z;
}
// fract(sin(x) * 43758.5453): the sine in fp64 of the fp32 argument, rounded to fp32 (the product amplifies any error of it)
__device__ __forceinline__ float hash_fract(float x) {
    const float v = (float)sin((double)x) * 43758.5453f;
    return v - floorf(v);
}

// The homogeneous edge functions of the triangle with clip positions (x, y, w): e_i(n) = (n.x A_i - n.y B_i) + C_i
struct Homog { double A[3], B[3], C[3]; };
__device__ __forceinline__ void homog_setup(const float4 (&c)[3], Homog& g) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        const double xj = c[j].x, yj = c[j].y, wj = c[j].w, xk = c[k].x, yk = c[k].y, wk = c[k].w;
        g.A[i] = yj * wk - wj * yk;
        g.B[i] = xj * wk - wj * xk;
        g.C[i] = xj * yk - yj * xk;
    }
}
// lambda at the centre of pixel (x, y): fp64 throughout, rounded to fp32 at the end
__device__ __forceinline__ void homog_bary(const Homog& g, int x, int y, int W, int H, float (&l)[3]) {
    const double nx = (double)(2 * x + 1) / (double)W - 1.0, ny = (double)(2 * y + 1) / (double)H - 1.0;
    const double e0 = (nx * g.A[0] - ny * g.B[0]) + g.C[0], e1 = (nx * g.A[1] - ny * g.B[1]) + g.C[1], e2 = (nx * g.A[2] - ny * g.B[2]) + g.C[2];
    const double s = (e0 + e1) + e2;
    l[0] = (float)(e0 / s); l[1] = (float)(e1 / s); l[2] = (float)(e2 / s);
}
__device__ __forceinline__ float lerp3(const float (&l)[3], float a0, float a1, float a2) { return (l[0] * a0 + l[1] * a1) + l[2] * a2; }

// texture(map, uv) of one map with the implicit LOD of the pass: levels 0..4, REPEAT, the conversion's sampler unchanged
template <int NCH>
__device__ __forceinline__ void sample_map(const TexDesc* t, float uf, float vf, float dudx, float dvdx, float dudy, float dvdy, bool finite_grad, float (&out)[NCH]) {
    float lam = lod_from_grad((float)t->w, (float)t->h, dudx, dvdx, dudy, dvdy);
    if (!finite_grad) lam = __builtin_inff();             // a non-finite rho: the last level
    TexState st;
    TexFetch tf;
    tex_state(t, uf, vf, lam, st);
    tex_issue(t->texels, st, tf);
    tex_finish<NCH>(tf, st, out);
}

__global__ void __launch_bounds__(256) k_mr_shade(const MeshRenderK k, const SceneDev sc, const unsigned long long* __restrict__ vis,
                                                  uint2* __restrict__ g_pos, uint2* __restrict__ g_nrm, uint32_t* __restrict__ g_alb,
                                                  uint2* __restrict__ g_dep, uint32_t* __restrict__ g_mr) {
    const size_t px = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (px >= (size_t)k.W * (size_t)k.H) return;
    const unsigned long long key = vis[px];
    const uint32_t gt = (uint32_t)key;
    const uint32_t t = gt - sc.tri_first;
    if ((uint32_t)(key >> 32) >= kOne || t >= sc.n_tri) {      // empty: glClear(0, 0, 0, 0)
        g_pos[px] = g_nrm[px] = g_dep[px] = make_uint2(0u, 0u);
        g_alb[px] = g_mr[px] = 0u;
        return;
    }
    const int x = (int)(px % (size_t)k.W), y = (int)(px / (size_t)k.W);
    const uint2 mo = sc.mesh_of8[t >> 3];
    const uint32_t mesh = t < mo.y ? mo.x : find_mesh(sc, gt);
    const MeshParams* mp = sc.meshes + mesh;
    float p[9];
    load_positions(sc.tri, t, p);
    const float4 b0 = ld_plane(sc.tri.B0, t);
    const float2 b1 = ld_plane(sc.tri.B1, t);
    float4 c[3];
#pragma unroll
    for (int v = 0; v < 3; ++v) c[v] = m4_mul(k.PVM, p[3 * v], p[3 * v + 1], p[3 * v + 2], 1.0f);
    Homog g;
    homog_setup(c, g);
    float l[3], lx[3], ly[3];
    homog_bary(g, x, y, k.W, k.H, l);
    homog_bary(g, x + 1, y, k.W, k.H, lx);
    homog_bary(g, x, y + 1, k.W, k.H, ly);
    const float U = lerp3(l, b0.x, b0.z, b1.x), V = lerp3(l, b0.y, b0.w, b1.y);
    const float dudx = lerp3(lx, b0.x, b0.z, b1.x) - U, dvdx = lerp3(lx, b0.y, b0.w, b1.y) - V;
    const float dudy = lerp3(ly, b0.x, b0.z, b1.x) - U, dvdy = lerp3(ly, b0.y, b0.w, b1.y) - V;
    const bool fin = isfinite(dudx) && isfinite(dvdx) && isfinite(dudy) && isfinite(dvdy);
    const float uf = frac_repeat(U), vf = frac_repeat(V);

    // the textures first: their reads are the long latency of the lane
    const TexDesc* ta = &mp->tex[0];
    const TexDesc* tn = &mp->tex[1];
    const TexDesc* tm = &mp->tex[2];
    float alb[3] = { mp->color[0], mp->color[1], mp->color[2] };
    if (ta->texels != nullptr) {
        float s[3];
        sample_map<3>(ta, uf, vf, dudx, dvdx, dudy, dvdy, fin, s);
        alb[0] *= s[0]; alb[1] *= s[1]; alb[2] *= s[2];
    }
    float metal = 0.1f, rough = 0.5f;
    if (tm->texels != nullptr) {
        float s[3];
        sample_map<3>(tm, uf, vf, dudx, dvdx, dudy, dvdy, fin, s);
        metal = s[2]; rough = s[1];                          // .bg
    }

    // the vertex shader's varyings, per corner, then sum(lambda_i a_i) in fixed order
    const float4 n0 = ld_plane(sc.tri.C0, t), n1 = ld_plane(sc.tri.C1, t);
    const float n2 = ld_plane(sc.tri.C2, t);
    const float nin[9] = { n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w, n2 };
    float ws[3][3], vn[3][3], vd[3];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const float4 w4 = m4_mul(k.M, p[3 * v], p[3 * v + 1], p[3 * v + 2], 1.0f);
        ws[v][0] = w4.x; ws[v][1] = w4.y; ws[v][2] = w4.z;
        vd[v] = -m4_mul(k.V, w4.x, w4.y, w4.z, w4.w).z;
        m3_mul(k.N, nin[3 * v], nin[3 * v + 1], nin[3 * v + 2], vn[v][0], vn[v][1], vn[v][2]);
        normalize3(vn[v][0], vn[v][1], vn[v][2]);
    }
    const float wx = lerp3(l, ws[0][0], ws[1][0], ws[2][0]), wy = lerp3(l, ws[0][1], ws[1][1], ws[2][1]), wz = lerp3(l, ws[0][2], ws[1][2], ws[2][2]);
    const float view_depth = lerp3(l, vd[0], vd[1], vd[2]);
    float Nx = lerp3(l, vn[0][0], vn[1][0], vn[2][0]), Ny = lerp3(l, vn[0][1], vn[1][1], vn[2][1]), Nz = lerp3(l, vn[0][2], vn[1][2], vn[2][2]);
    normalize3(Nx, Ny, Nz);
    if (tn->texels != nullptr) {
        float s[3];
        sample_map<3>(tn, uf, vf, dudx, dvdx, dudy, dvdy, fin, s);
        float mx = s[0] * 2.0f - 1.0f, my = s[1] * 2.0f - 1.0f, mz = s[2] * 2.0f - 1.0f;
        normalize3(mx, my, mz);
        const float4 d[3] = { ld_plane(sc.tri.D0, t), ld_plane(sc.tri.D1, t), ld_plane(sc.tri.D2, t) };
        float vt[3][3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            m3_mul(k.N, d[v].x, d[v].y, d[v].z, vt[v][0], vt[v][1], vt[v][2]);
            normalize3(vt[v][0], vt[v][1], vt[v][2]);
        }
        float Tx = lerp3(l, vt[0][0], vt[1][0], vt[2][0]), Ty = lerp3(l, vt[0][1], vt[1][1], vt[2][1]), Tz = lerp3(l, vt[0][2], vt[1][2], vt[2][2]);
        const float Tw = lerp3(l, d[0].w, d[1].w, d[2].w);
        normalize3(Tx, Ty, Tz);
        float Bx = Ny * Tz - Nz * Ty, By = Nz * Tx - Nx * Tz, Bz = Nx * Ty - Ny * Tx;      // cross(N, T)
        normalize3(Bx, By, Bz);
        Bx *= Tw; By *= Tw; Bz *= Tw;
        const float ox = (Tx * mx + Bx * my) + Nx * mz, oy = (Ty * mx + By * my) + Ny * mz, oz = (Tz * mx + Bz * my) + Nz * mz;   // TBN * mapped
        Nx = ox; Ny = oy; Nz = oz;
        normalize3(Nx, Ny, Nz);
    }
    const float e0 = Nx * 0.5f + 0.5f, e1 = Ny * 0.5f + 0.5f, e2 = Nz * 0.5f + 0.5f;             // encodeNormal
    const float nd = (view_depth - k.near_far[0]) / (k.near_far[1] - k.near_far[0]);          // computeExponentialDepth
    const float cd = clamp01(__expf(-20.0f * clamp01(nd)));
    float o0 = alb[0], o1 = alb[1], o2 = alb[2];                                               // modes 0, 6, 5 (and any other): albedo
    if (k.mode == 1) { o0 = o1 = o2 = cd; }
    else if (k.mode == 2) { o0 = e0; o1 = e1; o2 = e2; }
    else if (k.mode == 3) {
        const float id = (float)(gt - sc.mesh_first[mesh]);                                    // gl_PrimitiveID: one draw per mesh
        o0 = hash_fract(id * 311.7f);
        o1 = hash_fract(id * 269.5f + 1.3f);
        o2 = hash_fract(id * 183.3f + 2.7f);
    } else if (k.mode == 4) { o0 = 0.01f; o1 = 0.005f; o2 = 0.0f; }
    g_pos[px] = half4(wx, wy, wz, 1.0f);
    g_nrm[px] = half4(e0, e1, e2, 1.0f);
    g_alb[px] = q8(o0) | (q8(o1) << 8) | (q8(o2) << 16) | 0xFF000000u;
    g_dep[px] = half4(cd, cd, cd, 1.0f);
    g_mr[px] = q8(metal) | (q8(rough) << 8) | 0xFF000000u;
}

}  // namespace

hipError_t meshrender_shade(const MeshRenderK& k, const SceneDev& sc, const unsigned long long* vis, void* const planes[5], hipStream_t st) {
    const size_t px = (size_t)k.W * (size_t)k.H;
    hipLaunchKernelGGL(k_mr_shade, dim3((uint32_t)((px + 255u) / 256u)), dim3(256), 0, st, k, sc, vis, (uint2*)planes[0], (uint2*)planes[1],
                       (uint32_t*)planes[2], (uint2*)planes[3], (uint32_t*)planes[4]);
    return hipGetLastError();
}

hipError_t preload_meshrender() { hipFuncAttributes a; return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_mr_shade)); }

}  // namespace m2s
