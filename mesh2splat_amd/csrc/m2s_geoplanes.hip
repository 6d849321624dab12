// m2s_geoplanes.hip — the geometry planes of an uploaded scene (gfx950): what a triangle's setup yields that does not depend on the
// resolution, computed once per upload and read by k_fused3's triangle phase (m2s_fused3.hip, the kGeo instances) in place of the positions.
//
// Per resident triangle, three float4 in three SoA planes (GeoPlanes, m2s_device.h; one coalesced 16-byte access per lane each):
//     G0 = Quaternion (w, x, y, z)                       geo_flat's rot
//     G1 = (Scale.x, Scale.y, ou[0], ov[0])              geo_flat's sx, sy; Geo::ou / ov: the box-normalised orthogonal UVs of geo_setup
//     G2 = (ou[1], ov[1], ou[2], ov[2])
// Inputs: the position planes and the mesh's box, both fixed at upload.  The kernel calls the device functions the conversion kernels
// call (geo_setup_mp, geo_flat: m2s_devfn.h, m2s_exact.h; contraction off, explicit fma_), so a plane word holds the bits k_fused3 would
// have computed: the fast and the IEEE forms of geo_setup's roots and quotients (chosen per wave, wave_all) agree bit for bit where the
// fast form is taken at all, and geo_flat's hardware roots and reciprocals depend on their operands only.  A triangle without area gets
// whatever that arithmetic gives (NaN, infinities): it covers no pixel, so no record reads its Scale or Quaternion, and raster_head
// rejects its ou / ov as it would have.
#include "m2s_device.h"
#include "m2s_devfn.h"

#pragma clang fp contract(off)

namespace m2s {

__global__ void __launch_bounds__(kBlock) k_geo_planes(SceneDev sc, float4* __restrict__ g0, float4* __restrict__ g1, float4* __restrict__ g2) {
    const uint32_t wave0 = (blockIdx.x * (uint32_t)kBlock + (threadIdx.x & ~63u));   // first triangle of the wave: a multiple of 64
    if (wave0 >= sc.n_tri) return;
    const uint32_t t = wave0 + (threadIdx.x & 63u);
    bool uniform_mesh = false;
    const uint32_t m0 = mesh_of_range(sc, wave0, min(wave0 + 64u, sc.n_tri) - 1u, uniform_mesh);
    if (t >= sc.n_tri) return;
    float p[9];
    Geo g;
    load_positions(sc.tri, t, p);
    if (uniform_mesh) geo_setup_mp(p, kConstMesh(sc.meshes + m0), g);
    else geo_setup_mp(p, sc.meshes + find_mesh(sc, sc.tri_first + t), g);
    float sx, sy;
    float4 rot;
    geo_flat(p, g, sx, sy, rot);
    g0[t] = rot;
    g1[t] = make_float4(sx, sy, g.ou[0], g.ov[0]);
    g2[t] = make_float4(g.ou[1], g.ov[1], g.ou[2], g.ov[2]);
}

void launch_geo_planes(const SceneDev& sc, float4* g0, float4* g1, float4* g2, hipStream_t st) {
    if (sc.n_tri) hipLaunchKernelGGL(k_geo_planes, dim3((sc.n_tri + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, g0, g1, g2);
}

}  // namespace m2s
