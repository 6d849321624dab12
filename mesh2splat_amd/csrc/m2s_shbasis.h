// m2s_shbasis.h — the 16 real spherical harmonics of the 3DGS format, with the sign convention of its viewers
// (colour(dir) = 0.5 + sum_i sh_i B_i(dir)), written once for the host (double: the quadrature table of m2s_bake_light) and the device
// (float: k_sh_shade).  The operation order below IS the pin (include/m2s.h, m2s_bake_light); mesh2splat_amd/bake.py repeats it.
#pragma once
#include <hip/hip_runtime.h>

namespace m2s {

template <typename T>
__host__ __device__ inline void sh_basis(T x, T y, T z, T B[16]) {
    const T C0 = (T)0.28209479177387814, C1 = (T)0.4886025119029199;
    const T C2[5] = { (T)1.0925484305920792, (T)-1.0925484305920792, (T)0.31539156525252005, (T)-1.0925484305920792, (T)0.5462742152960396 };
    const T C3[7] = { (T)-0.5900435899266435, (T)2.890611442640554, (T)-0.4570457994644658, (T)0.3731763325901154, (T)-0.4570457994644658,
                      (T)1.445305721320277,  (T)-0.5900435899266435 };
    const T xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    B[0] = C0;
    B[1] = -C1 * y;
    B[2] = C1 * z;
    B[3] = -C1 * x;
    B[4] = C2[0] * xy;
    B[5] = C2[1] * yz;
    B[6] = C2[2] * (((T)2 * zz - xx) - yy);
    B[7] = C2[3] * xz;
    B[8] = C2[4] * (xx - yy);
    B[9] = C3[0] * (y * ((T)3 * xx - yy));
    B[10] = C3[1] * (xy * z);
    B[11] = C3[2] * (y * (((T)4 * zz - xx) - yy));
    B[12] = C3[3] * (z * (((T)2 * zz - (T)3 * xx) - (T)3 * yy));
    B[13] = C3[4] * (x * (((T)4 * zz - xx) - yy));
    B[14] = C3[5] * (z * (xx - yy));
    B[15] = C3[6] * (x * (xx - (T)3 * yy));
}

}  // namespace m2s
