"""The point light baked into the spherical harmonics of the standard 3DGS .ply (`Converter.bake_light`, m2s_bake_light): parameters,
the quadrature table and the basis.  The table is built by the SAME sequence of double-precision operations as
csrc/m2s_bake.cpp (gauss_legendre, azimuths, build_table) and csrc/m2s_shbasis.h, so both sides hold the same bits
(tests/test_bake_cpu.py compares them with m2s_bake_directions)."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)
TABLE_ROW = 20                  # floats per direction: d.xyz, w, w * B_0..15
ALLOWED_THETA, ALLOWED_PHI = (4, 8), (8, 16)
SH_FLOATS = 48                  # per record: f_dc[3], f_rest[45] channel-major


def _eye() -> np.ndarray:
    return np.eye(4, dtype=np.float32)


@dataclass
class BakeParams:
    model_mat: np.ndarray = field(default_factory=_eye)   # u_modelToWorld, glm's memory order (m[c] is column c), as PrepassParams
    degree: int = 3                                       # 0..3: coefficients above it are written as +0.0
    n_theta: int = 0                                      # 4 | 8 Gauss-Legendre nodes (0: 8)
    n_phi: int = 0                                        # 8 | 16 azimuths (0: 16)
    use_shadows: bool = True                              # False: shadow factor 0, no cube needed
    viewer_metallic: bool = False                         # True: metallic 0, as the viewer's frame (its shader reads an always-zero channel)
    want_shadow_counts: bool = False                      # also keep the per-record count of shadowed taps


class BakeParamsC(C.Structure):
    """== m2s_bake_params (include/m2s.h)."""
    _fields_ = [("model_to_world", C.c_float * 16), ("degree", C.c_uint32), ("n_theta", C.c_uint32), ("n_phi", C.c_uint32),
                ("use_shadows", C.c_uint32), ("viewer_metallic", C.c_uint32), ("want_shadow_counts", C.c_uint32), ("reserved", C.c_uint32)]


def to_c(p: BakeParams) -> BakeParamsC:
    c = BakeParamsC()
    c.model_to_world[:] = np.ascontiguousarray(p.model_mat, np.float32).reshape(16).tolist()
    c.degree, c.n_theta, c.n_phi = int(p.degree), int(p.n_theta), int(p.n_phi)
    c.use_shadows = 1 if p.use_shadows else 0
    c.viewer_metallic = 1 if p.viewer_metallic else 0
    c.want_shadow_counts = 1 if p.want_shadow_counts else 0
    c.reserved = 0
    return c


def sh_basis(dirs) -> np.ndarray:
    """B_0..15 of (..., 3) directions -> (..., 16), in the dtype of `dirs` (float64 unless it is float32), the operation order of
    csrc/m2s_shbasis.h."""
    d = np.asarray(dirs)
    dt = np.float32 if d.dtype == np.float32 else np.float64
    d = d.astype(dt)
    k = dt
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    B = np.empty(d.shape[:-1] + (16,), dt)
    B[..., 0] = k(C0)
    B[..., 1] = -k(C1) * y
    B[..., 2] = k(C1) * z
    B[..., 3] = -k(C1) * x
    B[..., 4] = k(C2[0]) * xy
    B[..., 5] = k(C2[1]) * yz
    B[..., 6] = k(C2[2]) * ((k(2) * zz - xx) - yy)
    B[..., 7] = k(C2[3]) * xz
    B[..., 8] = k(C2[4]) * (xx - yy)
    B[..., 9] = k(C3[0]) * (y * (k(3) * xx - yy))
    B[..., 10] = k(C3[1]) * (xy * z)
    B[..., 11] = k(C3[2]) * (y * ((k(4) * zz - xx) - yy))
    B[..., 12] = k(C3[3]) * (z * ((k(2) * zz - k(3) * xx) - k(3) * yy))
    B[..., 13] = k(C3[4]) * (x * ((k(4) * zz - xx) - yy))
    B[..., 14] = k(C3[5]) * (z * (xx - yy))
    B[..., 15] = k(C3[6]) * (x * (xx - k(3) * yy))
    return B


def gauss_legendre(n: int):
    """n nodes in z, descending, and their weights (python floats): csrc/m2s_bake.cpp gauss_legendre, line for line."""
    guess = {4: (0.8611, 0.3400), 8: (0.9603, 0.7967, 0.5255, 0.1834)}[n]
    z, w = [0.0] * n, [0.0] * n
    for r in range(n // 2):
        x, dp = guess[r], 0.0
        for it in range(6):
            p0, p1 = 1.0, x
            for k in range(2, n + 1):
                pk = (((2.0 * k - 1.0) * x) * p1 - (k - 1.0) * p0) / k
                p0, p1 = p1, pk
            dp = (n * (x * p1 - p0)) / (x * x - 1.0)
            if it == 5:
                break
            x = x - p1 / dp
        wt = 2.0 / ((1.0 - x * x) * (dp * dp))
        z[r], w[r] = x, wt
        z[n - 1 - r], w[n - 1 - r] = -x, wt
    return z, w


def azimuths(n_phi: int):
    """cos / sin of 2 pi (j + 0.5) / n_phi from the first quadrant's cosines (literals, as in csrc/m2s_bake.cpp)."""
    Q = {8: (0.9238795325112867, 0.3826834323650898),
         16: (0.9807852804032304, 0.8314696123025452, 0.5555702330196022, 0.19509032201612825)}[n_phi]
    h = n_phi // 4
    cs, sn = [], []
    for j in range(n_phi):
        q, k = divmod(j, h)
        c, s = Q[k], Q[h - 1 - k]
        cs.append((c, -s, -c, s)[q])
        sn.append((s, c, -s, -c)[q])
    return cs, sn


def quadrature(n_theta: int = 0, n_phi: int = 0):
    """-> (dirs (n, 3), weights (n,)) in float64 BEFORE the rounding to float; row t * n_phi + j."""
    n_theta, n_phi = n_theta or 8, n_phi or 16
    if n_theta not in ALLOWED_THETA or n_phi not in ALLOWED_PHI:
        raise ValueError("n_theta must be 4 or 8 and n_phi 8 or 16")
    z, wz = gauss_legendre(n_theta)
    cs, sn = azimuths(n_phi)
    wphi = (2.0 * 3.141592653589793) / float(n_phi)
    dirs, wts = [], []
    for t in range(n_theta):
        st = math.sqrt(1.0 - z[t] * z[t])
        w = wz[t] * wphi
        for j in range(n_phi):
            dirs.append((st * cs[j], st * sn[j], z[t]))
            wts.append(w)
    return np.array(dirs, np.float64), np.array(wts, np.float64)


def quadrature_table(n_theta: int = 0, n_phi: int = 0) -> np.ndarray:
    """The table k_bake_sh reads: (n_theta * n_phi, 20) float32 rows d.xyz, w, w * B_0..15(d) — double, rounded once."""
    dirs, wts = quadrature(n_theta, n_phi)
    tab = np.empty((dirs.shape[0], TABLE_ROW), np.float64)
    tab[:, 0:3] = dirs
    tab[:, 3] = wts
    tab[:, 4:] = wts[:, None] * sh_basis(dirs)
    return tab.astype(np.float32)


def eval_sh(sh: np.ndarray, dirs: np.ndarray) -> np.ndarray:
    """colour (n, 3) float64 a standard 3DGS viewer shows of (n, 48) planes along (n, 3) unit directions, before its max(0, .)."""
    sh = np.asarray(sh, np.float64)
    B = sh_basis(np.asarray(dirs, np.float64))
    out = np.empty((sh.shape[0], 3))
    for c in range(3):
        out[:, c] = 0.5 + sh[:, c] * B[:, 0] + (sh[:, 3 + 15 * c:18 + 15 * c] * B[:, 1:]).sum(-1)
    return out
