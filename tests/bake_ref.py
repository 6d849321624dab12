"""numpy restatement of m2s_bake_light / m2s_sh_shade_records (include/m2s.h): the yardstick of tests/test_bake_cpu.py and
tests/test_gpu_bake.py.  Nothing here reads the device's results.

  * ws is float32, operation by operation (it feeds decision arithmetic); the shadow counts are tests/light_ref.py's float32 restatement
    of computeShadowFactor taken at ws.
  * Everything else is float64 from those float32 inputs: the shader of light_ref.shade with the Gaussian's own normal, albedo,
    roughness and metallic, V = -d_k from the float32 table, projected with the float32 products w_k B_i(d_k) of the table.

The bar and why it holds.  Per record the 48 coefficients are held to tests/parity.py's vector rule with the absolute term the issue
sets: |gpu - ref| <= 1e-4 * max|ref| + 1e-6.  The device works in fp32 with v_log_f32 / v_exp_f32 / v_rsq_f32 (1 ulp each):
  - pow(x, y) = exp2(y log2 x) has a relative error of about (1 + |y log2 x| ln 2) ulp: <= 1e-6 for x >= 2^-10; every other operation
    is correctly rounded (6e-8).  One direction's colour L is a tone-mapped value in [0, 1) — d tone / d c = tone / (2.2 c (c + 1)) <=
    0.45 tone / c — so a relative error e of the linear colour moves L by at most 0.45 e: some 3e-7 for the ~10 operations of the diffuse
    path.
  - The specular lobe is the one ill-conditioned place: den = nh^2 (aa - 1) + 1 cancels to ~aa at the peak, so the 1.2e-7 absolute error
    of nh^2 becomes 1.2e-7 / aa relative in den and twice that in NDF.  At roughness >= 0.15 (aa >= 5e-4) that is <= 5e-4, i.e. <= 2.3e-4
    in L for the few directions inside the lobe; their weights sum |w B_i| are ~0.05 each: ~1e-5 in a coefficient, against a bar that is
    >= 1e-4 * |f_dc| ~ 3e-5 for such a record (a lit, glossy record is not mid-grey).  Roughness 0 makes aa = 0 and the term exactly 0.
    The random records therefore draw roughness from [0.15, 1] as tests/light_ref.random_gbuffer does, and 0 and 1 are planted.
  - A coefficient sums 128 products with sum_k |w_k B_i(d_k)| <= 4 pi C0 = 3.54 (i = 0) and ~2.9 above it.  Rounding errors of L are
    independent from direction to direction (3e-7 * 0.05 * sqrt(128) = 2e-7); errors COMMON to all directions (albedo^2.2, attenuation,
    n.l: <= 1e-6 relative) move every direction's L the same way, by <= 0.45e-6 tone, and f_dc by 3.54 times that: <= 1.6e-6 for a
    bright record, whose |f_dc| is of order one (bar ~1e-4).  A mid-grey record (f_dc ~ 0, bar 1e-6) has tone ~ 0.5: 8e-7, inside, but
    this is where the bar is tight, which is what the guard below watches.
  - The fp32 accumulation itself: 128 additions of terms <= 0.05, partial sums <= 3.54: <= 128 * 6e-8 * |partial| / 2 ~ 4e-7 worst case
    for f_dc of order one (bar 1e-4), ~1e-8 near zero.

ACHIEVED (the project's convention: the guard is 4x the measured maximum |gpu - ref| over every finite record of every case of
tests/test_gpu_bake.py, against THIS restatement, never the kernel against itself): 4.8e-6 for a coefficient (the largest error / bar
ratio of any record was 0.04), 1.7e-7 for a shaded colour; ACHIEVED_MAX_ABS below and DESIGN 5.13."""
import numpy as np

import light_ref as lr
from mesh2splat_amd import bake as bk

f32 = np.float32
# measured on MI355X over all cases of tests/test_gpu_bake.py (profiles/bake/gpu_tests.log): max |gpu - ref| of a coefficient (the
# 4 x 8 table on 257 records; 3.0e-6 with the default table on 1000) / of a shaded colour
ACHIEVED_MAX_ABS = {"sh": 4.8e-6, "shade": 1.7e-7}
GUARD = {k: 4.0 * v for k, v in ACHIEVED_MAX_ABS.items()}
RTOL, ATOL = 1e-4, 1e-6          # tests/parity.py's vector rule with the issue's absolute term


def world_positions(rec, M):
    """u_modelToWorld * vec4(P, 1) in float32, glm's association (m0 x + m1 y) + (m2 z + m3 w); M in glm's memory order (4, 4)."""
    m = np.ascontiguousarray(M, np.float32).reshape(4, 4)
    x, y, z = (rec[:, k].astype(np.float32) for k in range(3))
    with np.errstate(all="ignore"):
        return np.stack([(m[0, i] * x + m[1, i] * y) + (m[2, i] * z + m[3, i] * f32(1.0)) for i in range(3)], -1)


def world_normals(rec, M):
    """normalize((transpose(inverse(M)) * vec4(n, 1)).xyz) in float64 from the float32 matrix."""
    Mm = np.asarray(M, np.float64).reshape(4, 4).T          # math order
    T = np.linalg.inv(Mm).T
    n = rec[:, 12:15].astype(np.float64)
    with np.errstate(all="ignore"):
        nw = n @ T[:3, :3].T + T[:3, 3]
        return nw / np.sqrt((nw * nw).sum(-1, keepdims=True))


def _max0(v):
    return np.where(v > 0, v, np.where(np.isnan(v), v, 0.0))


def radiance(rec, M, light, table, counts, viewer_metallic=False):
    """L_c(V = -d_k) for every record and direction: (n, K, 3) float64, not clamped."""
    ws = world_positions(rec, M).astype(np.float64)
    N = world_normals(rec, M)[:, None, :]
    c = lambda v: np.float64(f32(v))                          # a float literal of the shader
    dot = lambda u, v: ((u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2])[..., None]
    norm = lambda v: v * (1.0 / np.sqrt(dot(v, v)))
    with np.errstate(all="ignore"):
        a = np.fmin(np.fmax(rec[:, 4:7].astype(np.float32), f32(0)), f32(1)).astype(np.float64)[:, None, :]
        rough = rec[:, 21].astype(np.float64)[:, None, None]
        metal = (np.zeros_like(rec[:, 20]) if viewer_metallic else rec[:, 20]).astype(np.float64)[:, None, None]
        shadow = counts.astype(np.float64)[:, None, None] / c(20.0)
        a = np.power(a, c(2.2))
        Lv = (np.asarray(light.light_position, np.float32).astype(np.float64) - ws)[:, None, :]
        d = np.sqrt(dot(Lv, Lv))
        L = norm(Lv)
        V = -table[None, :, 0:3].astype(np.float64)
        H = norm(V + L)
        att = 1.0 / (d * d)
        rad = (np.asarray(light.light_color, np.float32).astype(np.float64) * np.float64(f32(light.light_intensity))) * att
        im = 1.0 - metal
        F0 = c(0.04) * im + a * metal
        hv = _max0(dot(H, V))
        f5 = np.power(np.fmin(np.fmax(1.0 - hv, 0.0), 1.0), 5.0)
        F = F0 + (1.0 - F0) * f5
        aa = rough * rough
        aa = aa * aa
        nh = _max0(dot(N, H))
        den = (nh * nh) * (aa - 1.0) + 1.0
        den = ((c(22.0) / c(7.0)) * den) * den
        NDF = aa / den
        nv, nl = _max0(dot(N, V)), _max0(dot(N, L))
        rr = rough + 1.0
        kk = (rr * rr) / 8.0
        G = (nl / (nl * (1.0 - kk) + kk)) * (nv / (nv * (1.0 - kk) + kk))
        spec = ((NDF * G) * F) / ((4.0 * nv) * nl + c(0.0001))
        kD = (1.0 - F) * im
        Lo = ((((kD * a) / 22.0) / 7.0 + spec) * rad) * nl * (1.0 - shadow)
        col = c(0.3) * a + Lo
        col = col / (col + 1.0)
        return np.power(col, 1.0 / c(2.2))


def project(Lk, table, degree=3):
    """(n, K, 3) colours -> (n, 48) float64 planes: f_dc[3], f_rest[45] channel-major; coefficients above the degree 0."""
    wB = table[:, 4:20].astype(np.float64)
    with np.errstate(all="ignore"):
        sh = np.einsum("ki,nkc->nci", wB, Lk - 0.5)            # (n, 3, 16)
    sh[:, :, (degree + 1) ** 2:] = 0.0
    return np.concatenate([sh[:, :, 0], sh[:, :, 1:].reshape(sh.shape[0], 45)], 1)


def bake(rec, M, light, cube=None, degree=3, n_theta=0, n_phi=0, viewer_metallic=False):
    """-> (plane (n, 48) float64, counts (n,) uint8).  cube None: use_shadows = 0."""
    rec = np.ascontiguousarray(rec, np.float32)
    table = bk.quadrature_table(n_theta, n_phi)
    if cube is None:
        counts = np.zeros(rec.shape[0], np.uint8)
    else:
        counts = lr.shadow_counts(world_positions(rec, M), cube, light.light_position, light.far_plane)
    return project(radiance(rec, M, light, table, counts, viewer_metallic), table, degree), counts


def shade(rec, sh, M, cam):
    """m2s_sh_shade_records in float64: (n, 24) float64 records whose colour is max(0, 0.5 + sum sh_i B_i(dir)), NaN kept."""
    ws = world_positions(rec, M).astype(np.float64)
    with np.errstate(all="ignore"):
        v = ws - np.asarray(cam, np.float32).astype(np.float64)
        dirs = v / np.sqrt((v * v).sum(-1, keepdims=True))
        col = bk.eval_sh(np.asarray(sh, np.float64), dirs)
    out = np.asarray(rec, np.float64).copy()
    out[:, 4:7] = _max0(col)
    return out


def within_bar(got, ref):
    """per record: |got - ref| <= RTOL * max|ref| + ATOL over its finite vector -> (ok (n,), err (n,), tol (n,))"""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = RTOL * np.abs(r).max(-1) + ATOL
    err = np.abs(g - r).max(-1)
    return err <= tol, err, tol


def random_records(n, seed, M, light):
    """Seeded records in a box round the origin (model space), unit normals, albedo in [0, 1], roughness in [0.15, 1] (see the module
    docstring), metallic in [0, 1] — and, from n >= 16 on, the hostile ones in the first slots.  -> (records, hostile indices whose
    restatement may be non-finite)."""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 24), np.float32)
    r[:, 0:3] = rng.uniform(-1.5, 1.5, (n, 3))
    r[:, 3] = 1
    r[:, 4:7] = rng.uniform(0, 1, (n, 3))
    r[:, 7] = rng.uniform(0.2, 1, n)
    r[:, 8:11] = rng.uniform(0.005, 0.05, (n, 3))
    nn = rng.normal(size=(n, 3))
    r[:, 12:15] = nn / np.linalg.norm(nn, axis=-1, keepdims=True)
    q = rng.normal(size=(n, 4))
    r[:, 16:20] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    r[:, 20] = rng.uniform(0, 1, n)
    r[:, 21] = rng.uniform(0.15, 1, n)
    r[:, 23] = 1
    may_be_nonfinite = []
    if n >= 16:
        # a record AT the light: the model-space point whose float32 world position is the light's, found by inverting M in float64 and
        # checking the float32 product (the test's light position is chosen as the world position of this model point)
        r[0, 0:3] = AT_LIGHT_MODEL
        r[1, 12:15] = 0                                       # zero normal
        r[2, 12:15] = (np.nan, 0.2, 0.1)                      # NaN normal
        r[3, 21] = 0                                          # roughness 0
        r[4, 21] = 1                                          # roughness 1
        r[5, 20] = 0                                          # metallic 0
        r[6, 20] = 1                                          # metallic 1
        r[7, 4:7] = (-0.5, 1.7, 0.5)                          # albedo outside [0, 1]
        r[8, 4:7] = (0.0, 1.0, 2.0 ** -12)                    # albedo 0, 1 and tiny
        may_be_nonfinite = [0, 1, 2]
    return r, may_be_nonfinite


AT_LIGHT_MODEL = (0.25, 0.5, -0.125)      # exactly representable: the light of the GPU tests sits at M * this point (float32)


def cube_for(S, seed, light, far):
    """Depths round the distances of random_records' box from the light, so that the 20 taps disagree on many records."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.3, 4.5, (6, S, S)) / far).astype(np.float32)
