"""Test infrastructure: a numpy restatement of the shadow and relighting passes exactly as include/m2s.h pins them (m2s_shadow,
m2s_relight).  Not imported by the product.

Where the header pins operations (stage A of the shadow pass, the depth d, coverage, the cube lookup, the 20-tap shadow count)
every fp32 operation is one numpy float32 operation (numpy does not fuse) and edge functions are int64 — coverage goes through
splat_ref.setup (snapping, guard band, edges, boxes) with the 48-byte shadow quad padded to the 24-float layout.  The value
arithmetic of render mode 6 is evaluated in a dtype of the caller's choice: float64 (rounded once at the end) is the reference,
float32 tells which pixels are ill-conditioned.  The restatement never takes a shortcut the kernels take."""
from __future__ import annotations

import numpy as np

import splat_ref as sr

f32 = np.float32
FACE_F = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))          # GaussianShadowPass.cpp:91-108
FACE_UP = ((0, -1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, -1, 0), (0, -1, 0))
OFFSETS = ((1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, 1), (1, 1, -1), (1, -1, -1), (-1, -1, -1), (-1, 1, -1),
           (1, 1, 0), (1, -1, 0), (-1, -1, 0), (-1, 1, 0), (1, 0, 1), (-1, 0, 1), (1, 0, -1), (-1, 0, -1),
           (0, 1, 1), (0, -1, 1), (0, -1, -1), (0, 1, -1))                                # gaussianSplattingDeferredPS.glsl:72-79


def default_light(bbox_min, bbox_max):
    """The CLI's default light (tools/mesh2splat_cli.cpp: preview_light), in double: above and to the right of the preview camera's
    side of the scene, at 1.5 bounding-sphere radii from the centre; intensity = 4 radius^2.  -> (position (3,), intensity)"""
    mn, mx = np.asarray(bbox_min, np.float64), np.asarray(bbox_max, np.float64)
    ctr = (mn + mx) / 2
    d2 = 0.0
    for k in range(3):
        d2 += (mx[k] - mn[k]) * (mx[k] - mn[k])
    radius = np.sqrt(d2) / 2
    pos = np.array([ctr[0] + 0.75 * radius, ctr[1] + 0.75 * radius, ctr[2] + 1.5 * radius])
    return pos, 4.0 * radius * radius


def shadow_cameras(light, near, far):
    """-> (views (6, 16) float32, proj (16,) float32), column-major like glm: the header's pin (double, rounded to float)."""
    eye = np.asarray(light, np.float32).astype(np.float64)
    views = np.zeros((6, 16), np.float32)
    for fc in range(6):
        f, up = np.array(FACE_F[fc], np.float64), np.array(FACE_UP[fc], np.float64)
        s = np.array([f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]])
        u = np.array([s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]])
        m = np.zeros(16)
        m[15] = 1
        for k in range(3):
            m[k * 4 + 0], m[k * 4 + 1], m[k * 4 + 2] = s[k], u[k], -f[k]
        with np.errstate(all="ignore"):
            m[12] = -((s[0] * eye[0] + s[1] * eye[1]) + s[2] * eye[2])
            m[13] = -((u[0] * eye[0] + u[1] * eye[1]) + u[2] * eye[2])
            m[14] = (f[0] * eye[0] + f[1] * eye[1]) + f[2] * eye[2]
        views[fc] = (m + 0.0).astype(np.float32)
    n, f = float(f32(near)), float(f32(far))
    proj = np.zeros(16, np.float32)
    with np.errstate(all="ignore"):
        proj[0] = proj[5] = 1.0
        proj[10] = f32(-(f + n) / (f - n))
        proj[11] = -1.0
        proj[14] = f32(-(2.0 * f * n) / (f - n))
    return views, proj


def _m4_mul(m, x, y, z, w):
    """mat4 * vec4 in glm's association; m: sequence of 16 (scalars or per-record arrays)."""
    return [(m[0 + i] * x + m[4 + i] * y) + (m[8 + i] * z + m[12 + i] * w) for i in range(4)]


def _m3_mul(a, b):
    return [[(a[0][i] * b[c][0] + a[1][i] * b[c][1]) + a[2][i] * b[c][2] for i in range(3)] for c in range(3)]


def _m3_t(a):
    return [[a[i][c] for i in range(3)] for c in range(3)]


def _min_glsl(a, b):
    return np.where(b < a, b, a)


def shadow_quads(records, model, resolution, near_far, gaussian_std, resolution_target, fmt, light, light_near_far, masks=False):
    """Stage A.  -> list of six (n_f, 12) float32 arrays, each in input order; with masks=True also (face, passes the 1.05 w test,
    passes the lambda2 test) per record."""
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, 24)
    n = rec.shape[0]
    M = [f32(v) for v in np.asarray(model, np.float32).reshape(16)]
    views, proj = shadow_cameras(light, *light_near_far)
    L = [f32(v) for v in np.asarray(light, np.float32)]
    one, zero = f32(1.0), np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        # uniforms (m2s_prepass.hip: prepass_prepare): inverse(mat3(M)), the model scale as written, u_stdDev
        def A(c, r):
            return M[c * 4 + r]
        ood = one / ((A(0, 0) * (A(1, 1) * A(2, 2) - A(2, 1) * A(1, 2)) - A(1, 0) * (A(0, 1) * A(2, 2) - A(2, 1) * A(0, 2))) +
                     A(2, 0) * (A(0, 1) * A(1, 2) - A(1, 1) * A(0, 2)))
        mri = [[None] * 3 for _ in range(3)]            # [col][row]
        mri[0][0] = (A(1, 1) * A(2, 2) - A(2, 1) * A(1, 2)) * ood
        mri[1][0] = -(A(1, 0) * A(2, 2) - A(2, 0) * A(1, 2)) * ood
        mri[2][0] = (A(1, 0) * A(2, 1) - A(2, 0) * A(1, 1)) * ood
        mri[0][1] = -(A(0, 1) * A(2, 2) - A(2, 1) * A(0, 2)) * ood
        mri[1][1] = (A(0, 0) * A(2, 2) - A(2, 0) * A(0, 2)) * ood
        mri[2][1] = -(A(0, 0) * A(2, 1) - A(2, 0) * A(0, 1)) * ood
        mri[0][2] = (A(0, 1) * A(1, 2) - A(1, 1) * A(0, 2)) * ood
        mri[1][2] = -(A(0, 0) * A(1, 2) - A(1, 0) * A(0, 2)) * ood
        mri[2][2] = (A(0, 0) * A(1, 1) - A(1, 0) * A(0, 1)) * ood
        l0 = np.sqrt((M[0] * M[0] + M[1] * M[1]) + (M[2] * M[2] + M[3] * M[3]))
        l1 = np.sqrt((M[4] * M[4] + M[5] * M[5]) + (M[6] * M[6] + M[7] * M[7]))
        ms2 = [l0 * l0, l0 * l0, l1 * l1]
        std_dev = f32(gaussian_std) / f32(resolution_target)
        res = [f32(resolution[0]), f32(resolution[1])]
        nf = [f32(near_far[0]), f32(near_far[1])]
        # :80, :58-69
        ws = _m4_mul(M, rec[:, 0], rec[:, 1], rec[:, 2], one)
        dx, dy, dz = ws[0] - L[0], ws[1] - L[1], ws[2] - L[2]
        ln = np.sqrt((dx * dx + dy * dy) + dz * dz)
        nx, ny, nz = dx / ln, dy / ln, dz / ln
        ax, ay, az = np.abs(nx), np.abs(ny), np.abs(nz)
        cx = (ax >= ay) & (ax >= az)
        cy = (ay >= ax) & (ay >= az)
        face = np.where(cx, np.where(nx > 0, 0, 1), np.where(cy, np.where(ny > 0, 2, 3), np.where(nz > 0, 4, 5)))
        V = [views[face, i] for i in range(16)]
        vs = _m4_mul(V, ws[0], ws[1], ws[2], one)                                   # :85
        p2 = _m4_mul([f32(v) for v in proj], vs[0], vs[1], vs[2], vs[3])            # :87
        clip = f32(1.05) * p2[3]
        clip_ok = ~((p2[2] < -clip) | (p2[0] < -clip) | (p2[0] > clip) | (p2[1] < -clip) | (p2[1] > clip))   # :89-94
        # :96-112
        mult = std_dev if fmt in (0, 3) else one
        scale = [(rec[:, 8 + k] * mult) * ms2[k] for k in range(3)]
        x, y, z, w = rec[:, 16], rec[:, 17], rec[:, 18], rec[:, 19]
        two = f32(2.0)
        rot = [[one - two * (z * z + w * w), two * (y * z - x * w), two * (y * w + x * z)],
               [two * (y * z + x * w), one - two * (y * y + w * w), two * (z * w - x * y)],
               [two * (y * w - x * z), two * (z * w + x * y), one - two * (y * y + z * z)]]
        rot = _m3_mul(rot, mri)
        sm = [[scale[c] if c == i else zero for i in range(3)] for c in range(3)]
        mm = _m3_mul(sm, rot)
        cov3d = _m3_mul(_m3_t(mm), mm)
        pos2d = [p2[0] / p2[3], p2[1] / p2[3], p2[2] / p2[3], p2[3]]                # :153
        # :160-196
        p00, p11, p32 = f32(proj[0]), f32(proj[5]), f32(proj[14])
        tz_sq = vs[2] * vs[2]
        jsx = -(p00 * res[0]) / (two * vs[2])
        jsy = -(p11 * res[1]) / (two * vs[2])
        jtx = (p00 * vs[0] * res[0]) / (two * tz_sq)
        jty = (p11 * vs[1] * res[1]) / (two * tz_sq)
        jtz = ((nf[1] - nf[0]) * p32) / (two * tz_sq)
        J = [[jsx, zero, zero], [zero, jsy, zero], [jtx, jty, jtz]]
        Wm = [[V[c * 4 + i] for i in range(3)] for c in range(3)]
        JW = _m3_mul(J, Wm)
        Vp = _m3_mul(_m3_mul(JW, cov3d), _m3_t(JW))
        c00, c01, c11 = Vp[0][0] + f32(0.3), Vp[0][1], Vp[1][1] + f32(0.3)
        mid = c00 + c11
        da, db = c00 - c11, two * c01
        delta = np.sqrt(da * da + db * db)
        lam1, lam2 = f32(0.5) * (mid + delta), f32(0.5) * (mid - delta)
        lam_ok = ~(lam2 < 0)                                                        # :189
        vis = clip_ok & lam_ok
        dvy = (-c00 + c01 + lam1) / (c01 - c11 + lam1)
        inv_len = one / np.sqrt(one * one + dvy * dvy)
        ddx, ddy = one * inv_len, dvy * inv_len
        major = _min_glsl(f32(3.0) * np.sqrt(lam1), f32(1024.0))
        minor = _min_glsl(f32(3.0) * np.sqrt(lam2), f32(1024.0))
        hx, hy = res[0] * f32(0.5), res[1] * f32(0.5)
        qs = [(major * ddx) / hx, (major * ddy) / hy, (minor * ddy) / hx, (minor * (-ddx)) / hy]
    q = np.stack([np.broadcast_to(np.asarray(v, np.float32), (n,)) for v in pos2d + qs + ws], 1).astype(np.float32)
    lists = [q[vis & (face == fc)] for fc in range(6)]
    return (lists, (face, clip_ok, np.broadcast_to(lam_ok, (n,)))) if masks else lists


def depth_of(ws, light, far):
    """d of the pin: sqrt((dx dx + dy dy) + dz dz) / far in fp32, clamped to [0, 1], NaN -> 1."""
    L = np.asarray(light, np.float32)
    with np.errstate(all="ignore"):
        dx, dy, dz = ws[:, 0] - L[0], ws[:, 1] - L[1], ws[:, 2] - L[2]
        d = np.sqrt((dx * dx + dy * dy) + dz * dz) / f32(far)
        return np.where(d > 0, np.fmin(d, f32(1.0)), np.where(np.isnan(d), f32(1.0), f32(0.0))).astype(np.float32)


def pad24(q12):
    q = np.zeros((q12.shape[0], 24), np.float32)
    q[:, 0:8] = q12[:, 0:8]
    q[:, 20:24] = q12[:, 8:12]
    return q


def shadow_cube(lists, S, light, far):
    """Stage B.  -> (cube (6, S, S) float32, skipped)"""
    cube = np.ones((6, S, S), np.float32)
    skipped = 0
    for fc in range(6):
        q12 = np.ascontiguousarray(lists[fc], np.float32).reshape(-1, 12)
        if not q12.shape[0]:
            continue
        s = sr.setup(pad24(q12), S, S)
        skipped += int(s["skip"].sum())
        d = depth_of(q12[:, 8:12], light, far)
        for tri in s["tris"]:
            for qi in np.nonzero(tri["valid"])[0]:
                x0, y0, x1, y1 = (int(v) for v in tri["box"][qi])
                Px = 256 * np.arange(x0, x1 + 1, dtype=np.int64) + 128
                Py = 256 * np.arange(y0, y1 + 1, dtype=np.int64) + 128
                inside = np.ones((Py.size, Px.size), bool)
                for i in range(3):                                        # the inside test of splat_ref.render
                    E = tri["a"][qi, i] * Px[None, :] + tri["b"][qi, i] * Py[:, None] + tri["c"][qi, i]
                    inside &= (E > 0) | ((E == 0) & tri["bias"][qi, i])
                win = cube[fc, y0:y1 + 1, x0:x1 + 1]
                win[inside & (d[qi] < win)] = d[qi]                      # GL_LESS
    return cube, skipped


def cube_texel(cube, x, y, z):
    """texture(u_shadowCubemap, v).r by the header's rule; x, y, z float32 arrays."""
    S = cube.shape[1]
    with np.errstate(all="ignore"):
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        isx = (ax >= ay) & (ax >= az)
        isy = ~isx & (ay >= az)
        isz = ~isx & ~isy
        face = np.where(isx, np.where(x < 0, 1, 0), np.where(isy, np.where(y < 0, 3, 2), np.where(z < 0, 5, 4)))
        ma = np.where(isx, ax, np.where(isy, ay, az))
        sc = np.select([face == 0, face == 1, face == 2, face == 3, face == 4, face == 5], [-z, z, x, x, x, -x])
        tc = np.select([face == 0, face == 1, face == 2, face == 3, face == 4, face == 5], [-y, -y, z, -z, -y, -y])
        s = f32(0.5) * (sc / ma + f32(1.0))
        t = f32(0.5) * (tc / ma + f32(1.0))
        bad = np.isnan(s) | np.isnan(t)
        i = np.fmin(np.fmax(np.floor(s * f32(S)), f32(0.0)), f32(S - 1))
        j = np.fmin(np.fmax(np.floor(t * f32(S)), f32(0.0)), f32(S - 1))
        i = np.where(bad, 0, i).astype(np.int64)
        j = np.where(bad, 0, j).astype(np.int64)
        face = np.where(bad, 5, face)
    return cube[face, j, i]


def shadow_counts(pos, cube, light, far):
    """computeShadowFactor's count 0..20 per pixel; pos (..., 3) float32."""
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    L = np.asarray(light, np.float32)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - L[0], p[:, 1] - L[1], p[:, 2] - L[2]
        cur = np.sqrt((dx * dx + dy * dy) + dz * dz)
        sx, sy, sz = dx / cur, dy / cur, dz / cur
        lhs = cur - f32(0.05)
        count = np.zeros(p.shape[0], np.int32)
        for o in OFFSETS:
            vx, vy, vz = sx + f32(o[0]) * f32(0.025), sy + f32(o[1]) * f32(0.025), sz + f32(o[2]) * f32(0.025)
            closest = cube_texel(cube, vx, vy, vz) * f32(far)
            count += (lhs > closest).astype(np.int32)
    return count.reshape(np.asarray(pos).shape[:-1]).astype(np.uint8)


def _max0(v):
    return np.where(v > 0, v, np.where(np.isnan(v), v, v * 0 + 0))     # max(v, 0.0), NaN kept


def shade(planes, counts, lp, dt):
    """The value arithmetic of render mode 6 (gaussianSplattingDeferredPS.glsl:119-164) in dtype `dt`.  planes: the five G-buffer
    planes (H, W, 4); counts (H, W); lp: an object with light_position, light_color, light_intensity, camera_position (float32
    values).  -> colour (H, W, 3) in dt BEFORE clamping and quantisation."""
    pos, nrm, alb, _, mr = planes
    c = lambda v: dt(f32(v))                                            # a float literal of the shader
    with np.errstate(all="ignore"):
        a = (alb[..., :3].astype(np.float32) / f32(255.0)).astype(dt)   # the texture read: q / 255 in fp32
        rough = (mr[..., 1].astype(np.float32) / f32(255.0)).astype(dt)[..., None]
        metal = (mr[..., 2].astype(np.float32) / f32(255.0)).astype(dt)[..., None]
        P = pos[..., :3].astype(np.float32).astype(dt)
        N = nrm[..., :3].astype(np.float32).astype(dt) * c(2.0) - c(1.0)
        dot = lambda u, v: ((u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2])[..., None]
        norm = lambda v: v * (c(1.0) / np.sqrt(dot(v, v)))
        N = norm(N)
        shadow = counts.astype(dt)[..., None] / c(20.0)
        a = np.power(a, c(2.2))
        Lp = np.asarray(lp.light_position, np.float32).astype(dt)
        Cp = np.asarray(lp.camera_position, np.float32).astype(dt)
        Lv = Lp - P
        d = np.sqrt(dot(Lv, Lv))
        L = norm(Lv)
        V = norm(Cp - P)
        H = norm(V + L)
        att = c(1.0) / (d * d)
        rad = (np.asarray(lp.light_color, np.float32).astype(dt) * dt(f32(lp.light_intensity))) * att
        im = c(1.0) - metal
        F0 = c(0.04) * im + a * metal
        hv = _max0(dot(H, V))
        f5 = np.power(np.fmin(np.fmax(c(1.0) - hv, c(0.0)), c(1.0)), c(5.0))
        F = F0 + (c(1.0) - F0) * f5
        aa = rough * rough
        aa = aa * aa
        nh = _max0(dot(N, H))
        den = (nh * nh) * (aa - c(1.0)) + c(1.0)
        den = ((c(22.0) / c(7.0)) * den) * den                          # PI * denom * denom, PI the macro 22.0f/7.0f
        NDF = aa / den
        nv, nl = _max0(dot(N, V)), _max0(dot(N, L))
        rr = rough + c(1.0)
        kk = (rr * rr) / c(8.0)
        G = (nl / (nl * (c(1.0) - kk) + kk)) * (nv / (nv * (c(1.0) - kk) + kk))
        spec = ((NDF * G) * F) / ((c(4.0) * nv) * nl + c(0.0001))
        kD = (c(1.0) - F) * im
        Lo = ((((kD * a) / c(22.0)) / c(7.0) + spec) * rad) * nl * (c(1.0) - shadow)      # kD * albedo / PI: the macro again
        col = c(0.3) * a + Lo
        col = col / (col + c(1.0))
        col = np.power(col, c(1.0) / c(2.2))
    return col


def quantise(col):
    with np.errstate(all="ignore"):
        q = np.rint(np.fmin(np.fmax(col.astype(np.float64), 0.0), 1.0) * 255.0)
    return np.where(np.isnan(q), 0, q).astype(np.uint8)


def relight(planes, cube, lp, mode=6):
    """-> (frame (H, W, 4) uint8, counts (H, W) uint8 or None, ill (H, W) bool or None): the reference frame (float64, rounded once)
    and the pixels whose float32 and float64 evaluations differ by more than a quarter LSB before quantisation."""
    H, W = planes[2].shape[:2]
    frame = np.zeros((H, W, 4), np.uint8)
    frame[..., 3] = 255
    if mode == 5:
        frame[..., 0:2] = planes[4][..., 0:2]
        return frame, None, None
    if mode != 6:
        frame[..., 0:3] = planes[2][..., 0:3]
        return frame, None, None
    counts = shadow_counts(planes[0][..., :3].astype(np.float32), cube, lp.light_position, lp.far_plane)
    c64, c32 = shade(planes, counts, lp, np.float64), shade(planes, counts, lp, np.float32)
    frame[..., 0:3] = quantise(c64.astype(np.float32))
    with np.errstate(all="ignore"):
        k64 = np.fmin(np.fmax(c64, 0.0), 1.0) * 255.0
        k32 = np.fmin(np.fmax(c32.astype(np.float64), 0.0), 1.0) * 255.0
        both_nan = np.isnan(k64) & np.isnan(k32)
        diff = np.where(both_nan, 0.0, np.where(np.isnan(k64) | np.isnan(k32), np.inf, np.abs(k64 - k32)))
    return frame, counts, (diff > 0.25).any(-1)


# ---- the cases tests/test_light_cpu.py and tests/test_gpu_light.py share ------------------------------------------------------
class Light:
    def __init__(self, pos=(0.3, 1.9, 1.2), color=(1.0, 0.9, 0.8), intensity=12.0, cam=(0.2, 0.4, 3.0), near=0.01, far=50.0):
        self.light_position = tuple(float(f32(v)) for v in pos)
        self.light_color = tuple(float(f32(v)) for v in color)
        self.light_intensity = float(f32(intensity))
        self.camera_position = tuple(float(f32(v)) for v in cam)
        self.near_plane, self.far_plane = float(f32(near)), float(f32(far))


def random_gbuffer(W, H, seed, edge=False):
    """A plausible G-buffer: positions on a bumpy sheet in front of the camera, unit normals facing it (encoded n * 0.5 + 0.5),
    random albedo, roughness in [0.15, 1], metallic 0 (what m2s_splat leaves).  edge: special values in the first pixels."""
    rng = np.random.default_rng(seed)
    pos = np.zeros((H, W, 4), np.float16)
    pos[..., 0] = rng.uniform(-2, 2, (H, W))
    pos[..., 1] = rng.uniform(-1.5, 1.5, (H, W))
    pos[..., 2] = rng.uniform(-0.5, 0.5, (H, W))
    pos[..., 3] = 1
    n = rng.normal(size=(H, W, 3)) * 0.35 + np.array([0.0, 0.3, 1.0])
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    nrm = np.zeros((H, W, 4), np.float16)
    nrm[..., :3] = n * 0.5 + 0.5
    nrm[..., 3] = 1
    alb = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    mr = np.zeros((H, W, 4), np.uint8)
    mr[..., 0] = rng.integers(0, 256, (H, W))
    mr[..., 1] = rng.integers(38, 256, (H, W))
    mr[..., 3] = 255
    dep = np.zeros((H, W, 4), np.float16)
    if edge:
        flat = [a.reshape(-1, 4) for a in (pos, nrm, alb, mr)]
        flat[0][0, :3] = 0                                  # zero position
        flat[0][1, :3] = (0.3, 1.9, 1.2)                    # (nearly) the light itself: light inside the receiver
        flat[3][2, 1] = 0                                   # roughness 0
        flat[3][3, 1] = 255                                 # roughness 1
        flat[2][4, :3] = 0                                  # albedo 0
        flat[2][5, :3] = 255                                # albedo 255
        flat[0][6, 0] = np.nan                              # NaN / Inf texels in the position plane
        flat[0][7, 1] = np.inf
        flat[3][8, 2] = 255                                 # metallic 1 (an uploaded G-buffer may carry it)
    return [pos, nrm, alb, dep, mr]


def random_cube(S, seed, far):
    """Depths around the distances of random_gbuffer's sheet from Light's position, so that the 20 taps disagree on many pixels."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 4.0, (6, S, S)) / far).astype(np.float32)


RELIGHT_CASES = (dict(W=97, H=61, seed=11, S=64, edge=False), dict(W=64, H=48, seed=12, S=257, edge=True))
ILL_SHARE_MAX = 0.005
