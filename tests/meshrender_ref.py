"""numpy restatement of the mesh render pass as include/m2s.h pins it (m2s_mesh_render).  Test infrastructure: the GPU tests hold
m2s_meshdepth.hip (visibility stage) and m2s_meshrender.hip (shading) to this file, tests/test_meshrender_cpu.py holds THIS file to
geometry.

 - visibility(): the winner + depth image, exact (fp32 decision arithmetic, int64 edges), built on tests/meshdepth_ref.py.
 - shade(): the five planes of the winners, evaluated in a chosen precision: np.float32 = as pinned (fp64 barycentrics rounded to
   fp32, then fp32 operation by operation), np.float64 = everything in float64 from the fp32 inputs (the yardstick of the GPU tests).

Matrices are (4, 4) float32 in glm's memory order (m[c] = column c), as everywhere in the tests."""
from __future__ import annotations

import numpy as np

import meshdepth_ref as md
import pyref

F = np.float32
D = np.float64
ONE_BITS = 0x3F800000
EMPTY = np.uint64((ONE_BITS << 32) | 0xFFFFFFFF)
COUNT_NAMES = ("drawn", "clipped", "non_finite", "pairs", "culled")        # (the kernel's fifth, texel updates, depends on timing)


# ---- stage 1: visibility ---------------------------------------------------------------------------------------------------------------
def _stored_area(pcs, W, H):
    """pieces (K, 3, 4) -> (reach (K,): the piece gets as far as the area test, area2 (K,) int64 of the snapped vertices in STORED order)."""
    c = np.asarray(pcs, F).reshape(-1, 3, 4)
    with np.errstate(all="ignore"):
        w = c[..., 3]
        nx, ny = c[..., 0] / w, c[..., 1] / w
        zw = (c[..., 2] / w) * F(0.5) + F(0.5)
        reach = (zw < F(1.0)).any(1)
        hw, hh = F(W) * F(0.5), F(H) * F(0.5)
        xw, yw = hw * nx + hw, hh * ny + hh
        reach &= ((np.abs(xw) < md.GUARD) & (np.abs(yw) < md.GUARD)).all(1)
        X = np.rint(np.where(reach[:, None], xw * F(256.0), F(0))).astype(np.int64)
        Y = np.rint(np.where(reach[:, None], yw * F(256.0), F(0))).astype(np.int64)
    x0 = np.maximum((X.min(1) - 128 + 255) >> 8, 0)
    x1 = np.minimum((X.max(1) - 128) >> 8, W - 1)
    y0 = np.maximum((Y.min(1) - 128 + 255) >> 8, 0)
    y1 = np.minimum((Y.max(1) - 128) >> 8, H - 1)
    reach &= (x0 <= x1) & (y0 <= y1)
    area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    return reach, area2


def visibility(positions, proj, view, model, W, H, inplace=md.INPLACE, tri_first=0):
    """positions (N, 3, 3) float32 triangle vertices in draw order (every mesh is drawn); tri_first: global index of triangle 0.
    -> dict: vis (H, W) uint64 row 0 = bottom, winner (H, W) int64 LOCAL index (-1: none), depth (H, W) float32 (1.0: none),
       frags (H, W) int32 fragments that passed the cull, counts = [drawn, clipped, non_finite, pairs, culled]."""
    pos = np.asarray(positions, F).reshape(-1, 3, 3)
    N = pos.shape[0]
    vis = np.full((H, W), EMPTY, np.uint64)
    frags = np.zeros((H, W), np.int32)
    counts = [0, 0, 0, 0, 0]
    if N:
        PVM = md.pvm(proj, view, model)
        with np.errstate(all="ignore"):
            c = md.clip_positions(PVM, pos)
        fin, dead, clip = md.classify(c)
        counts[2] = int((~fin).sum())
        counts[1] = int(clip.sum())
        plain = fin & ~dead & ~clip
        tri_ids, pcs = [np.nonzero(plain)[0]], [c[plain]]
        for t in np.nonzero(clip)[0]:
            poly = md.clip_polygon(c[t])
            for i in range(1, len(poly) - 1):
                tri_ids.append(np.array([t]))
                pcs.append(np.stack([poly[0], poly[i], poly[i + 1]])[None])
        tri_ids = np.concatenate(tri_ids)
        pcs = np.concatenate(pcs, 0) if len(tri_ids) else np.zeros((0, 3, 4), F)
        ok, X, Y, box, zw = md.pieces_setup(pcs, W, H)
        reach, stored = _stored_area(pcs, W, H)
        ok &= stored > 0                                          # GL_CULL_FACE, front = CCW
        back = reach & (stored < 0)
        drawn_tris = np.unique(tri_ids[ok])
        counts[0] = int(drawn_tris.size)
        counts[4] = int(np.setdiff1d(np.unique(tri_ids[back]), drawn_tris).size)
        bw, bh = box[:, 1] - box[:, 0], box[:, 3] - box[:, 2]
        deferred = clip[tri_ids] | ~((bw < inplace) & (bh < inplace))
        tiles = (box[:, 1] // md.TILE - box[:, 0] // md.TILE + 1) * (box[:, 3] // md.TILE - box[:, 2] // md.TILE + 1)
        counts[3] = int(tiles[ok & deferred].sum())
        for k in np.nonzero(ok)[0]:
            cov, z = md.raster_piece(X[k], Y[k], zw[k], box[k])
            x0, x1, y0, y1 = (int(v) for v in box[k])
            frags[y0:y1 + 1, x0:x1 + 1] += cov
            key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(tri_first + int(tri_ids[k]))
            sub = vis[y0:y1 + 1, x0:x1 + 1]
            win = cov & (z < F(1.0)) & (key < sub)                # GL_LESS, the lowest index wins a tie; a NaN never competes
            sub[win] = key[win]
    hit = vis != EMPTY
    winner = np.where(hit, (vis & np.uint64(0xFFFFFFFF)).astype(np.int64) - tri_first, -1)
    depth = np.where(hit, (vis >> np.uint64(32)).astype(np.uint32).view(F), F(1.0)).astype(F)
    return dict(vis=vis, winner=winner, depth=depth, frags=frags, counts=counts)


# ---- the scene as arrays ---------------------------------------------------------------------------------------------------------------
def scene_arrays(scene):
    """mesh2splat_amd.scene.Scene -> dict of per-triangle arrays in the flattened draw order and per-mesh material data."""
    from mesh2splat_amd.scene import TEXTURE_SLOTS
    P, Nn, T, UV, M, PID, mats = [], [], [], [], [], [], []
    for i, m in enumerate(scene.meshes):
        v = np.asarray(m.vertices, F)
        n = m.n_triangles
        P.append(v[:, 0:3].reshape(n, 3, 3)); Nn.append(v[:, 3:6].reshape(n, 3, 3)); T.append(v[:, 6:10].reshape(n, 3, 4))
        UV.append(v[:, 10:12].reshape(n, 3, 2)); M.append(np.full(n, i, np.int64)); PID.append(np.arange(n, dtype=np.int64))
        mats.append(dict(color=np.asarray(m.base_color, F),
                         levels=[pyref.build_mips(m.textures[k]) if k in m.textures else None for k in TEXTURE_SLOTS]))
    cat = lambda a, shape: np.concatenate(a) if a else np.zeros(shape, F)
    return dict(pos=cat(P, (0, 3, 3)), nrm=cat(Nn, (0, 3, 3)), tan=cat(T, (0, 3, 4)), uv=cat(UV, (0, 3, 2)),
                mesh=np.concatenate(M) if M else np.zeros(0, np.int64), pid=np.concatenate(PID) if PID else np.zeros(0, np.int64), mats=mats)


# ---- stage 2: shading ------------------------------------------------------------------------------------------------------------------
def _mat4_vec(m, x, y, z, w, T):
    m = np.asarray(m, T)
    return (m[0] * x[..., None] + m[1] * y[..., None]) + (m[2] * z[..., None] + m[3] * w[..., None])


def _mat3_vec(m, v, T):
    m = np.asarray(m, T)
    return (m[0] * v[..., 0:1] + m[1] * v[..., 1:2]) + m[2] * v[..., 2:3]


def _normalize(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt((v[..., 0:1] * v[..., 0:1] + v[..., 1:2] * v[..., 1:2]) + v[..., 2:3] * v[..., 2:3])


def normal_matrix(model, T):
    """mat3(transpose(inverse(M))) from the fp32 matrix in float64 (rounded to fp32 for the pinned evaluation), glm memory order."""
    Mm = np.asarray(model, F).astype(D).T                  # math matrix
    Nm = np.linalg.inv(Mm).T[:3, :3]                       # math
    return np.ascontiguousarray(Nm.T).astype(T)            # glm order: [c] = column c


def _bary(c, px, py, W, H):
    """c (n, 3, 4) clip coordinates (fp32, or float64 for the yardstick), pixel (px, py) -> lambda (n, 3) float64."""
    c = c.astype(D)
    nx, ny = (2 * px + 1).astype(D) / D(W) - 1.0, (2 * py + 1).astype(D) / D(H) - 1.0
    e = []
    with np.errstate(all="ignore"):
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            A = c[:, j, 1] * c[:, k, 3] - c[:, j, 3] * c[:, k, 1]
            B = c[:, j, 0] * c[:, k, 3] - c[:, j, 3] * c[:, k, 0]
            C = c[:, j, 0] * c[:, k, 1] - c[:, j, 1] * c[:, k, 0]
            e.append((nx * A - ny * B) + C)
        s = (e[0] + e[1]) + e[2]
        return np.stack([e[0] / s, e[1] / s, e[2] / s], 1)


def _lerp(l, a):
    """l (n, 3), a (n, 3, k) -> (n, k): (l0 a0 + l1 a1) + l2 a2."""
    return (l[:, 0:1] * a[:, 0] + l[:, 1:2] * a[:, 1]) + l[:, 2:3] * a[:, 2]


def _bilinear(level, uf, vf, T):
    Hh, Ww = level.shape[:2]
    up, vp = uf * T(Ww) - T(0.5), vf * T(Hh) - T(0.5)
    fi, fj = np.floor(up), np.floor(vp)
    a, b = (up - fi)[:, None], (vp - fj)[:, None]
    i0, j0 = fi.astype(np.int64) % Ww, fj.astype(np.int64) % Hh
    i1, j1 = (i0 + 1) % Ww, (j0 + 1) % Hh
    t = level.astype(T)
    na, nb = T(1) - a, T(1) - b
    return ((na * nb) * t[j0, i0] + (a * nb) * t[j0, i1] + (na * b) * t[j1, i0]) + (a * b) * t[j1, i1]


def _sample(levels, u, v, grads, T):
    """texture(map, uv) with the pass's implicit LOD: levels 0..4, REPEAT, trilinear -> (n, 4) in [0, 1]."""
    def frac(x):
        with np.errstate(all="ignore"):
            f = x - np.floor(x)
        return np.minimum(np.where(f >= 0, f, T(0)), T(1)).astype(T)
    uf, vf = frac(u), frac(v)
    Hh, Ww = levels[0].shape[:2]
    dudx, dvdx, dudy, dvdy = grads
    with np.errstate(all="ignore"):
        sx, tx, sy, ty = dudx * T(Ww), dvdx * T(Hh), dudy * T(Ww), dvdy * T(Hh)
        lam = T(0.5) * np.log2(np.fmax(sx * sx + tx * tx, sy * sy + ty * ty))
    lam = np.where(np.isfinite(dudx) & np.isfinite(dvdx) & np.isfinite(dudy) & np.isfinite(dvdy), lam, np.inf).astype(T)
    q = len(levels) - 1
    pos = lam > 0
    d = np.where(pos, np.where(lam >= q, T(q), np.floor(np.where(np.isfinite(lam), lam, 0))), T(0)).astype(T)
    f = np.where(pos & (lam < q), lam - d, T(0)).astype(T)[:, None]
    l0 = d.astype(np.int64)
    l1 = np.minimum(l0 + 1, q)
    lo, hi = np.zeros((len(u), 4), T), np.zeros((len(u), 4), T)
    for L in range(q + 1):
        for sel, out in ((l0 == L, lo), (l1 == L, hi)):
            if sel.any():
                out[sel] = _bilinear(levels[L], uf[sel], vf[sel], T)
    return ((f * hi + (T(1) - f) * lo) * T(F(0.003921568859368563))).astype(T), lam


def shade(arr, winner, proj, view, model, W, H, near_far, mode, T=F, tri_first=0):
    """arr: scene_arrays(); winner (H, W) local triangle index or -1.  T = np.float32: as pinned; np.float64: the yardstick.
    -> dict: planes = [pos (H, W, 4) float16, normal float16, albedo uint8, depth float16, metallic-roughness uint8],
             raw = unquantised pos (H, W, 3), normal (encoded), colour (the albedo plane's rgb), depth (H, W), mr (H, W, 2),
             uv (H, W, 2), lam (H, W, 3) barycentrics, lod (H, W) of the first map present (NaN: none)."""
    ys, xs = np.nonzero(winner >= 0)
    t = winner[ys, xs]
    n = len(t)
    pos = arr["pos"][t]
    if T == F:
        PVM = md.pvm(proj, view, model)
        with np.errstate(all="ignore"):
            c = md.clip_positions(PVM, pos)
    else:
        mm = lambda a: np.asarray(a, F).astype(D).T
        PVMm = mm(proj) @ mm(view) @ mm(model)
        c = np.concatenate([pos.astype(D), np.ones((n, 3, 1))], -1) @ PVMm.T
    lam = _bary(c, xs, ys, W, H).astype(T)
    lx = _bary(c, xs + 1, ys, W, H).astype(T)
    ly = _bary(c, xs, ys + 1, W, H).astype(T)
    uvc = arr["uv"][t].astype(T)
    with np.errstate(all="ignore"):
        uv = _lerp(lam, uvc)
        gx, gy = _lerp(lx, uvc) - uv, _lerp(ly, uvc) - uv
        grads = (gx[:, 0], gx[:, 1], gy[:, 0], gy[:, 1])
        p = pos.astype(T)
        one = np.ones(p.shape[:2], T)
        ws4 = _mat4_vec(np.asarray(model, F).astype(T), p[..., 0], p[..., 1], p[..., 2], one, T)
        vdc = -_mat4_vec(np.asarray(view, F).astype(T), ws4[..., 0], ws4[..., 1], ws4[..., 2], ws4[..., 3], T)[..., 2]
        Nm = normal_matrix(model, T)
        vn = _normalize(_mat3_vec(Nm, arr["nrm"][t].astype(T), T))
        tin = arr["tan"][t].astype(T)
        vt = _normalize(_mat3_vec(Nm, tin[..., :3], T))
        wpos = _lerp(lam, ws4[..., :3])
        vdepth = _lerp(lam, vdc[..., None])[:, 0]
        Nv = _normalize(_lerp(lam, vn))
        Tv = _normalize(_lerp(lam, vt))
        Tw = _lerp(lam, tin[..., 3:4])
    mesh = arr["mesh"][t]
    alb = np.zeros((n, 3), T)
    mr = np.zeros((n, 2), T)
    lod = np.full(n, np.nan)
    for mi in np.unique(mesh):
        sel = mesh == mi
        mat = arr["mats"][mi]
        g = tuple(a[sel] for a in grads)
        a = np.broadcast_to(mat["color"][:3].astype(T), (int(sel.sum()), 3)).copy()
        if mat["levels"][0] is not None:
            s, l = _sample(mat["levels"][0], uv[sel, 0], uv[sel, 1], g, T)
            a = a * s[:, :3]
            lod[sel] = l
        alb[sel] = a
        m2 = np.broadcast_to(np.array([F(0.1), F(0.5)]).astype(T), (int(sel.sum()), 2)).copy()
        if mat["levels"][2] is not None:
            s, l = _sample(mat["levels"][2], uv[sel, 0], uv[sel, 1], g, T)
            m2 = np.stack([s[:, 2], s[:, 1]], 1)
            lod[sel] = np.where(np.isnan(lod[sel]), l, lod[sel])
        mr[sel] = m2
        if mat["levels"][1] is not None:
            s, l = _sample(mat["levels"][1], uv[sel, 0], uv[sel, 1], g, T)
            lod[sel] = np.where(np.isnan(lod[sel]), l, lod[sel])
            with np.errstate(all="ignore"):
                mp = _normalize(s[:, :3] * T(2) - T(1))
                Nn, Tt = Nv[sel], Tv[sel]
                B = np.stack([Nn[:, 1] * Tt[:, 2] - Nn[:, 2] * Tt[:, 1], Nn[:, 2] * Tt[:, 0] - Nn[:, 0] * Tt[:, 2],
                              Nn[:, 0] * Tt[:, 1] - Nn[:, 1] * Tt[:, 0]], 1)
                B = _normalize(B) * Tw[sel]
                Nv[sel] = _normalize((Tt * mp[:, 0:1] + B * mp[:, 1:2]) + Nn * mp[:, 2:3])
    with np.errstate(all="ignore"):
        enc = Nv * T(0.5) + T(0.5)
        nd = (vdepth - T(F(near_far[0]))) / (T(F(near_far[1])) - T(F(near_far[0])))
        cd = np.clip(np.exp(T(-20) * np.clip(nd, 0, 1)), 0, 1).astype(T)
        if mode == 1:
            col = np.repeat(cd[:, None], 3, 1)
        elif mode == 2:
            col = enc
        elif mode == 3:
            pid = arr["pid"][t].astype(F)
            args = [pid * F(311.7), pid * F(269.5) + F(1.3), pid * F(183.3) + F(2.7)]       # fp32 in either evaluation
            vv = [np.sin(a.astype(D)).astype(F).astype(T) * T(F(43758.5453)) for a in args]
            col = np.stack([v - np.floor(v) for v in vv], 1)
        elif mode == 4:
            col = np.broadcast_to(np.array([F(0.01), F(0.005), F(0)]).astype(T), (n, 3))
        else:
            col = alb

    def q8(x):
        with np.errstate(all="ignore"):
            return np.where(np.isnan(x), 0, np.rint(np.clip(x, 0, 1) * T(255))).astype(np.uint8)

    def h(x):
        with np.errstate(all="ignore"):
            return np.asarray(x).astype(np.float16)
    planes = [np.zeros((H, W, 4), np.float16), np.zeros((H, W, 4), np.float16), np.zeros((H, W, 4), np.uint8),
              np.zeros((H, W, 4), np.float16), np.zeros((H, W, 4), np.uint8)]
    one16 = np.float16(1)
    planes[0][ys, xs] = np.concatenate([h(wpos), np.full((n, 1), one16)], 1)
    planes[1][ys, xs] = np.concatenate([h(enc), np.full((n, 1), one16)], 1)
    planes[2][ys, xs] = np.concatenate([q8(col), np.full((n, 1), 255, np.uint8)], 1)
    planes[3][ys, xs] = np.concatenate([np.repeat(h(cd)[:, None], 3, 1), np.full((n, 1), one16)], 1)
    planes[4][ys, xs] = np.concatenate([q8(mr), np.zeros((n, 1), np.uint8), np.full((n, 1), 255, np.uint8)], 1)

    def img(v, k):
        out = np.zeros((H, W, k), D)
        out[ys, xs] = np.asarray(v, D).reshape(n, k)
        return out
    raw = dict(pos=img(wpos, 3), normal=img(enc, 3), colour=img(col, 3), depth=img(cd, 1)[..., 0], mr=img(mr, 2), uv=img(uv, 2),
               lam=img(lam, 3), lod=img(lod, 1)[..., 0])
    return dict(planes=planes, raw=raw)


# ---- comparing planes in output steps ---------------------------------------------------------------------------------------------------
def half_steps(a, b):
    """|a - b| in steps of the half-precision format (float16 arrays of one shape) -> int64 array; NaN against NaN counts 0."""
    def key(x):
        u = np.ascontiguousarray(x, np.float16).view(np.uint16).astype(np.int64)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    d = np.abs(key(a) - key(b))
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


def plane_steps(got, want):
    """Five planes against five planes -> (H, W) int64: the largest difference in output steps over planes and channels."""
    worst = np.zeros(got[0].shape[:2], np.int64)
    for k in range(5):
        if k in (2, 4):
            d = np.abs(got[k].astype(np.int64) - want[k].astype(np.int64))
        else:
            d = half_steps(got[k], want[k])
        worst = np.maximum(worst, d.max(-1))
    return worst


def render(scene, proj, view, model, W, H, near_far=(0.1, 50.0), mode=0, tri_first=0, count=None):
    """Both stages -> dict: vis (visibility()), arr, pinned, exact (shade() in fp32 and in float64), well (H, W) bool: pixels on which
    the two evaluations agree within one output step (empty pixels included)."""
    arr = scene_arrays(scene)
    if count is not None or tri_first:
        sl = slice(tri_first, None if count is None else tri_first + count)
        arr = {k: (v[sl] if k != "mats" else v) for k, v in arr.items()}
    v = visibility(arr["pos"], proj, view, model, W, H, tri_first=tri_first)
    pinned = shade(arr, v["winner"], proj, view, model, W, H, near_far, mode, F)
    exact = shade(arr, v["winner"], proj, view, model, W, H, near_far, mode, D)
    well = plane_steps(pinned["planes"], exact["planes"]) <= 1
    return dict(vis=v, arr=arr, pinned=pinned, exact=exact, well=well)
