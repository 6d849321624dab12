"""numpy restatement of the mesh depth prepass as include/m2s.h pins it (m2s_mesh_depth): fp32 operation by operation, int64 edges.
Test infrastructure: the GPU tests hold m2s_meshdepth.hip to these bits, tests/test_meshdepth_cpu.py holds THIS file to geometry.

Matrices are (4, 4) float32 in glm's memory order (m[c] = column c), as everywhere in the tests."""
from __future__ import annotations

import numpy as np

F = np.float32
TILE = 16
INPLACE = 4           # kMdInplace: the default in-place threshold (only the `pairs` count depends on it)
GUARD = F(16384.0)


def mat4_mul(A, B):
    """glm's mat4 * mat4: element (column j, row i) = ((A[0][i] B[j][0] + A[1][i] B[j][1]) + A[2][i] B[j][2]) + A[3][i] B[j][3]."""
    A, B = np.asarray(A, F), np.asarray(B, F)
    R = np.zeros((4, 4), F)
    for j in range(4):
        R[j] = ((A[0] * B[j, 0] + A[1] * B[j, 1]) + A[2] * B[j, 2]) + A[3] * B[j, 3]
    return R


def pvm(proj, view, model):
    return mat4_mul(mat4_mul(proj, view), model)


def clip_positions(PVM, pos):
    """pos (..., 3) float32 -> (..., 4): (m0 x + m1 y) + (m2 z + m3 * 1)."""
    pos = np.asarray(pos, F)
    x, y, z = pos[..., 0:1], pos[..., 1:2], pos[..., 2:3]
    return (PVM[0] * x + PVM[1] * y) + (PVM[2] * z + PVM[3])


def plane_d(pl, c):
    w2 = c[..., 3] + c[..., 3]
    return [c[..., 2] + c[..., 3], w2 - c[..., 0], w2 + c[..., 0], w2 - c[..., 1], w2 + c[..., 1]][pl]


def clip_polygon(c):
    """Sutherland-Hodgman of one triangle c (3, 4) against the five planes, in order -> list of float32 (4,) vertices (maybe empty)."""
    poly = [np.asarray(v, F) for v in c]
    for pl in range(5):
        if len(poly) < 3:
            break
        out = []
        n = len(poly)
        for i in range(n):
            a, b = poly[i], poly[(i + 1) % n]
            da, db = plane_d(pl, a), plane_d(pl, b)
            ain, bin_ = bool(da >= 0), bool(db >= 0)
            if ain and len(out) < 8:
                out.append(a)
            if ain != bin_ and len(out) < 8:           # (8 vertices at most, as the kernel's array)
                vi, vo, di, do = (a, b, da, db) if ain else (b, a, db, da)
                t = F(di / F(di - do))
                out.append((vi + t * (vo - vi)).astype(F))
        poly = out
    return poly if len(poly) >= 3 else []


def pieces_setup(c, W, H):
    """c (K, 3, 4) clip positions of K pieces -> ok (K,), X, Y (K, 3) int64, box (K, 4) = x0, x1, y0, y1, zw (K, 3) float32."""
    c = np.asarray(c, F).reshape(-1, 3, 4)
    with np.errstate(all="ignore"):
        w = c[..., 3]
        nx, ny = c[..., 0] / w, c[..., 1] / w
        zw = (c[..., 2] / w) * F(0.5) + F(0.5)
        ok = (zw < F(1.0)).any(1)
        hw, hh = F(W) * F(0.5), F(H) * F(0.5)
        xw, yw = hw * nx + hw, hh * ny + hh
        ok &= ((np.abs(xw) < GUARD) & (np.abs(yw) < GUARD)).all(1)
        X = np.rint(np.where(ok[:, None], xw * F(256.0), F(0))).astype(np.int64)
        Y = np.rint(np.where(ok[:, None], yw * F(256.0), F(0))).astype(np.int64)
    order = np.argsort(Y * (1 << 32) + X, axis=1, kind="stable")          # canonical vertex order: ascending (Y, X)
    X, Y, zw = np.take_along_axis(X, order, 1), np.take_along_axis(Y, order, 1), np.take_along_axis(zw, order, 1)
    x0 = np.maximum((X.min(1) - 128 + 255) >> 8, 0)
    x1 = np.minimum((X.max(1) - 128) >> 8, W - 1)
    y0 = np.maximum((Y.min(1) - 128 + 255) >> 8, 0)
    y1 = np.minimum((Y.max(1) - 128) >> 8, H - 1)
    ok &= (x0 <= x1) & (y0 <= y1)
    area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    ok &= area2 != 0
    return ok, X, Y, np.stack([x0, x1, y0, y1], 1), zw


def raster_piece(X, Y, zw, box):
    """-> covered (h, w) bool, z (h, w) float32 over the piece's pixel box."""
    X, Y = [int(v) for v in X], [int(v) for v in Y]
    x0, x1, y0, y1 = (int(v) for v in box)
    area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    sgn = -1 if area2 < 0 else 1
    Px = (np.arange(x0, x1 + 1, dtype=np.int64) * 256 + 128)[None, :]
    Py = (np.arange(y0, y1 + 1, dtype=np.int64) * 256 + 128)[:, None]
    inva = F(1.0) / np.array([abs(area2)], np.int64).astype(F)[0]
    cov = np.ones((y1 - y0 + 1, x1 - x0 + 1), bool)
    b = []
    for i in range(3):
        ia, ib = (i + 1) % 3, (i + 2) % 3
        dy, dx = Y[ib] - Y[ia], X[ib] - X[ia]
        a_, b_ = -dy * sgn, dx * sgn
        c_ = (dy * X[ia] - dx * Y[ia]) * sgn
        E = a_ * Px + b_ * Py + c_
        bias = a_ > 0 or (a_ == 0 and b_ > 0)
        cov &= (E > 0) | ((E == 0) & bias)
        b.append(E.astype(F) * inva)
    with np.errstate(all="ignore"):
        z = (b[0] * zw[0] + b[1] * zw[1]) + b[2] * zw[2]
        z = np.where(z < 0, F(0), np.where(z > 1, F(1), z)).astype(F)
    return cov, z


def classify(c):
    """c (N, 3, 4) -> finite (N,), dead (N,), needs_clip (N,)"""
    fin = np.isfinite(c).all((1, 2))
    with np.errstate(all="ignore"):
        out = np.stack([~(plane_d(pl, c) >= 0) for pl in range(5)], 0)         # (5, N, 3)
    dead = out.all(2).any(0)
    return fin, dead & fin, out.any((0, 2)) & fin & ~dead


def mesh_depth(positions, opaque, proj, view, model, W, H, inplace=INPLACE, want_winner=True):
    """positions (N, 3, 3) float32 triangle vertices in draw order; opaque (N,) bool (base colour alpha == 1.0 exactly).
    -> dict: image (H, W) float32 row 0 = bottom, winner (H, W) int32 (-1: none), frags (H, W) int32 covering fragments,
       counts = [drawn, clipped, non_finite, pairs]."""
    pos = np.asarray(positions, F).reshape(-1, 3, 3)
    opaque = np.asarray(opaque, bool).reshape(-1)
    N = pos.shape[0]
    image = np.ones((H, W), F)
    winner = np.full((H, W), -1, np.int32)
    frags = np.zeros((H, W), np.int32)
    counts = [0, 0, 0, 0]
    if N == 0:
        return dict(image=image, winner=winner, frags=frags, counts=counts)
    PVM = pvm(proj, view, model)
    with np.errstate(all="ignore"):
        c = clip_positions(PVM, pos)
    fin, dead, clip = classify(c)
    counts[2] = int((opaque & ~fin).sum())
    clip &= opaque
    counts[1] = int(clip.sum())
    plain = opaque & fin & ~dead & ~clip
    # pieces: (triangle, clip positions (3, 4))
    tri_ids = [np.nonzero(plain)[0]]
    pcs = [c[plain]]
    for t in np.nonzero(clip)[0]:
        poly = clip_polygon(c[t])
        for i in range(1, len(poly) - 1):
            tri_ids.append(np.array([t]))
            pcs.append(np.stack([poly[0], poly[i], poly[i + 1]])[None])
    tri_ids = np.concatenate(tri_ids)
    pcs = np.concatenate(pcs, 0) if len(tri_ids) else np.zeros((0, 3, 4), F)
    ok, X, Y, box, zw = pieces_setup(pcs, W, H)
    counts[0] = int(np.unique(tri_ids[ok]).size)
    bw, bh = box[:, 1] - box[:, 0], box[:, 3] - box[:, 2]
    deferred = clip[tri_ids] | ~((bw < inplace) & (bh < inplace))
    tiles = (box[:, 1] // TILE - box[:, 0] // TILE + 1) * (box[:, 3] // TILE - box[:, 2] // TILE + 1)
    counts[3] = int(tiles[ok & deferred].sum())
    for k in np.nonzero(ok)[0]:
        cov, z = raster_piece(X[k], Y[k], zw[k], box[k])
        x0, x1, y0, y1 = (int(v) for v in box[k])
        frags[y0:y1 + 1, x0:x1 + 1] += cov
        sub = image[y0:y1 + 1, x0:x1 + 1]
        win = cov & (z < sub)                      # GL_LESS; a NaN never passes
        sub[win] = z[win]
        if want_winner:
            winner[y0:y1 + 1, x0:x1 + 1][win] = tri_ids[k]
    return dict(image=image, winner=winner, frags=frags, counts=counts)


def scene_triangles(scene):
    """mesh2splat_amd.scene.Scene -> (positions (N, 3, 3), opaque (N,)) in the flattened draw order."""
    P, O = [], []
    for m in scene.meshes:
        P.append(np.asarray(m.vertices[:, 0:3], F).reshape(-1, 3, 3))
        O.append(np.full(m.n_triangles, F(m.base_color[3]) == F(1.0)))
    if not P:
        return np.zeros((0, 3, 3), F), np.zeros(0, bool)
    return np.concatenate(P), np.concatenate(O)


def prepass_texel(uv, W, H):
    """The viewer prepass's lookup (gaussianSplattingPrepassCS.glsl:79-91, GL_NEAREST, clamp to edge): uv in [0, 1]^2 -> (x, y)."""
    x = int(min(max(np.floor(F(uv[0]) * F(W)), 0), W - 1))
    y = int(min(max(np.floor(F(uv[1]) * F(H)), 0), H - 1))
    return x, y
