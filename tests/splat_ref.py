"""Test infrastructure: a numpy restatement of the splat pass exactly as include/m2s.h pins it (m2s_splat).  Not imported by the product.

Every fp32 operation is one numpy float32 operation (numpy does not fuse), edge functions are int64, half rounding is np.float16's
RNE, the RGBA8 rule is q = rint(clamp(r, 0, 1) * 255) read back as q / 255.  exp is float64 exp rounded to fp32 — the one step
the kernel may do differently.  The restatement never stops early.  It can be restricted to a pixel window (and the quads whose
boxes touch it), so that large frames can be checked window by window."""
from __future__ import annotations

import numpy as np

f32 = np.float32
GUARD = f32(16384.0)
VX = (-1.0, -1.0, 1.0, 1.0)        # the quad's vertices (vx, vy): (-1,-1), (-1,1), (1,1), (1,-1)
VY = (-1.0, 1.0, 1.0, -1.0)
TRIS = ((0, 1, 2), (0, 2, 3))
TILE = 16


def _h(x):
    return x.astype(np.float16).astype(np.float32)


def _clamp(x):
    return np.fmin(np.fmax(x, f32(0.0)), f32(1.0))


def _unorm8(r):
    return np.rint(_clamp(r) * f32(255.0)) / f32(255.0)


def setup(quads, W: int, H: int) -> dict:
    """Per quad: skip flag, the two triangles' edge functions and pixel boxes (as the pinned rasteriser clamps them to W x H)."""
    q = np.ascontiguousarray(quads, np.float32).reshape(-1, 24)
    n = q.shape[0]
    with np.errstate(all="ignore"):
        fin = np.isfinite(q[:, 0:2]).all(1) & np.isfinite(q[:, 4:24]).all(1)
        hw, hh = f32(W) * f32(0.5), f32(H) * f32(0.5)
        X = np.zeros((n, 4), np.int64)
        Y = np.zeros((n, 4), np.int64)
        guard = np.ones(n, bool)
        for v in range(4):
            vx, vy = f32(VX[v]), f32(VY[v])
            x = q[:, 0] + (vx * q[:, 4] + vy * q[:, 6])
            y = q[:, 1] + (vx * q[:, 5] + vy * q[:, 7])
            xw, yw = hw * x + hw, hh * y + hh
            ok = (np.abs(xw) < GUARD) & (np.abs(yw) < GUARD)
            guard &= ok
            X[:, v] = np.where(ok, np.rint(xw * f32(256.0)), 0).astype(np.int64)
            Y[:, v] = np.where(ok, np.rint(yw * f32(256.0)), 0).astype(np.int64)
    skip = ~(fin & guard)
    tris = []
    for idx in TRIS:
        Xt, Yt = X[:, idx], Y[:, idx]
        area2 = (Xt[:, 1] - Xt[:, 0]) * (Yt[:, 2] - Yt[:, 0]) - (Yt[:, 1] - Yt[:, 0]) * (Xt[:, 2] - Xt[:, 0])
        sgn = np.where(area2 < 0, -1, 1).astype(np.int64)
        a = np.zeros((n, 3), np.int64)
        b = np.zeros((n, 3), np.int64)
        c = np.zeros((n, 3), np.int64)
        for i in range(3):
            ia, ib = (i + 1) % 3, (i + 2) % 3
            dy, dx = Yt[:, ib] - Yt[:, ia], Xt[:, ib] - Xt[:, ia]
            a[:, i] = -dy * sgn
            b[:, i] = dx * sgn
            c[:, i] = (dy * Xt[:, ia] - dx * Yt[:, ia]) * sgn
        bias = (a > 0) | ((a == 0) & (b > 0))
        x0 = np.maximum((Xt.min(1) - 128 + 255) >> 8, 0)
        x1 = np.minimum((Xt.max(1) - 128) >> 8, W - 1)
        y0 = np.maximum((Yt.min(1) - 128 + 255) >> 8, 0)
        y1 = np.minimum((Yt.max(1) - 128) >> 8, H - 1)
        valid = ~skip & (area2 != 0) & (x0 <= x1) & (y0 <= y1)
        tris.append(dict(a=a, b=b, c=c, bias=bias, box=np.stack([x0, y0, x1, y1], 1), valid=valid))
    return dict(q=q, skip=skip, tris=tris, W=W, H=H)


def tile_counts(s: dict) -> np.ndarray:
    """(tiles_y, tiles_x) number of quads whose (union) box meets each 16 x 16 tile: the kernel's (tile, quad) pairs."""
    W, H = s["W"], s["H"]
    tx, ty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    t0, t1 = s["tris"]
    any_v = t0["valid"] | t1["valid"]
    big = np.iinfo(np.int64).max // 4
    bx0 = np.minimum(np.where(t0["valid"], t0["box"][:, 0], big), np.where(t1["valid"], t1["box"][:, 0], big))[any_v] // TILE
    by0 = np.minimum(np.where(t0["valid"], t0["box"][:, 1], big), np.where(t1["valid"], t1["box"][:, 1], big))[any_v] // TILE
    bx1 = np.maximum(np.where(t0["valid"], t0["box"][:, 2], -1), np.where(t1["valid"], t1["box"][:, 2], -1))[any_v] // TILE
    by1 = np.maximum(np.where(t0["valid"], t0["box"][:, 3], -1), np.where(t1["valid"], t1["box"][:, 3], -1))[any_v] // TILE
    d = np.zeros((ty + 1, tx + 1), np.int64)
    np.add.at(d, (by0, bx0), 1)
    np.add.at(d, (by0, bx1 + 1), -1)
    np.add.at(d, (by1 + 1, bx0), -1)
    np.add.at(d, (by1 + 1, bx1 + 1), 1)
    return d.cumsum(0).cumsum(1)[:ty, :tx]


def render(quads, W: int, H: int, mode: int = 0, window=None, s: dict | None = None, chunk_elems: int = 1 << 22):
    """-> (planes, skipped): five arrays (h, w, 4) — float16 for attachments 0, 1, 3, uint8 for 2, 4 — of the window
    (x0, y0, x1, y1) (exclusive ends; default the whole W x H), row 0 = the window's bottom row."""
    if s is None:
        s = setup(quads, W, H)
    q = s["q"]
    x0, y0, x1, y1 = window if window is not None else (0, 0, W, H)
    ww, wh = x1 - x0, y1 - y0
    npx = ww * wh
    px = (np.arange(npx) % ww + x0).astype(np.int64)
    py = (np.arange(npx) // ww + y0).astype(np.int64)
    # fragments (quad, triangle, pixel) of the quads whose boxes touch the window
    frag_key, frag_q, frag_p = [], [], []
    for t, tri in enumerate(s["tris"]):
        bx = tri["box"]
        sel = np.nonzero(tri["valid"] & (bx[:, 0] < x1) & (bx[:, 2] >= x0) & (bx[:, 1] < y1) & (bx[:, 3] >= y0))[0]
        step = max(1, chunk_elems // max(npx, 1))
        Px, Py = 256 * px + 128, 256 * py + 128
        for k in range(0, sel.size, step):
            qs = sel[k:k + step]
            inside = np.ones((qs.size, npx), bool)
            for i in range(3):
                E = tri["a"][qs, i, None] * Px[None, :] + tri["b"][qs, i, None] * Py[None, :] + tri["c"][qs, i, None]
                inside &= (E > 0) | ((E == 0) & tri["bias"][qs, i, None])
            qi, pi = np.nonzero(inside)
            frag_q.append(qs[qi])
            frag_p.append(pi)
            frag_key.append(qs[qi].astype(np.int64) * 2 + t)
    fq = np.concatenate(frag_q) if frag_q else np.zeros(0, np.int64)
    fp = np.concatenate(frag_p) if frag_p else np.zeros(0, np.int64)
    fk = np.concatenate(frag_key) if frag_key else np.zeros(0, np.int64)
    o = np.lexsort((fk, fp))                      # per pixel, in array order (triangle 0 before triangle 1 of the same quad)
    fq, fp = fq[o], fp[o]
    start = np.ones(fp.size, bool)
    start[1:] = fp[1:] != fp[:-1]
    run0 = np.maximum.accumulate(np.where(start, np.arange(fp.size), 0))
    rank = np.arange(fp.size) - run0
    # the fragment shader (VS:34-40, PS:30-45), fp32 operation by operation
    with np.errstate(all="ignore"):
        sx = ((q[fq, 0] + f32(1.0)) * f32(0.5)) * f32(W)
        sy = ((q[fq, 1] + f32(1.0)) * f32(0.5)) * f32(H)
        fx = px[fp].astype(np.float32) + f32(0.5)
        fy = py[fp].astype(np.float32) + f32(0.5)
        dx, dy = sx - fx, sy - fy
        A, B, Cc = f32(-0.5) * q[fq, 12], f32(-0.5) * q[fq, 14], -q[fq, 13]
        alpha = (A * (dx * dx) + B * (dy * dy)) + Cc * (dx * dy)
        g = np.exp(alpha.astype(np.float64)).astype(np.float32)
        op = q[fq, 11]
        opg = op * g
        src = {
            "P": [q[fq, 20] * g, q[fq, 21] * g, q[fq, 22] * g, g],
            "N": [q[fq, 16] * g, q[fq, 17] * g, q[fq, 18] * g, opg],
            "D": [q[fq, 15] * g, opg],
            "M": [_clamp(q[fq, 19] * g), _clamp(q[fq, 23] * g), _clamp(g)],
        }
        if mode == 4:
            one = np.ones(fq.size, np.float32)
            src["A"] = [one * f32(0.01), one * f32(0.005), one * f32(0.0), one * f32(0.01)]
        else:
            src["A"] = [_clamp((q[fq, 8] * op) * g), _clamp((q[fq, 9] * op) * g), _clamp((q[fq, 10] * op) * g), _clamp(opg)]
        st = {"P": np.zeros((npx, 4), np.float32), "N": np.zeros((npx, 4), np.float32), "D": np.zeros((npx, 2), np.float32),
              "A": np.zeros((npx, 4), np.float32), "M": np.zeros((npx, 3), np.float32)}
        q8 = {"A", "M"}
        by_rank = np.argsort(rank, kind="stable")
        bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2 if rank.size else 1))
        for r in range(len(bounds) - 1):
            sel = by_rank[bounds[r]:bounds[r + 1]]
            p = fp[sel]
            for key, planes in st.items():
                dst = planes[p]
                t = f32(1.0) - dst[:, -1]
                for ch in range(dst.shape[1]):
                    sv = src[key][ch][sel]
                    r_ = sv + dst[:, ch] if mode == 4 else sv * t + dst[:, ch]
                    dst[:, ch] = _unorm8(r_) if key in q8 else _h(r_)
                planes[p] = dst
    def u8(v):
        return np.rint(v * f32(255.0)).astype(np.uint8)
    P, N, D, Al, M = st["P"], st["N"], st["D"], st["A"], st["M"]
    zero = np.zeros(npx, np.float32)
    out = [P.astype(np.float16), N.astype(np.float16), u8(Al),
           np.stack([D[:, 0], D[:, 0], D[:, 0], D[:, 1]], 1).astype(np.float16),
           u8(np.stack([M[:, 0], M[:, 1], zero, M[:, 2]], 1))]
    return [a.reshape(wh, ww, 4) for a in out], int(s["skip"].sum())


def random_quads(n: int, W: int, H: int, seed: int = 0, max_px: float = 24.0, opacity=(0.2, 1.0)) -> np.ndarray:
    """Plausible prepass output: means inside the frame (some outside), rotated axes of up to max_px pixels, a positive definite
    conic that matches them (3 sigma at the axis ends), colours / normals / positions in their usual ranges."""
    rng = np.random.default_rng(seed)
    q = np.zeros((n, 24), np.float32)
    q[:, 0] = rng.uniform(-1.1, 1.1, n)
    q[:, 1] = rng.uniform(-1.1, 1.1, n)
    q[:, 2] = rng.uniform(-1, 1, n)
    q[:, 3] = 1.0
    th = rng.uniform(0, np.pi, n)
    l1 = rng.uniform(1.0, max_px, n)
    l2 = l1 * rng.uniform(0.2, 1.0, n)
    ux, uy = np.cos(th), np.sin(th)
    q[:, 4] = l1 * ux / (W * 0.5)
    q[:, 5] = l1 * uy / (H * 0.5)
    q[:, 6] = l2 * uy / (W * 0.5)
    q[:, 7] = -l2 * ux / (H * 0.5)
    s1, s2 = (l1 / 3.0) ** 2, (l2 / 3.0) ** 2           # covariance eigenvalues (px^2)
    cxx = ux * ux * s1 + uy * uy * s2
    cxy = ux * uy * (s1 - s2)
    cyy = uy * uy * s1 + ux * ux * s2
    det = cxx * cyy - cxy * cxy
    q[:, 12] = cyy / det
    q[:, 13] = -cxy / det
    q[:, 14] = cxx / det
    q[:, 15] = rng.uniform(0.5, 20, n)
    q[:, 8:11] = rng.uniform(0, 1, (n, 3))
    q[:, 11] = rng.uniform(*opacity, n)
    nv = rng.normal(size=(n, 3))
    q[:, 16:19] = nv / np.linalg.norm(nv, axis=1, keepdims=True)
    q[:, 19] = rng.uniform(0, 1, n)
    q[:, 20:23] = rng.uniform(-3, 3, (n, 3))
    q[:, 23] = rng.uniform(0, 1, n)
    return q


def quad_at(W: int, H: int, px: int, py: int, half_px: float, rgb=(0.8, 0.4, 0.2), a: float = 0.75, conic=(0.05, 0.0, 0.05),
            depth: float = 3.0, normal=(0.0, 0.6, 0.8), metallic: float = 0.25, ws=(1.0, -2.0, 0.5), roughness: float = 0.5) -> np.ndarray:
    """One axis-aligned quad whose mean sits exactly on the centre of pixel (px, py): screen = fragcoord there, so g = exp(0) = 1."""
    q = np.zeros(24, np.float32)
    q[0] = f32((px + 0.5) / (W * 0.5) - 1.0)
    q[1] = f32((py + 0.5) / (H * 0.5) - 1.0)
    # the mean must map back to the pixel centre exactly: screen = ((m + 1) * 0.5) * W
    assert ((q[0] + f32(1)) * f32(0.5)) * f32(W) == f32(px + 0.5) and ((q[1] + f32(1)) * f32(0.5)) * f32(H) == f32(py + 0.5)
    q[3] = 1.0
    q[4] = f32(half_px / (W * 0.5))
    q[7] = f32(half_px / (H * 0.5))
    q[8:11] = rgb
    q[11] = a
    q[12:15] = conic
    q[15] = depth
    q[16:19] = normal
    q[19] = metallic
    q[20:23] = ws
    q[23] = roughness
    return q
