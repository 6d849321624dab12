"""Test infrastructure: a numpy restatement of the contribution pass exactly as include/m2s.h pins it (m2s_contrib_accumulate), built on
splat_ref.setup and its fragment enumeration.  Not imported by the product.

It tracks the albedo attachment's alpha alone, fp32 operation by operation: per fragment sA3 = clamp01(a * g), tA = 1 - A3,
w = sA3 * tA, A3 <- unorm8(w + A3); exp is float64 exp rounded to fp32 — the one step the kernel may do differently.  It never stops
early."""
from __future__ import annotations

import numpy as np

import splat_ref
from splat_ref import f32

# |w_gpu - w_ref| <= one quantisation step of the destination alpha (times sA3 <= 1) + the rounding of the device's fast exp: the 1 LSB
# tests/test_gpu_splat.py allows the plane itself
W_BAR = 1.0 / 255.0 + 1e-5
# the largest difference measured on MI355X over the cases of tests/test_gpu_contrib.py: 5.96e-8, one ulp of a weight below 1
# (DESIGN.md 5.14), and the guard at 4 x it, as tests/parity.py keeps one beside its bar
W_ACHIEVED = 6.0e-8
W_GUARD = 4 * W_ACHIEVED


def fragments(s: dict):
    """-> (quad, pixel index y * W + x) of every fragment, per pixel in array order (triangle 0 before triangle 1 of one quad), and
    the rank of each fragment in its pixel's list."""
    W, H = s["W"], s["H"]
    fq, fp, fk = [], [], []
    for t, tri in enumerate(s["tris"]):
        for qi in np.nonzero(tri["valid"])[0]:
            x0, y0, x1, y1 = (int(v) for v in tri["box"][qi])
            xs, ys = np.meshgrid(np.arange(x0, x1 + 1, dtype=np.int64), np.arange(y0, y1 + 1, dtype=np.int64))
            Px, Py = 256 * xs + 128, 256 * ys + 128
            inside = np.ones(xs.shape, bool)
            for i in range(3):
                E = tri["a"][qi, i] * Px + tri["b"][qi, i] * Py + tri["c"][qi, i]
                inside &= (E > 0) | ((E == 0) & bool(tri["bias"][qi, i]))
            p = (ys * W + xs)[inside]
            fq.append(np.full(p.size, qi, np.int64))
            fp.append(p)
            fk.append(np.full(p.size, qi * 2 + t, np.int64))
    if not fq:
        z = np.zeros(0, np.int64)
        return z, z, z
    fq, fp, fk = np.concatenate(fq), np.concatenate(fp), np.concatenate(fk)
    o = np.lexsort((fk, fp))
    fq, fp = fq[o], fp[o]
    start = np.ones(fp.size, bool)
    start[1:] = fp[1:] != fp[:-1]
    run0 = np.maximum.accumulate(np.where(start, np.arange(fp.size), 0))
    return fq, fp, np.arange(fp.size) - run0


def contrib(quads, W: int, H: int, count_weight: float = 0.0, bar: float = 0.0, s: dict | None = None) -> dict:
    """-> dict(wmax: uint32[n] bits of the largest fragment weight per quad, n / n_lo / n_hi: int64[n] fragments with
    w > count_weight (the restatement's own count) / w > count_weight + bar / w > count_weight - bar, alpha: uint8 (H, W) the final
    albedo alpha, row 0 = bottom)."""
    if s is None:
        s = splat_ref.setup(quads, W, H)
    q = s["q"]
    n = q.shape[0]
    fq, fp, rank = fragments(s)
    wmax = np.zeros(n, np.float32)
    n_lo = np.zeros(n, np.int64)
    n_hi = np.zeros(n, np.int64)
    n_at = np.zeros(n, np.int64)
    A3 = np.zeros(W * H, np.float32)
    with np.errstate(all="ignore"):
        sx = ((q[fq, 0] + f32(1.0)) * f32(0.5)) * f32(W)
        sy = ((q[fq, 1] + f32(1.0)) * f32(0.5)) * f32(H)
        fx = (fp % W).astype(np.float32) + f32(0.5)
        fy = (fp // W).astype(np.float32) + f32(0.5)
        dx, dy = sx - fx, sy - fy
        A, B, Cc = f32(-0.5) * q[fq, 12], f32(-0.5) * q[fq, 14], -q[fq, 13]
        alpha = (A * (dx * dx) + B * (dy * dy)) + Cc * (dx * dy)
        g = np.exp(alpha.astype(np.float64)).astype(np.float32)
        sA3 = splat_ref._clamp(q[fq, 11] * g)
        by_rank = np.argsort(rank, kind="stable")
        bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2 if rank.size else 1))
        cw = np.float64(np.float32(count_weight))
        for r in range(len(bounds) - 1):
            sel = by_rank[bounds[r]:bounds[r + 1]]          # at most one fragment per pixel
            p = fp[sel]
            tA = f32(1.0) - A3[p]
            w = sA3[sel] * tA
            np.maximum.at(wmax, fq[sel], w)
            np.add.at(n_at, fq[sel], (w.astype(np.float64) > cw).astype(np.int64))
            np.add.at(n_lo, fq[sel], (w.astype(np.float64) > cw + bar).astype(np.int64))
            np.add.at(n_hi, fq[sel], (w.astype(np.float64) > cw - bar).astype(np.int64))
            A3[p] = splat_ref._unorm8(w + A3[p])
    return dict(wmax=wmax.view(np.uint32).copy(), n=n_at, n_lo=n_lo, n_hi=n_hi,
                alpha=np.rint(A3 * f32(255.0)).astype(np.uint8).reshape(H, W))


def per_record(c: dict, sources, n_records: int) -> dict:
    """The per-quad result folded onto records: maximum of wmax, sums of n / n_lo / n_hi."""
    src = np.asarray(sources, np.int64)
    w = np.zeros(n_records, np.uint32)
    lo = np.zeros(n_records, np.int64)
    hi = np.zeros(n_records, np.int64)
    at = np.zeros(n_records, np.int64)
    np.maximum.at(w, src, c["wmax"])
    np.add.at(at, src, c["n"])
    np.add.at(lo, src, c["n_lo"])
    np.add.at(hi, src, c["n_hi"])
    return dict(wmax=w, n=at, n_lo=lo, n_hi=hi)
