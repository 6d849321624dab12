"""Test infrastructure: a numpy restatement of the colour refit exactly as include/m2s.h pins it (m2s_refit_accumulate,
m2s_refit_apply), built on splat_ref.setup and contrib_ref.fragments.  Not imported by the product.

accumulate() tracks the albedo attachment's alpha as contrib_ref.contrib does (fp32 operation by operation, exp = float64 exp rounded to
fp32 — the one step the kernel may do differently) and never stops early; everything behind the weight is integer arithmetic.
apply() is float64 operation by operation."""
from __future__ import annotations

import numpy as np

import contrib_ref
import splat_ref
from splat_ref import f32

EQ_ONE = 4096
WQ_ONE = 65536
# |wq_gpu - wq_ref| per fragment: the project's bar on the weight itself (contrib_ref.W_BAR: one quantisation step of the destination
# alpha + the rounding of the device's fast exp) in units of 1 / 65536, rounded up.  A record with F fragments (the restatement's count)
# may differ by F * WQ_BAR in den and by F * WQ_BAR * 4096 in a num word (|eq| <= 4096).
WQ_BAR = int(np.ceil(contrib_ref.W_BAR * WQ_ONE))          # 258
assert WQ_BAR == 258
# the largest differences of a record's words measured on MI355X over the cases of tests/test_gpu_refit.py: |d den| = 3
# and |d num| = 5498, on the record of one quad over 64 tiles (16 thousand fragments); 99 % of all records are bit-identical.  The guards
# at 4 x them, as contrib_ref.W_GUARD is kept beside W_BAR
DEN_ACHIEVED = 3
NUM_ACHIEVED = 5498
DEN_GUARD = 4 * DEN_ACHIEVED
NUM_GUARD = 4 * NUM_ACHIEVED


def error_q(m, s, sa):
    """eq = floor((2 n + d) / (2 d)) clamped to +-4096 with n = 4096 (m sa - 255 s), d = 255 sa (sa >= 1); integer arrays broadcast."""
    m, s, sa = (np.asarray(v, np.int64) for v in (m, s, sa))
    n = EQ_ONE * (m * sa - 255 * s)
    d = 255 * sa
    return np.clip((2 * n + d) // (2 * d), -EQ_ONE, EQ_ONE)          # (numpy's // floors)


def participation(target, render, min_cover: int):
    """-> (mask bool[H * W], eq int64[H * W, 3]) of two (H, W, 4) uint8 planes, row 0 = bottom; eq is 0 where the pixel takes no part."""
    t = np.ascontiguousarray(target, np.uint8).reshape(-1, 4).astype(np.int64)
    r = np.ascontiguousarray(render, np.uint8).reshape(-1, 4).astype(np.int64)
    sa = r[:, 3]
    mask = (t[:, 3] != 0) & (sa >= int(min_cover))
    eq = np.zeros((t.shape[0], 3), np.int64)
    eq[mask] = error_q(t[mask, :3], r[mask, :3], sa[mask, None])
    return mask, eq


def accumulate(quads, sources, n_records: int, W: int, H: int, target, render, min_cover: int, s: dict | None = None) -> dict:
    """-> dict(num int64 (n_records, 3), den uint64 (n_records,), frags int64 (n_records,): every fragment of the record's quads,
    participating or not — the F of the bars —, pixels: participating pixels, pairs: the (tile, quad) pairs)."""
    if not 1 <= int(min_cover) <= 255:
        raise ValueError("min_cover is 1..255")
    if s is None:
        s = splat_ref.setup(quads, W, H)
    q = s["q"]
    src = np.asarray(sources, np.int64)
    mask, eq = participation(target, render, min_cover)
    fq, fp, rank = contrib_ref.fragments(s)
    num = np.zeros((n_records, 3), np.int64)
    den = np.zeros(n_records, np.int64)
    frags = np.zeros(n_records, np.int64)
    np.add.at(frags, src[fq], 1)
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
        for r in range(len(bounds) - 1):
            sel = by_rank[bounds[r]:bounds[r + 1]]          # at most one fragment per pixel
            p = fp[sel]
            tA = f32(1.0) - A3[p]
            w = sA3[sel] * tA
            wq = np.rint(w * f32(WQ_ONE)).astype(np.int64)
            take = mask[p]
            rec = src[fq[sel]][take]
            np.add.at(den, rec, wq[take])
            np.add.at(num, rec, wq[take, None] * eq[p[take]])
            A3[p] = splat_ref._unorm8(w + A3[p])
    return dict(num=num, den=den.astype(np.uint64), frags=frags, pixels=int(mask.sum()), pairs=int(splat_ref.tile_counts(s).sum()))


def threshold(min_weight_sum: float) -> int:
    """D = llrint((double)min_weight_sum * 65536), saturating at 2^64 - 1."""
    dq = float(np.float32(min_weight_sum)) * 65536.0
    return (1 << 64) - 1 if dq >= 2.0 ** 63 else int(np.rint(dq))


def apply(records, num, den, step: float = 1.0, min_weight_sum: float = 1.0):
    """-> (records after the update, (n, 24) float32; counts dict(records, updated, clamped, no_weight))."""
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, 24).copy()
    num = np.asarray(num, np.int64).reshape(-1, 3)
    den = np.asarray(den, np.uint64).reshape(-1)
    D = threshold(min_weight_sum)
    starved = np.array([int(d) == 0 or int(d) < D for d in den], bool)
    live = ~starved
    st = np.float64(np.float32(step))
    clamped = np.zeros(rec.shape[0], bool)
    with np.errstate(all="ignore"):
        scale = den.astype(np.float64) * 4096.0
        for k in range(3):
            c = rec[:, 4 + k]
            ok = live & np.isfinite(c)
            dlt = num[:, k].astype(np.float64) / scale
            v = c.astype(np.float64) + st * dlt
            cl = np.fmin(np.fmax(v, 0.0), 1.0)
            clamped |= ok & (cl != v)
            rec[ok, 4 + k] = cl[ok].astype(np.float32)
    return rec, dict(records=int(rec.shape[0]), updated=int(live.sum()), clamped=int(clamped.sum()), no_weight=int(starved.sum()))


def assert_within_bars(num, den, ref: dict, what: str) -> None:
    """The device's accumulators against accumulate()'s: within the bars of the header, and within 4 x what MI355X achieved."""
    num = np.asarray(num, np.int64).reshape(-1, 3)
    den = np.asarray(den, np.uint64).astype(np.int64)
    F = ref["frags"]
    dd = np.abs(den - ref["den"].astype(np.int64))
    dn = np.abs(num - ref["num"]).max(axis=1)
    print(f"{what}: max |d den| = {int(dd.max(initial=0))}, max |d num| = {int(dn.max(initial=0))}, bit-identical records: "
          f"{float(((dd == 0) & (dn == 0)).mean()):.4f}, max |d den| / F = {np.where(F > 0, dd / np.maximum(F, 1), 0.0).max(initial=0.0):.4g}, "
          f"max |d num| / (4096 F) = {np.where(F > 0, dn / np.maximum(F, 1) / EQ_ONE, 0.0).max(initial=0.0):.4g}")
    assert (dd <= F * WQ_BAR).all() and (dn <= F * WQ_BAR * EQ_ONE).all(), what
    assert dd.max(initial=0) <= DEN_GUARD and dn.max(initial=0) <= NUM_GUARD, f"{what}: within the bars but beyond 4 x the achieved difference"
