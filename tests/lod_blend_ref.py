"""numpy restatement of m2s_lod_blend (the pin is in include/m2s.h), on top of tests/lod_ref.py: the transition weight t of every record
of a cut, the choice among the eight turns of the parent's frame, and the lerp of records and SH rows.  float32 arithmetic with one
rounding per operation (numpy's float32 array operations neither contract nor reassociate) and the IEEE division: the device is
compared for equality, bit for bit."""
import numpy as np

import lod_ref as lr

F = np.float32
KC = F(0.70710678118654752)
UNIT_TOL = F(2.0 ** -10)
COUNTS = ("records", "blended", "saturated", "turned")
ODD = np.array([k & 1 for k in range(8)], bool)
# which words of a record are lerped plainly, kept, or go through the frame rule
LERPED = (0, 1, 2, 4, 5, 6, 7, 10, 12, 13, 14, 20, 21)
KEPT = (3, 11, 15, 22, 23)
EDGES, ROT = (8, 9), (16, 17, 18, 19)


def q_of(b, camera_position, focal_px, near):
    """(s * s) / d2 per bound, d2 and s as lod_ref.refine computes them"""
    b = np.asarray(b, F).reshape(-1, 4)
    c = [F(v) for v in camera_position]
    with np.errstate(all="ignore"):
        dx, dy, dz = b[:, 0] - c[0], b[:, 1] - c[1], b[:, 2] - c[2]
        d2 = np.fmax((dx * dx + dy * dy) + dz * dz, F(near) * F(near))
        s = b[:, 3] * F(focal_px)
        out = (s * s) / d2
    assert out.dtype == F
    return out


def weights(b, parent, ids, camera_position, focal_px, tau_px, near, band, info=None):
    """pin 2 -> t per record (float32, every zero +0).  info (a dict): gets "den": den per record, NaN where the node has no parent.
    tau_px may be an array of shape (K, 1): t is then (K, records)."""
    b = np.asarray(b, F).reshape(-1, 4)
    parent = np.asarray(parent, np.uint32)
    ids = np.asarray(ids, np.uint32).astype(np.int64)
    p = parent[ids]
    has = p != lr.NO_PARENT
    pi = np.where(has, p, 0).astype(np.int64)
    q = q_of(b, camera_position, focal_px, near)
    band = F(band)
    with np.errstate(all="ignore"):
        qi, qp = q[ids], q[pi]
        den = qp - qi
        tau = np.asarray(tau_px, F)
        num = tau * tau - qi
        t_raw = num / den
        t = np.fmin(np.fmax((t_raw - (F(1) - band)) / band, F(0)), F(1))
        t = np.where(has & (den > 0) & (t > 0), t, F(0)).astype(F)
    assert t.dtype == F and t_raw.dtype == F
    if info is not None:
        info["den"] = np.where(has, den, F(np.nan))
    return t


def raw_candidates(r):
    """the eight turns of a stored quaternion (w, x, y, z) = r[..., 0..3], unscaled: (..., 8, 4) float32, each component one sum or a copy"""
    r = np.asarray(r, F)
    w, x, y, z = r[..., 0], r[..., 1], r[..., 2], r[..., 3]
    with np.errstate(all="ignore"):
        rows = [(w, x, y, z), (w - z, x + y, y - x, z + w), (-z, y, -x, w), (w + z, x - y, y + x, z - w),
                (-x, w, z, -y), (-(x + y), w - z, w + z, x - y), (-y, -z, w, x), (y - x, w + z, z - w, -(x + y))]
        out = np.stack([np.stack(row, -1) for row in rows], -2).astype(F)
    return out


def candidates(r):
    """raw_candidates with kC applied to the odd ones: eight quaternions of the same norm as r"""
    raw = raw_candidates(r)
    with np.errstate(all="ignore"):
        return np.where(ODD[:, None], raw * KC, raw).astype(F)


def is_unit(r):
    r = np.asarray(r, F)
    w, x, y, z = r[..., 0], r[..., 1], r[..., 2], r[..., 3]
    with np.errstate(all="ignore"):
        return np.abs(((w * w + x * x) + (y * y + z * z)) - F(1)) <= UNIT_TOL


def frame(c, r):
    """pin 5 for child quaternions c (n, 4) and parent quaternions r (n, 4) -> (k (n,) int, cand (n, 4) float32)"""
    c, r = np.asarray(c, F).reshape(-1, 4), np.asarray(r, F).reshape(-1, 4)
    raw = raw_candidates(r)
    with np.errstate(all="ignore"):
        cc = c[:, None, :]
        d = (cc[..., 0] * raw[..., 0] + cc[..., 1] * raw[..., 1]) + (cc[..., 2] * raw[..., 2] + cc[..., 3] * raw[..., 3])
        score = d * d
        score = np.where(ODD, score * F(0.5), score).astype(F)
        unit = is_unit(r)
        k = np.zeros(len(c), np.int64)
        best = score[:, 0].copy()
        for j in range(1, 8):
            win = unit & (score[:, j] > best)                                        # (false for a NaN on either side)
            k = np.where(win, j, k)
            best = np.where(win, score[:, j], best)
        idx = np.arange(len(c))
        cand = candidates(r)[idx, k]
        cand = np.where((d[idx, k] < 0)[:, None], -cand, cand).astype(F)
    assert d.dtype == F and score.dtype == F
    return k, cand


def lerp(t, a, b):
    """u * a + t * b with u = 1 - t: two products, one sum"""
    t = np.asarray(t, F)
    with np.errstate(all="ignore"):
        out = (F(1) - t) * np.asarray(a, F) + t * np.asarray(b, F)
    assert out.dtype == F
    return out


def blend_records(tree, parent, ids, t):
    """pins 3 to 5 -> (records (n, 24) float32, k per record: the turn, 0 where t == 0)"""
    tree = np.ascontiguousarray(tree, F).reshape(-1, 24)
    ids = np.asarray(ids, np.uint32).astype(np.int64)
    t = np.asarray(t, F)
    out = tree[ids].copy()
    on = np.flatnonzero(t != 0)
    k = np.zeros(len(ids), np.int64)
    if not on.size:
        return out, k
    a = tree[ids[on]]
    b = tree[np.asarray(parent, np.uint32)[ids[on]].astype(np.int64)]
    tt = t[on]
    res = a.copy()
    res[:, LERPED] = lerp(tt[:, None], a[:, LERPED], b[:, LERPED])
    kk, cand = frame(a[:, ROT], b[:, ROT])
    odd = (kk & 1) == 1
    target = np.where(odd[:, None], b[:, EDGES[::-1]], b[:, EDGES])
    res[:, EDGES] = lerp(tt[:, None], a[:, EDGES], target)
    res[:, ROT] = lerp(tt[:, None], a[:, ROT], cand)
    out[on] = res
    k[on] = kk
    return out, k


def blend_sh(tree_sh, parent, ids, t):
    """pin 6 -> rows (n, 48) float32"""
    tree_sh = np.ascontiguousarray(tree_sh, F).reshape(-1, 48)
    ids = np.asarray(ids, np.uint32).astype(np.int64)
    t = np.asarray(t, F)
    out = tree_sh[ids].copy()
    on = np.flatnonzero(t != 0)
    if on.size:
        out[on] = lerp(t[on][:, None], tree_sh[ids[on]], tree_sh[np.asarray(parent, np.uint32)[ids[on]].astype(np.int64)])
    return out


def blend(tree, parent, b, ids, camera_position, focal_px, tau_px, near, band, tree_sh=None):
    """the whole pass over the records of a cut whose nodes are ids -> {"t", "records", "k", "counts": m2s_lod_blend's out_counts by name,
    "den", "sh" (with tree_sh)}"""
    info = {}
    t = weights(b, parent, ids, camera_position, focal_px, tau_px, near, band, info)
    rec, k = blend_records(tree, parent, ids, t)
    counts = {"records": len(t), "blended": int(np.count_nonzero(t > 0)), "saturated": int(np.count_nonzero(t == 1)),
              "turned": int(np.count_nonzero((t > 0) & (k != 0)))}
    out = {"t": t, "records": rec, "k": k, "counts": counts, "den": info["den"]}
    if tree_sh is not None:
        out["sh"] = blend_sh(tree_sh, parent, ids, t)
    return out
