"""M2S_MERGE_UNSIGNED_AXIS restated in numpy: pins 2u and 5u of include/m2s.h ("merge pass") on top of tests/merge_ref.py, whose order,
segments, bars and comparison are used as they are.  Pin 2u drops the sign of pin 2's fp32 dot before the comparison; pin 5u orients
the members' third rows one after the other, each against the oriented row of the member before it, in float64 with the dot written
(x x + y y) + z z — the kernel evaluates the same expressions on the same float64 rows, so the two must take the same sign decisions,
not similar ones.  parent() is merge_ref.parent with o_i in r3_i's place and is otherwise the same arithmetic, operation for operation:
where nothing flips the two produce the same bytes."""
import numpy as np

import compact_ref as cr
import lod_ref as lr
import merge_ref as mr

F = np.float32
DRY_RUN = 1
UNSIGNED_AXIS = 4                                   # M2S_MERGE_UNSIGNED_AXIS: bit 2; bit 1 names nothing
MERGE_FLAGS_ACCEPTED = (0, 1, 4, 5)                 # m2s_merge_params.flags
MERGE_FLAGS_REFUSED = (2, 3, 6, 7, 8)
BUILD_FLAGS_ACCEPTED = (0, 4)                       # m2s_lod_build_params.flags (the word that was `reserved`)
BUILD_FLAGS_REFUSED = (1, 2, 3, 5, 6, 8)


def segment_heads(rec, level, max_group, min_axis_dot):
    """pins 1, 2u, 3 -> (perm, heads: the sorted positions that start a segment, ascending)"""
    rec = np.ascontiguousarray(rec, F).reshape(-1, 24)
    n = len(rec)
    perm, keys = mr.order(rec)
    if n == 0:
        return perm, np.zeros(0, np.int64)
    a = mr.axis3_f32(rec[perm][:, 16:20])
    with np.errstate(all="ignore"):
        d = ((a[1:, 0] * a[:-1, 0]) + a[1:, 1] * a[:-1, 1]) + a[1:, 2] * a[:-1, 2]
        assert d.dtype == F
        brk = ~(np.abs(d) >= F(min_axis_dot))
    inval = keys == mr.INVALID_KEY
    cell = keys >> np.uint32(3 * level)
    run = np.ones(n, bool)
    run[1:] = inval[1:] | inval[:-1] | (cell[1:] != cell[:-1]) | brk
    run_start = np.maximum.accumulate(np.where(run, np.arange(n), 0))
    return perm, np.flatnonzero((np.arange(n) - run_start) % max_group == 0)


def orient(r3):
    """pin 5u: r3 (m, 3) float64 in sorted order -> (o (m, 3), flipped (m,) bool).  o_0 = r3_0; o_i = -r3_i where
    (r3_i.x o.x + r3_i.y o.y) + r3_i.z o.z < 0 with o = o_{i-1}, else r3_i: a dot of zero or NaN does not flip."""
    r3 = np.asarray(r3, np.float64)
    o = r3.copy()
    flipped = np.zeros(len(r3), bool)
    with np.errstate(all="ignore"):
        for i in range(1, len(r3)):
            d = (r3[i, 0] * o[i - 1, 0] + r3[i, 1] * o[i - 1, 1]) + r3[i, 2] * o[i - 1, 2]
            if d < 0:
                o[i] = -r3[i]
                flipped[i] = True
    return o, flipped


def parent(members):
    """pins 5 + 5u: as merge_ref.parent; the info also has "flipped", the members pin 5u turned"""
    r = np.asarray(members, np.float64)
    first32 = np.asarray(members, F)[0]
    with np.errstate(all="ignore"):
        sx, sy = r[:, 8], r[:, 9]
        w = sx * sy
        if w.sum() == 0:
            w = np.ones(len(r))
        W = w.sum()
        d = r[:, 0:3] - r[0, 0:3]
        mu = (w[:, None] * d).sum(0) / W
        r1, r2, r3 = mr.rows_f64(r[:, 16:20])
        o, flipped = orient(r3)
        nb = (w[:, None] * o).sum(0)
        l2 = nb @ nb
        if not (l2 > 0) or not np.isfinite(l2):
            nb = r3[0].copy()
            l2 = nb @ nb
        nb = nb / np.sqrt(l2) if (l2 > 0 and np.isfinite(l2)) else np.array([0.0, 0.0, 1.0])
        t1 = mr._tangent(r1[0], nb)
        if t1 is None:
            t1 = mr._tangent(r2[0], nb)
        if t1 is None:
            t1 = r1[0]
        t2 = np.cross(nb, t1)
        e = d - mu
        M = (np.einsum("i,ij,ik->jk", w * sx * sx / 12.0, r1, r1) + np.einsum("i,ij,ik->jk", w * sy * sy / 12.0, r2, r2) +
             np.einsum("i,ij,ik->jk", w, e, e)) / W
        a, b, c = t1 @ M @ t1, t1 @ M @ t2, t2 @ M @ t2
        dl = np.sqrt((a - c) ** 2 + 4 * b * b)
        lam1, lam2 = (a + c + dl) / 2, max((a + c - dl) / 2, 0.0)
        if dl == 0:
            e1 = t1
        else:
            v, u = np.array([b, lam1 - a]), np.array([lam1 - c, b])
            if u @ u > v @ v:
                v = u
            v = v / np.sqrt(v @ v)
            e1 = v[0] * t1 + v[1] * t2
        e2 = np.cross(nb, e1)
        out = np.zeros(24, np.float64)
        out[0:3] = r[0, 0:3] + mu
        alpha_w = w * r[:, 7]
        out[7] = alpha_w.sum() / W
        out[4:7] = (alpha_w[:, None] * r[:, 4:7]).sum(0) / alpha_w.sum() if alpha_w.sum() != 0 else (w[:, None] * r[:, 4:7]).sum(0) / W
        out[8], out[9] = np.sqrt(12 * lam1), np.sqrt(12 * lam2)
        ns = (w[:, None] * r[:, 12:15]).sum(0)
        nl2 = ns @ ns
        out[12:15] = ns / np.sqrt(nl2) if (nl2 > 0 and np.isfinite(nl2)) else 0.0
        out[16:20] = mr.quat_cast_wxyz(e1, e2, nb)
        out[20:22] = (w[:, None] * r[:, 20:22]).sum(0) / W
        out = out.astype(F)
    for k in mr.COPIED:
        out[k] = first32[k]                              # the first member's bits
    cov = 12 * (a * np.outer(t1, t1) + b * (np.outer(t1, t2) + np.outer(t2, t1)) + c * np.outer(t2, t2)) + float(first32[10]) ** 2 * np.outer(nb, nb)
    return out, {"cov": cov, "l1": lam1, "l2": lam2, "M": M, "nb": nb, "e1": e1, "flipped": flipped}


def merge(rec, level, max_group=4, min_axis_dot=0.5):
    """merge_ref.merge with pins 2u and 5u -> (records after, map, counts, info)"""
    rec = np.ascontiguousarray(rec, F).reshape(-1, 24)
    n = len(rec)
    perm, heads = segment_heads(rec, level, max_group, min_axis_dot)
    S = len(heads)
    ends = np.append(heads[1:], n)
    out = np.zeros((S, 24), F)
    mp = np.zeros(n, np.uint32)
    info = []
    for s in range(S):
        idx = perm[heads[s]:ends[s]]
        mp[idx] = s
        if len(idx) == 1:
            out[s] = rec[idx[0]]
            info.append(None)
        else:
            out[s], i = parent(rec[idx])
            info.append(i)
    counts = {"before": n, "after": S, "merged": int(np.count_nonzero(ends - heads >= 2)), "invalid": int(n - np.count_nonzero(cr.valid_mask(rec)))}
    return out, mp, counts, info


def chain(rec, levels, max_group=4, min_axis_dot=0.5, merge_fn=None):
    """the merges one after the other, as m2s_lod_build runs them (a step that merges nothing adds no level and leaves the records in
    the order of the level below) -> (the levels' records, parent, first).  merge_fn: merge (default) or merge_ref.merge."""
    merge_fn = merge_fn or merge
    out, maps = [np.ascontiguousarray(rec, F).reshape(-1, 24)], []
    for lv in levels:
        nxt, m, counts, _ = merge_fn(out[-1], lv, max_group, min_axis_dot)
        if counts["after"] == len(out[-1]):
            continue
        out.append(nxt)
        maps.append(m)
    parent_, first = lr.link(maps, [len(v) for v in out])
    return out, parent_, first
