"""The merge pass of include/m2s.h ("merge pass") restated in numpy.  Order is the compact export's (tests/compact_ref.py: validity, box,
keys, the stable sort); runs and segments are integer logic and fp32 operation by operation, so they must equal the device's exactly;
the parent of a segment is float64 throughout and written as the pin writes it (the full 3 x 3 moment M, then its projections), where
the kernel accumulates the three projections directly: two formulations of one definition.

Bars.  Segmentation, counts, map and the bytes of copied records are exact.  A parent's scalar fields are fp32 roundings of an fp64
computation whose own error is far below an fp32 ulp: the bar is 4 fp32 ulps OF THE FIELD'S MAGNITUDE, the field being position.xyz,
colour.rgb, alpha, normal.xyz, pbr[0..1] and the pair of edges, its magnitude the largest |component| of the restatement's value (a
component that cancels to nearly nothing — one coordinate of a centroid, the short edge of a collinear group — carries the absolute
error of the large ones, not its own ulp).  The rotation is compared through the viewer covariance it produces: sum s_i^2 r_i r_i^T of
the parent's stored floats in float64 against 12 M projected on the plane (+ the third scale's own term), elementwise within
1e-5 * 12 l1; the fp32 rounding of six stored numbers perturbs it by about 1e-6.

ACHIEVED (the project's convention: what the MI355X measured over every case of tests/test_gpu_merge.py against THIS restatement, and a
guard at 4 x it beside the bar): see SCALAR_ULPS_ACHIEVED / COV_REL_ACHIEVED below and DESIGN 5.18."""
import numpy as np

import compact_ref as cr

F = np.float32
INVALID_KEY = np.uint32(1 << 30)
COUNTS = ("before", "after", "merged", "invalid")
SCALAR_ULPS_BAR = 4.0
COV_REL_BAR = 1e-5
# measured on MI355X over the cases of tests/test_gpu_merge.py (profiles/merge/gpu_tests.log): the largest error of a scalar field in
# fp32 ulps of the field's magnitude, and of a covariance element relative to 12 l1
SCALAR_ULPS_ACHIEVED = 0.153
COV_REL_ACHIEVED = 3.24e-7
SCALAR_ULPS_GUARD = 4 * SCALAR_ULPS_ACHIEVED
COV_REL_GUARD = 4 * COV_REL_ACHIEVED


def rows_f64(q):
    """r_1, r_2, r_3 of castQuatToMat3 of the stored floats (x, y, z, w) = q[0..3], float64; q: (..., 4) -> three (..., 3)"""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    r1 = np.stack([1 - 2 * (z * z + w * w), 2 * (y * z + x * w), 2 * (y * w - x * z)], -1)
    r2 = np.stack([2 * (y * z - x * w), 1 - 2 * (y * y + w * w), 2 * (z * w + x * y)], -1)
    r3 = np.stack([2 * (y * w + x * z), 2 * (z * w - x * y), 1 - 2 * (y * y + z * z)], -1)
    return r1, r2, r3


def axis3_f32(q):
    """r_3 in fp32, one rounding per operation"""
    q = np.ascontiguousarray(q, F)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    with np.errstate(all="ignore"):
        return np.stack([F(2) * (y * w + x * z), F(2) * (z * w - x * y), F(1) - F(2) * (y * y + z * z)], 1).astype(F)


def viewer_cov(rec):
    """sum_i s_i^2 r_i r_i^T of one record's stored floats, float64 (3, 3): what gaussian_cov3d draws at std_dev 1, identity model"""
    rec = np.asarray(rec, np.float64)
    r = rows_f64(rec[16:20])
    return sum(rec[8 + k] ** 2 * np.outer(r[k], r[k]) for k in range(3))


def order(rec):
    """pin 1 -> (perm, sorted keys)"""
    rec = np.ascontiguousarray(rec, F).reshape(-1, 24)
    ok = cr.valid_mask(rec)
    src, bad = np.flatnonzero(ok), np.flatnonzero(~ok)
    if src.size:
        p = rec[src][:, 0:3]
        keys = cr.keys_of(p, cr.omin(p), cr.omax(p)).astype(np.uint32)
        o = np.argsort(keys, kind="stable")
        src, keys = src[o], keys[o]
    else:
        keys = np.zeros(0, np.uint32)
    return np.concatenate([src, bad]).astype(np.int64), np.concatenate([keys, np.full(bad.size, INVALID_KEY, np.uint32)])


def segment_heads(rec, level, max_group, min_axis_dot):
    """pins 1 - 3 -> (perm, heads: the sorted positions that start a segment, ascending)"""
    rec = np.ascontiguousarray(rec, F).reshape(-1, 24)
    n = len(rec)
    perm, keys = order(rec)
    if n == 0:
        return perm, np.zeros(0, np.int64)
    a = axis3_f32(rec[perm][:, 16:20])
    with np.errstate(all="ignore"):
        d = ((a[1:, 0] * a[:-1, 0]) + a[1:, 1] * a[:-1, 1]) + a[1:, 2] * a[:-1, 2]
        brk = ~(d >= F(min_axis_dot))
    inval = keys == INVALID_KEY
    cell = keys >> np.uint32(3 * level)
    run = np.ones(n, bool)
    run[1:] = inval[1:] | inval[:-1] | (cell[1:] != cell[:-1]) | brk
    run_start = np.maximum.accumulate(np.where(run, np.arange(n), 0))
    return perm, np.flatnonzero((np.arange(n) - run_start) % max_group == 0)


def quat_cast_wxyz(e1, e2, nb):
    """the conversion's quat_cast of the matrix with columns e1, e2, nb, float64 -> stored (w, x, y, z) with w >= 0"""
    m = (e1, e2, nb)
    fx, fy, fz, fw = m[0][0] - m[1][1] - m[2][2], m[1][1] - m[0][0] - m[2][2], m[2][2] - m[0][0] - m[1][1], m[0][0] + m[1][1] + m[2][2]
    bi, fb = 0, fw
    for k, f in ((1, fx), (2, fy), (3, fz)):
        if f > fb:
            fb, bi = f, k
    bv = np.sqrt(fb + 1.0) * 0.5
    mult = 0.25 / bv
    d0, d1, d2 = m[1][2] - m[2][1], m[2][0] - m[0][2], m[0][1] - m[1][0]
    s0, s1, s2 = m[0][1] + m[1][0], m[2][0] + m[0][2], m[1][2] + m[2][1]
    q = {0: (bv, d0 * mult, d1 * mult, d2 * mult), 1: (d0 * mult, bv, s0 * mult, s1 * mult), 2: (d1 * mult, s0 * mult, bv, s2 * mult),
         3: (d2 * mult, s1 * mult, s2 * mult, bv)}[bi]
    q = np.array(q, np.float64)
    return -q if q[0] < 0 else q


def _tangent(v, nb):
    p = v - (v @ nb) * nb
    l2 = p @ p
    if not (l2 >= 1e-12 * (v @ v)) or not (l2 > 0):
        return None
    return p / np.sqrt(l2)


def parent(members):
    """pin 5: members (m >= 2, 24) float32 in sorted order -> (the parent's 24 floats, {"cov": 12 M projected on the plane + the third
    scale's term (3, 3), "l1", "l2", "M": the full moment, "nb", "e1"})"""
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
        r1, r2, r3 = rows_f64(r[:, 16:20])
        nb = (w[:, None] * r3).sum(0)
        l2 = nb @ nb
        if not (l2 > 0) or not np.isfinite(l2):
            nb = r3[0].copy()
            l2 = nb @ nb
        nb = nb / np.sqrt(l2) if (l2 > 0 and np.isfinite(l2)) else np.array([0.0, 0.0, 1.0])
        t1 = _tangent(r1[0], nb)
        if t1 is None:
            t1 = _tangent(r2[0], nb)
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
        out[16:20] = quat_cast_wxyz(e1, e2, nb)
        out[20:22] = (w[:, None] * r[:, 20:22]).sum(0) / W
        out = out.astype(F)
    for k in (3, 10, 11, 15, 22, 23):
        out[k] = first32[k]                              # the first member's bits
    cov = 12 * (a * np.outer(t1, t1) + b * (np.outer(t1, t2) + np.outer(t2, t1)) + c * np.outer(t2, t2)) + float(first32[10]) ** 2 * np.outer(nb, nb)
    return out, {"cov": cov, "l1": lam1, "l2": lam2, "M": M, "nb": nb, "e1": e1}


def merge(rec, level, max_group=4, min_axis_dot=0.5):
    """-> (records after (S, 24) float32, map (n,) uint32, counts, info: per segment None (a copy) or parent()'s second result)"""
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


FIELDS = {"position": slice(0, 3), "colour": slice(4, 7), "alpha": slice(7, 8), "edges": slice(8, 10), "normal": slice(12, 15), "pbr": slice(20, 22)}
COPIED = (3, 10, 11, 15, 22, 23)


def compare(got, want, info):
    """device records against the restatement's -> {"scalar_ulps": the largest field error in fp32 ulps of the field's magnitude,
    "cov_rel": the largest covariance element error / (12 l1)}; copied records and copied words must be bit-identical (asserted)."""
    got = np.ascontiguousarray(got, F).reshape(-1, 24)
    assert got.shape == want.shape, (got.shape, want.shape)
    worst_u, worst_c = 0.0, 0.0
    for s, i in enumerate(info):
        if i is None:
            assert np.array_equal(got[s].view(np.uint32), want[s].view(np.uint32)), ("copied record differs", s)
            continue
        assert np.array_equal(got[s, list(COPIED)].view(np.uint32), want[s, list(COPIED)].view(np.uint32)), ("first member's words differ", s)
        for name, sl in FIELDS.items():
            g, w = got[s, sl].astype(np.float64), want[s, sl].astype(np.float64)
            if not np.isfinite(w).all():
                assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(w)], w[~np.isnan(w)]), (name, s)
                continue
            mag = np.abs(w).max()
            err = np.abs(g - w).max()
            if mag == 0:
                assert err == 0, (name, s, g, w)
                continue
            worst_u = max(worst_u, err / float(np.spacing(F(mag))))
        l1 = i["l1"]
        dc = np.abs(viewer_cov(got[s]) - i["cov"]).max()
        if l1 == 0:
            assert dc == 0, ("covariance of a parent without extent", s)
        else:
            worst_c = max(worst_c, dc / (12 * l1))
    return {"scalar_ulps": worst_u, "cov_rel": worst_c}


DIRECTIONS = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float64)


def crafted_records(n, seed=0, invalid=True):
    """n records for the device tests.  Positions come from a pool of about n / 3 points in clusters, so that records share keys at
    level 0, cells at level 3 and everything at level 10; third axes from six fixed directions with a random turn about them, so that
    every dot product of two of them is 1, 0 or -1 to rounding and none lies near a threshold of 0.5 or -2; scales random with zeros
    among them; with `invalid` a NaN position, a zero quaternion and a negative scale where there is room."""
    rng = np.random.default_rng(1000 + seed)
    rec = np.zeros((n, 24), F)
    pool = max(1, n // 3)
    centres = rng.normal(0, 1, (max(1, pool // 6), 3))
    pts = centres[rng.integers(0, len(centres), pool)] + rng.normal(0, 0.01, (pool, 3))
    rec[:, 0:3] = pts[rng.integers(0, pool, n)]
    rec[:, 3] = 1
    rec[:, 4:8] = rng.random((n, 4))
    rec[:, 7] = np.where(rng.random(n) < 0.1, 0, rec[:, 7])
    rec[:, 8:10] = np.exp(rng.normal(-3, 1, (n, 2))) * (rng.random((n, 2)) > 0.15)
    rec[:, 11] = rng.random(n)
    rec[:, 12:15] = rng.normal(0, 1, (n, 3))
    rec[:, 15] = rng.random(n)
    nb = DIRECTIONS[rng.integers(0, 6, n)]
    ang = rng.uniform(0, 2 * np.pi, n)
    for i in range(n):
        helper = DIRECTIONS[(int(np.argmax(np.abs(nb[i]))) // 2 * 2 + 2) % 6]
        u = np.cross(nb[i], helper)
        v = np.cross(nb[i], u)
        e1 = np.cos(ang[i]) * u + np.sin(ang[i]) * v
        rec[i, 16:20] = quat_cast_wxyz(e1, np.cross(nb[i], e1), nb[i])
    rec[:, 20:24] = rng.random((n, 4))
    if invalid:
        for k, (col, val) in enumerate(((0, np.nan), (16, 0.0), (8, -0.25))):
            if n > 8 * (k + 1):
                i = (n * (2 * k + 1)) // 7
                rec[i, col] = val
                if col == 16:
                    rec[i, 16:20] = 0
    return rec


def grid_records(k=8):
    """k x k tiles of edge 1 / k on z = 0, centres (i + 0.5) / k; the identity rotation, stored (w, x, y, z) = (1, 0, 0, 0): r_1, r_2, r_3 are
    the coordinate axes; the colours vary so that the averages are not trivial"""
    h = 1.0 / k
    rec = np.zeros((k * k, 24), F)
    iy, ix = np.divmod(np.arange(k * k), k)
    rec[:, 0], rec[:, 1], rec[:, 3] = (ix + 0.5) * h, (iy + 0.5) * h, 1
    rec[:, 4], rec[:, 5], rec[:, 6], rec[:, 7] = ix / k, iy / k, 0.5, 1
    rec[:, 8], rec[:, 9], rec[:, 10] = h, h, 1e-7
    rec[:, 14] = 1
    rec[:, 16] = 1
    rec[:, 20:24] = (0.1, 0.5, 0, 1)
    return rec
