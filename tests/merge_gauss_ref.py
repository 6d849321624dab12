"""The merge pass under M2S_MERGE_MODEL_GAUSSIAN (m2s_set_merge_model; include/m2s.h pins 2g, 5g, 5sg, 4g) restated in numpy.  Order,
segments (pin 3), copies (pin 4), output order, map and counts are tests/merge_ref.py's, used as they are; what is restated here is the
axis of the run rule (the row of the smallest scale, sign-free), the parent (the full 3 x 3 moment of three-axis Gaussians and its
eigenpairs by the header's cyclic Jacobi iteration, operation for operation in float64), the SH weights and the tree bound.

Bars, carried over from merge_ref: segmentation, counts, map and the bytes of copied records are exact.  A parent's scalar fields
(position.xyz, colour.rgb, alpha, the three scales, normal.xyz, pbr[0..1]) lie within 4 fp32 ulps of the field's magnitude.  Scale and
rotation together are compared through the covariance they draw, sigma^2 sum_k s_k^2 r_k r_k^T of the stored parent in float64,
against the restatement's M, elementwise within 1e-5 l1 (l1 the largest eigenvalue): the fp32 rounding of seven stored numbers
perturbs it by about 1e-6.  (The eigenvectors themselves are not compared: where two eigenvalues agree they are any basis of a plane.)

ACHIEVED (the project's convention: what the MI355X measured over every case of tests/test_gpu_merge_gauss.py against THIS restatement,
and a guard at 4 x it beside the bar): SCALAR_ULPS_ACHIEVED / COV_REL_ACHIEVED below and DESIGN 5.26."""
import math

import numpy as np

import compact_ref as cr
import lod_ref as lr
import merge_ref as mr
import merge_sh_ref as ms

F = np.float32
FOOTPRINT, GAUSSIAN = 0, 1
SCALAR_ULPS_BAR = mr.SCALAR_ULPS_BAR
COV_REL_BAR = mr.COV_REL_BAR
# measured on MI355X over the cases of tests/test_gpu_merge_gauss.py: the largest error of a scalar field in fp32 ulps of the field's
# magnitude, and of a covariance element relative to l1.  Every scalar field of every case came out bit-identical: the kernel and
# parent() above add the same fp64 products in the same order and round once.  Four times nothing is no guard, so the scalars' guard
# is one differing fp32 rounding of one component, 1 ulp of the field's magnitude at most; the covariance's is the usual 4 x.
SCALAR_ULPS_ACHIEVED = 0.0
COV_REL_ACHIEVED = 3.05e-7
SCALAR_ULPS_GUARD = 1.0
COV_REL_GUARD = 4 * COV_REL_ACHIEVED
JACOBI_SWEEPS = 16


def rows_f32(q):
    """r_1, r_2, r_3 of castQuatToMat3 in fp32, one rounding per operation; q: (n, 4) -> (n, 3, 3) [record, row, component]"""
    q = np.ascontiguousarray(q, F).reshape(-1, 4)
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = F(1), F(2)
    with np.errstate(all="ignore"):
        r1 = np.stack([one - two * (z * z + w * w), two * (y * z + x * w), two * (y * w - x * z)], 1)
        r2 = np.stack([two * (y * z - x * w), one - two * (y * y + w * w), two * (z * w + x * y)], 1)
        r3 = np.stack([two * (y * w + x * z), two * (z * w - x * y), one - two * (y * y + z * z)], 1)
    return np.stack([r1, r2, r3], 1).astype(F)


def axis_index(scale):
    """pin 2g: the k of the smallest |scale[k]|, the lower k on a tie; scale: (n, 3+) -> (n,)"""
    s = np.abs(np.ascontiguousarray(scale, F).reshape(len(scale), -1)[:, 0:3])
    k = np.where(s[:, 1] < s[:, 0], 1, 0)
    return np.where(s[:, 2] < np.minimum(s[:, 0], s[:, 1]), 2, k)


def axes_f32(rec):
    """pin 2g: every record's axis, fp32 (n, 3)"""
    rec = np.ascontiguousarray(rec, F).reshape(-1, 24)
    return rows_f32(rec[:, 16:20])[np.arange(len(rec)), axis_index(rec[:, 8:11])]


def segment_heads(rec, level, max_group, min_axis_dot):
    """pins 1, 2g, 3 -> (perm, heads), as merge_ref.segment_heads"""
    rec = np.ascontiguousarray(rec, F).reshape(-1, 24)
    n = len(rec)
    perm, keys = mr.order(rec)
    if n == 0:
        return perm, np.zeros(0, np.int64)
    a = axes_f32(rec[perm])
    with np.errstate(all="ignore"):
        d = ((a[1:, 0] * a[:-1, 0]) + a[1:, 1] * a[:-1, 1]) + a[1:, 2] * a[:-1, 2]
        brk = ~(np.abs(d) >= F(min_axis_dot))
    inval = keys == mr.INVALID_KEY
    cell = keys >> np.uint32(3 * level)
    run = np.ones(n, bool)
    run[1:] = inval[1:] | inval[:-1] | (cell[1:] != cell[:-1]) | brk
    run_start = np.maximum.accumulate(np.where(run, np.arange(n), 0))
    return perm, np.flatnonzero((np.arange(n) - run_start) % max_group == 0)


def areas(scale):
    """pin 5g: the product of the two largest of |s1|, |s2|, |s3|, float64 (exact: two 24-bit significands); scale: (m, 3) float64"""
    a = np.abs(np.asarray(scale, np.float64).reshape(-1, 3))
    lo = np.minimum(np.minimum(a[:, 0], a[:, 1]), a[:, 2])
    return np.where(lo == a[:, 2], a[:, 0] * a[:, 1], np.where(lo == a[:, 1], a[:, 0] * a[:, 2], a[:, 1] * a[:, 2]))


def _seq(v):
    """the sum of v's rows, added one after the other in order (np.sum adds pairwise)"""
    return np.cumsum(v, axis=0)[-1]


def jacobi(m00, m01, m02, m11, m12, m22):
    """The header's cyclic Jacobi iteration on python floats (IEEE double, one rounding per operation) -> (the three diagonal elements,
    V as a list of rows [[v00, v01, v02], ...]: column k belongs to diagonal element k, the sweeps begun)"""
    A = [[m00, m01, m02], [m01, m11, m12], [m02, m12, m22]]       # only the upper triangle is read and written: A[p][q] with p < q
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    sweeps = 0

    def up(i, j):
        return (i, j) if i < j else (j, i)

    for _ in range(JACOBI_SWEEPS):
        if A[0][1] == 0.0 and A[0][2] == 0.0 and A[1][2] == 0.0:
            break
        sweeps += 1
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)             # (apq != 0: its double is not 0 either; an overflow is an infinity)
            t = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            A[p][p] = A[p][p] - t * apq
            A[q][q] = A[q][q] + t * apq
            A[p][q] = 0.0
            rp, rq = up(r, p), up(r, q)
            arp, arq = A[rp[0]][rp[1]], A[rq[0]][rq[1]]
            A[rp[0]][rp[1]] = c * arp - s * arq
            A[rq[0]][rq[1]] = s * arp + c * arq
            for k in range(3):
                x, y = V[k][p], V[k][q]
                V[k][p] = c * x - s * y
                V[k][q] = s * x + c * y
    return (A[0][0], A[1][1], A[2][2]), V, sweeps


def eigen_sorted(M):
    """pin 5g: eigenvalues clamped at 0 and sorted descending, the lower original index first on a tie -> (l (3,), E (3, 3): column k
    the eigenvector of l[k], as Jacobi left it — e3 = e1 x e2 is the caller's)"""
    diag, V, _ = jacobi(M[0][0], M[0][1], M[0][2], M[1][1], M[1][2], M[2][2])
    pairs = [[max(diag[k], 0.0), [V[0][k], V[1][k], V[2][k]]] for k in range(3)]
    for i, j in ((0, 1), (1, 2), (0, 1)):
        if pairs[j][0] > pairs[i][0]:
            pairs[i], pairs[j] = pairs[j], pairs[i]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]).T


def parent(members, sigma=1.0):
    """pin 5g: members (m >= 2, 24) float32 in sorted order -> (the parent's 24 floats, {"M": the moment (3, 3), "cov": the same (what
    sigma^2 sum s_k^2 r_k r_k^T of the stored parent is compared with), "l": the sorted eigenvalues, "l1", "E": their eigenvectors as
    columns (e3 = e1 x e2), "unit": the unit weights applied})"""
    r = np.asarray(members, np.float64)
    first32 = np.asarray(members, F)[0]
    sg = float(F(sigma))
    sg2 = sg * sg
    with np.errstate(all="ignore"):
        area = areas(r[:, 8:11])
        W = float(_seq(area))
        unit = W == 0.0
        w = np.ones(len(r)) if unit else area
        d = r[:, 0:3] - r[0, 0:3]
        if unit:
            W = float(len(r))
        mu = (1.0 / W) * _seq(w[:, None] * d)
        q = mr.rows_f64(r[:, 16:20])
        k = r[:, 8:11] * r[:, 8:11]
        e = d - mu
        M = np.zeros((3, 3))
        for a in range(3):
            for b in range(a, 3):
                c = (k[:, 0] * q[0][:, a] * q[0][:, b] + k[:, 1] * q[1][:, a] * q[1][:, b]) + k[:, 2] * q[2][:, a] * q[2][:, b]
                M[a, b] = M[b, a] = float(_seq(w * (sg2 * c + e[:, a] * e[:, b]))) / W
        l, E = eigen_sorted(M.tolist())
        e1, e2 = E[:, 0], E[:, 1]
        e3 = np.cross(e1, e2)
        sc = np.sqrt(l) / sg
        out = np.zeros(24, np.float64)
        out[0:3] = r[0, 0:3] + mu
        wa = w * r[:, 7]
        swa = float(_seq(wa))
        out[4:7] = (1.0 / swa) * _seq(wa[:, None] * r[:, 4:7]) if swa != 0 else (1.0 / W) * _seq(w[:, None] * r[:, 4:7])
        ap = sc[0] * sc[1]
        out[7] = min(1.0, (0.0 if unit else swa) / ap) if (ap > 0 and np.isfinite(ap)) else swa / W
        out[8:11] = sc
        ns = _seq(w[:, None] * r[:, 12:15])
        nl2 = (ns[0] * ns[0] + ns[1] * ns[1]) + ns[2] * ns[2]
        out[12:15] = ns * (1.0 / np.sqrt(nl2)) if (nl2 > 0 and np.isfinite(nl2)) else 0.0
        out[16:20] = mr.quat_cast_wxyz(e1, e2, e3)
        out[20:22] = _seq(w[:, None] * r[:, 20:22]) / W
        out = out.astype(F)
    for i in COPIED:
        out[i] = first32[i]                              # the first member's bits
    return out, {"M": M, "cov": M, "l": l, "l1": float(l[0]), "E": np.stack([e1, e2, e3], 1), "unit": unit}


FIELDS = {"position": slice(0, 3), "colour": slice(4, 7), "alpha": slice(7, 8), "scales": slice(8, 11), "normal": slice(12, 15), "pbr": slice(20, 22)}
COPIED = (3, 11, 15, 22, 23)


def merge(rec, level, max_group=4, min_axis_dot=0.5, sigma=1.0):
    """-> merge_ref.merge's four: (records after (S, 24) float32, map (n,) uint32, counts, info: per segment None or parent()'s second)"""
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
            out[s], i = parent(rec[idx], sigma)
            info.append(i)
    counts = {"before": n, "after": S, "merged": int(np.count_nonzero(ends - heads >= 2)), "invalid": int(n - np.count_nonzero(cr.valid_mask(rec)))}
    return out, mp, counts, info


def drawn_cov(rec, sigma):
    """sigma^2 sum_k s_k^2 r_k r_k^T of one record's stored floats, float64 (3, 3)"""
    sg = float(F(sigma))
    return sg * sg * mr.viewer_cov(rec)


def compare(got, want, info, sigma):
    """device records against the restatement's -> {"scalar_ulps", "cov_rel": the largest covariance element error / l1}; copied records
    and copied words must be bit-identical (asserted), as merge_ref.compare"""
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
            assert np.isfinite(w).all(), (name, s, w)       # (valid members: pin 5g has no non-finite result)
            mag = np.abs(w).max()
            err = np.abs(g - w).max()
            if mag == 0:
                assert err == 0, (name, s, g, w)
                continue
            worst_u = max(worst_u, err / float(np.spacing(F(mag))))
        dc = np.abs(drawn_cov(got[s], sigma) - i["cov"]).max()
        if i["l1"] == 0:
            assert dc == 0, ("covariance of a parent without extent", s)
        else:
            worst_c = max(worst_c, dc / i["l1"])
    return {"scalar_ulps": worst_u, "cov_rel": worst_c}


def merge_plane(rec, sh, perm, heads):
    """pin 5sg: merge_sh_ref.merge_plane with w_i = a_i -> (plane (S, 48) float32, info as merge_sh_ref's, for merge_sh_ref.compare)"""
    rec = np.ascontiguousarray(rec, F).reshape(-1, 24)
    sh = np.ascontiguousarray(sh, F).reshape(-1, ms.SH_FLOATS)
    n, S = len(rec), len(heads)
    heads = np.asarray(heads, np.int64)
    members = np.append(heads[1:], n) - heads if S else np.zeros(0, np.int64)
    seg_of = np.repeat(np.arange(S), members)
    r = rec[perm].astype(np.float64)
    shs = sh[perm].astype(np.float64)
    multi = members >= 2
    with np.errstate(all="ignore"):
        w = areas(r[:, 8:11])
        unit = multi & (ms._segment_sums(w, heads, members) == 0)
        w = np.where(unit[seg_of], 1.0, w)
        W = ms._segment_sums(w, heads, members)
        a = w * r[:, 7]
        A = ms._segment_sums(a, heads, members)
        by_alpha = A != 0
        num = np.where(by_alpha[:, None], ms._segment_sums(a[:, None] * shs, heads, members), ms._segment_sums(w[:, None] * shs, heads, members))
        exact = num / np.where(by_alpha, A, W)[:, None]
        out = exact.astype(F)
    single = ~multi
    out[single] = sh[perm[heads[single]]]
    exact[single] = shs[heads[single]]
    mag = np.zeros((S, ms.SH_FLOATS))
    if n:
        mag = np.maximum.reduceat(np.abs(np.nan_to_num(shs, nan=0.0, posinf=0.0, neginf=0.0)), heads, axis=0)
    return out, {"members": members, "unit": unit, "by_area": multi & ~by_alpha, "exact": exact, "mag": mag}


def bounds(rec, sigma=1.0):
    """pin 4g: (x, y, z, e) with e = sigma * fmaxf(fmaxf(|scale[0]|, |scale[1]|), |scale[2]|) in fp32, one rounding for the product"""
    rec = np.ascontiguousarray(rec, F).reshape(-1, 24)
    out = np.empty((len(rec), 4), F)
    out[:, 0:3] = rec[:, 0:3]
    with np.errstate(all="ignore"):
        out[:, 3] = F(sigma) * np.fmax(np.fmax(np.abs(rec[:, 8]), np.abs(rec[:, 9])), np.abs(rec[:, 10]))
    return out


def chain(rec, levels, max_group=4, min_axis_dot=0.5, sigma=1.0):
    """the tree of m2s_lod_build under the Gaussian model: a step that merges nothing adds no level -> (the levels' records, parent, first)"""
    recs, maps = [np.ascontiguousarray(rec, F).reshape(-1, 24)], []
    for lv in levels:
        nxt, m, counts, _ = merge(recs[-1], lv, max_group, min_axis_dot, sigma)
        if counts["after"] == len(recs[-1]):
            continue
        recs.append(nxt)
        maps.append(m)
    parent_, first = lr.link(maps, [len(v) for v in recs])
    return recs, parent_, first


def gauss_records(n, seed=0, invalid=True):
    """n records of a .ply of another origin for the tests: merge_ref.crafted_records' positions (clusters that share keys, cells and
    everything), colours and rotations (a third row along one of six fixed directions, a random turn about it: the first and second
    rows, which pin 2g also picks, point anywhere); three non-zero scales in random order, about one in six flat (s3 = 0), one in six isotropic, one in twelve with no extent
    at all; with `invalid` merge_ref's three invalid records (a NaN position, a zero quaternion, a negative scale)."""
    rec = mr.crafted_records(n, seed, invalid=False)
    rng = np.random.default_rng(7000 + seed)
    s = np.exp(rng.normal(-3, 1, (n, 3)))
    kind = rng.integers(0, 12, n)
    s[kind < 2, 2] = 0.0                                  # flat, the conversion's shape
    iso = (kind == 2) | (kind == 3)
    s[iso] = s[iso, 0:1]
    s[kind == 4] = 0.0
    order = np.argsort(rng.random((n, 3)), 1)
    keep_flat = kind < 2                                  # (a flat record keeps its zero on the third axis)
    s = np.where(keep_flat[:, None], s, np.take_along_axis(s, order, 1))
    rec[:, 8:11] = s
    if invalid:
        for k, (col, val) in enumerate(((0, np.nan), (16, 0.0), (8, -0.25))):
            if n > 8 * (k + 1):
                i = (n * (2 * k + 1)) // 7
                rec[i, col] = val
                if col == 16:
                    rec[i, 16:20] = 0
    return rec
