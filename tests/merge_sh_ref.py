"""Pin 5s of include/m2s.h ("merge pass") restated in numpy: the baked SH plane merged with its records (m2s_set_carry_sh), the planes of
the level-of-detail tree (pin 4s) and of its cuts (pin 3s).  Order, runs and segments are tests/merge_ref.py's (merge_unsigned_ref's with
M2S_MERGE_UNSIGNED_AXIS), used as they are: the plane is never read by the heads.

The pin.  A segment of one member: its 48 floats copied bit for bit (every invalid record is such a segment).  A segment of members
i = 1..m >= 2 in sorted order, every product and sum float64 from the stored floats, in member order:
    w_i = sx_i sy_i, W = sum w_i;  where W == 0: w_i = 1 for every member, W = m (merge_ref.parent's own test, the same value);
    a_i = w_i alpha_i, A = sum a_i;
    sh'_k = float32(sum a_i sh_ik / A) where A != 0, else float32(sum w_i sh_ik / W), for each of the 48 columns — the selector
    merge_ref.parent applies to rgb; one rounding to float32 per coefficient.
The 3DGS colour 0.5 + sum_k sh_k B_k(dir) is linear in the coefficients, so the parent's colour in every direction is that same weighted
mean of its members' colours in that direction (tests/test_merge_sh_ref.py checks it with mesh2splat_amd.bake's basis).

Vectorised over the segments: the sums run over the member RANK (at most 64 passes, each adding the k-th member of every segment that
has one), which is member order exactly — np.add.reduceat would add the same terms pairwise — so that 300 003 records cost seconds.

The bar of the device tests, derived, not measured: a singleton's row is bit-identical; otherwise |got - want| <= 1 fp32 ulp of
max_i |sh_ik| over the segment's members.  The weights are non-negative for valid records, so the mean is a convex combination, bounded
by that maximum: the final rounding gives 1/2 ulp of it at most, the fp64 sums (m + 3) 2^-53 relative to it — 1e-7 ulp for m = 64, in
any order of the additions, with or without contraction.  A coefficient whose restated value is not finite must be non-finite of the same
class on the device (NaN where NaN, the same infinity where infinite), as merge_ref.compare asks of the records."""
import numpy as np

import lod_ref as lr
import merge_ref as mr
import merge_unsigned_ref as mu

F = np.float32
SH_FLOATS = 48
PLANE_ULPS_BAR = 1.0
# measured on MI355X over the cases of tests/test_gpu_merge_sh.py: the largest |got - want| in fp32 ulps of max_i |sh_ik|.
# Zero: the kernel and the rank-ordered sums above add the same fp64 products in the same order and round once, so every coefficient
# of every case came out bit-identical.  Recorded, not asserted: the bar is the derived one.
PLANE_ULPS_ACHIEVED = 0.0


def _segment_sums(v, heads, members):
    """v: (n, ...) float64 in SORTED order -> (S, ...): per segment the sum of its members' entries, added in member order"""
    out = np.zeros((len(heads),) + v.shape[1:], np.float64)
    for k in range(int(members.max()) if len(members) else 0):
        sel = members > k
        out[sel] += v[heads[sel] + k]
    return out


def merge_plane(rec, sh, perm, heads):
    """pin 5s for the segments `heads` over the order `perm` (merge_ref.segment_heads or merge_unsigned_ref.segment_heads)
    -> (plane (S, 48) float32, info {"members" (S,), "unit": W == 0 (S,) bool, "by_area": A == 0 (S,) bool — both False for singletons,
    "exact": the (S, 48) float64 values before the one rounding (a singleton's: its floats), "mag": max_i |sh_ik| (S, 48) float64})"""
    rec = np.ascontiguousarray(rec, F).reshape(-1, 24)
    sh = np.ascontiguousarray(sh, F).reshape(-1, SH_FLOATS)
    n, S = len(rec), len(heads)
    assert len(sh) == n and len(perm) == n
    heads = np.asarray(heads, np.int64)
    members = np.append(heads[1:], n) - heads if S else np.zeros(0, np.int64)
    seg_of = np.repeat(np.arange(S), members)
    r = rec[perm].astype(np.float64)
    shs = sh[perm].astype(np.float64)
    multi = members >= 2
    with np.errstate(all="ignore"):
        w = r[:, 8] * r[:, 9]
        unit = multi & (_segment_sums(w, heads, members) == 0)
        w = np.where(unit[seg_of], 1.0, w)
        W = _segment_sums(w, heads, members)
        a = w * r[:, 7]
        A = _segment_sums(a, heads, members)
        by_alpha = A != 0
        num = np.where(by_alpha[:, None], _segment_sums(a[:, None] * shs, heads, members), _segment_sums(w[:, None] * shs, heads, members))
        exact = num / np.where(by_alpha, A, W)[:, None]
        out = exact.astype(F)
    single = ~multi
    out[single] = sh[perm[heads[single]]]                       # bit for bit (a NaN's payload included: no arithmetic touches them)
    exact[single] = shs[heads[single]]
    mag = np.zeros((S, SH_FLOATS))
    if n:
        mag = np.maximum.reduceat(np.abs(np.nan_to_num(shs, nan=0.0, posinf=0.0, neginf=0.0)), heads, axis=0)
    return out, {"members": members, "unit": unit, "by_area": multi & ~by_alpha, "exact": exact, "mag": mag}


def heads_of(rec, level, max_group=4, min_axis_dot=0.5, unsigned_axis=False):
    return (mu if unsigned_axis else mr).segment_heads(rec, level, max_group, min_axis_dot)


def merge(rec, sh, level, max_group=4, min_axis_dot=0.5, unsigned_axis=False):
    """the merge with the switch on -> (records after, map, counts, info: merge_ref.merge's four, plane after (S, 48) float32, plane info)"""
    out, mp, counts, info = (mu if unsigned_axis else mr).merge(rec, level, max_group, min_axis_dot)
    perm, heads = heads_of(rec, level, max_group, min_axis_dot, unsigned_axis)
    plane, pinfo = merge_plane(rec, sh, perm, heads)
    assert len(plane) == counts["after"]
    return out, mp, counts, info, plane, pinfo


def chain(rec, sh, levels, max_group=4, min_axis_dot=0.5, unsigned_axis=False):
    """pin 4s: the merges one after the other as m2s_lod_build runs them (a step that merges nothing adds no level and no rows)
    -> (the levels' records, the levels' planes, parent, first); np.concatenate(planes) is the tree's plane"""
    recs, planes, maps = [np.ascontiguousarray(rec, F).reshape(-1, 24)], [np.ascontiguousarray(sh, F).reshape(-1, SH_FLOATS)], []
    for lv in levels:
        nxt, m, counts, _, plane, _ = merge(recs[-1], planes[-1], lv, max_group, min_axis_dot, unsigned_axis)
        if counts["after"] == len(recs[-1]):
            continue
        recs.append(nxt)
        planes.append(plane)
        maps.append(m)
    parent, first = lr.link(maps, [len(v) for v in recs])
    return recs, planes, parent, first


def cut_plane(tree_plane, nodes):
    """pin 3s: the rows of the selected nodes, in node-index order"""
    return np.ascontiguousarray(tree_plane, F).reshape(-1, SH_FLOATS)[np.asarray(nodes, np.int64)]


def compare(got, want, pinfo):
    """the device's plane against merge_plane's -> the largest |got - want| in fp32 ulps of max_i |sh_ik| over the coefficients whose
    restated value is finite; singletons bit-identical and non-finite classes equal (asserted)"""
    got = np.ascontiguousarray(got, F).reshape(-1, SH_FLOATS)
    assert got.shape == want.shape, (got.shape, want.shape)
    single = pinfo["members"] == 1
    assert np.array_equal(got[single].view(np.uint32), want[single].view(np.uint32)), "a singleton's row is not a copy"
    g, w = got[~single].astype(np.float64), want[~single].astype(np.float64)
    fin = np.isfinite(w)
    assert np.array_equal(np.isnan(g), np.isnan(w)), "NaN where the restatement has none, or the reverse"
    assert np.array_equal(g[np.isinf(w)], w[np.isinf(w)]) and not np.isinf(g[fin]).any(), "infinities differ"
    mag = pinfo["mag"][~single]
    with np.errstate(all="ignore"):
        err = np.abs(np.where(fin, g - w, 0.0))
    zero = fin & (mag == 0)
    assert (err[zero] == 0).all(), "a column of zeros did not stay zero"
    sel = fin & (mag > 0)
    if not sel.any():
        return 0.0
    with np.errstate(all="ignore"):
        return float((err[sel] / np.spacing(mag[sel].astype(F)).astype(np.float64)).max())


def random_plane(n, seed, nonfinite=False, valid=None):
    """(n, 48) float32: normal values of both signs, magnitudes log-uniform over 1e-3 .. 1e3.  nonfinite: one inf and one NaN, in rows of
    valid records (`valid`: their mask) that are not the first two such rows"""
    rng = np.random.default_rng(4000 + seed)
    sh = (np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n, SH_FLOATS))) * rng.choice([-1.0, 1.0], (n, SH_FLOATS))).astype(F)
    if nonfinite:
        ok = np.flatnonzero(valid if valid is not None else np.ones(n, bool))
        sh[ok[len(ok) // 3], 5] = np.inf
        sh[ok[(2 * len(ok)) // 3], 17] = np.nan
    return sh
