"""numpy restatement of the cuts behind an occluder (m2s_lod_select_occluded, m2s_lod_select_budget_occluded; the pin is in
include/m2s.h), on top of tests/lod_frustum_ref.py: a leaf is inside iff it passes the frustum test and is not behind a depth image
under the prepass's own depth test.  Everything above the leaf test is the frustum restatement's with this `inside`: the visibility of
every node, the masked cut, the masked intervals and the search.  float32 arithmetic with one rounding per operation and integer
logic: the device is compared for equality."""
import numpy as np

import lod_budget_ref as br
import lod_frustum_ref as fr
import lod_ref as lr

F = np.float32
BIAS = 2e-5                                                  # the prepass's own (0.00002f)


def clip(b, model_to_world, world_to_view, view_to_clip):
    """the clip-space position of pin 1 of the frustum cuts per bound: four float32 arrays"""
    b = np.asarray(b, F).reshape(-1, 4)
    M, V, P = ([F(v) for v in np.asarray(m, F).reshape(16)] for m in (model_to_world, world_to_view, view_to_clip))
    one = F(1.0)
    with np.errstate(all="ignore"):
        ws = fr._m4_mul(M, b[:, 0], b[:, 1], b[:, 2], one)
        vs = fr._m4_mul(V, ws[0], ws[1], ws[2], one)
        return fr._m4_mul(P, vs[0], vs[1], vs[2], vs[3])


def _texel(t, size):
    """the prepass's clamp of floorf(u * size): below 0 and NaN give 0, at or above the size gives size - 1"""
    with np.errstate(all="ignore"):
        ok = (t >= 0) & (t < F(size))
        inner = np.where(ok, t, F(0)).astype(np.int64)
    return np.where(t >= 0, np.where(t < F(size), inner, size - 1), 0).astype(np.int64)


def leaf_test(b, alpha, frustum, depth, bias=BIAS):
    """pin 1 per bound.  frustum: (model_to_world, world_to_view, view_to_clip, guard_band); depth: (H, W) float32, row 0 = bottom.
    -> dict of arrays: "in_frustum", "my" (the leaf's window-space depth), "ti", "tj", "d" (its texel), "behind", "occluded",
    "kept" (behind, inside the frustum and not occluded), "inside", "clamped" (a texel index was clamped), "tie" (my == d + bias).  behind / occluded / kept are False outside the frustum."""
    depth = np.ascontiguousarray(depth, F)
    assert depth.ndim == 2 and depth.size
    H, W = depth.shape
    alpha = np.asarray(alpha, F).reshape(-1)
    c = clip(b, *frustum[:3])
    in_fr = fr.inside(b, *frustum)
    half = F(0.5)
    with np.errstate(all="ignore"):
        u = (c[0] / c[3]) * half + half
        v = (c[1] / c[3]) * half + half
        fu, fv = np.floor(u * F(W)), np.floor(v * F(H))
        ti, tj = _texel(fu, W), _texel(fv, H)
        clamped = in_fr & ((fu < 0) | (fu >= F(W)) | (fv < 0) | (fv >= F(H)))
        d = depth[tj, ti]
        my = (c[2] / c[3]) * half + half
        assert u.dtype == F and my.dtype == F and d.dtype == F
        behind = in_fr & (my > d + F(bias))
        occluded = behind & (alpha > F(.95))
    return {"in_frustum": in_fr, "my": my, "ti": ti, "tj": tj, "d": d, "behind": behind, "occluded": occluded, "kept": behind & ~occluded,
            "inside": in_fr & ~occluded, "clamped": clamped, "tie": in_fr & (my == d + F(bias))}


def inside(b, alpha, frustum, depth, bias=BIAS):
    """pin 1: bool per row"""
    return leaf_test(b, alpha, frustum, depth, bias)["inside"]


def visibility(b, alpha, parent, first, frustum, depth, bias=BIAS):
    """pin 2 of the frustum cuts with this inside.  alpha: color[3] of the leaves' node records (at least first[1] of them)"""
    parent = np.asarray(parent, np.uint32)
    n0 = first[1]
    vis = np.zeros(first[-1], bool)
    vis[:n0] = inside(np.asarray(b, F).reshape(-1, 4)[:n0], np.asarray(alpha, F).reshape(-1)[:n0], frustum, depth, bias)
    for l in range(len(first) - 2):
        sl = slice(first[l], first[l + 1])
        np.logical_or.at(vis, parent[sl][vis[sl]], True)
    return vis


def counts(b, alpha, first, frustum, depth, bias=BIAS):
    """pin 3, [0..2]: leaves inside the frustum, of those occluded, of those behind the image and kept"""
    n0 = first[1]
    t = leaf_test(np.asarray(b, F).reshape(-1, 4)[:n0], np.asarray(alpha, F).reshape(-1)[:n0], frustum, depth, bias)
    return {"visible_leaves": int(t["in_frustum"].sum()), "occluded_leaves": int(t["occluded"].sum()), "translucent_kept": int(t["kept"].sum())}


def select(b, alpha, parent, first, camera_position, focal_px, tau_px, near, frustum, depth, bias=BIAS, vis=None):
    """lod_frustum_ref.select over this visibility, with pin 3's counts: "visible_leaves" is the leaves inside the FRUSTUM, and
    "occluded_leaves", "translucent_kept" stand beside it"""
    if vis is None:
        vis = visibility(b, alpha, parent, first, frustum, depth, bias)
    sel = fr.select(b, parent, first, camera_position, focal_px, tau_px, near, frustum, vis)
    sel.update(counts(b, alpha, first, frustum, depth, bias))
    return sel


def intervals(b, alpha, parent, first, camera_position, focal_px, near, frustum, depth, bias=BIAS):
    """pin 5 of the frustum cuts: L := H where the node is not visible.  -> (L, H, T, vis)"""
    L, H, T = br.intervals(b, parent, first, camera_position, focal_px, near)
    vis = visibility(b, alpha, parent, first, frustum, depth, bias)
    return np.where(vis, L, H), H, T, vis


search = fr.search                                           # (L, H, first, vis, max_records, tau_min_px): it takes the vis it is given
budgets = fr.budgets
cut_ok = fr.cut_ok


def median_depth_image(b, alpha, first, frustum, W=64, H=36, bias=BIAS, rng=None):
    """A synthetic (H, W) depth image for one camera, from the restatement's own values: every texel takes the median `my` of the leaves
    inside the frustum that fall in it (so about half of them are behind it), 1.0 where none falls.  With rng: sprinkled with texels
    of 1.0, 0.0 and NaN, and texels set to exactly fl(my - bias) of one of their leaves where adding the bias back gives my (a tie:
    equality does not occlude)."""
    n0 = first[1]
    img = np.ones((H, W), F)
    t = leaf_test(np.asarray(b, F).reshape(-1, 4)[:n0], np.asarray(alpha, F).reshape(-1)[:n0], frustum, img, bias)
    ok = t["in_frustum"] & np.isfinite(t["my"])
    cell = t["tj"] * W + t["ti"]
    idx = np.flatnonzero(ok)
    if len(idx):
        order = idx[np.lexsort((t["my"][idx], cell[idx]))]                           # by texel, then by depth
        cs = cell[order]
        starts = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
        ends = np.r_[starts[1:], len(cs)]
        img.reshape(-1)[cs[starts]] = t["my"][order[starts + (ends - starts - 1) // 2]]
    if rng is not None:
        flat = img.reshape(-1)
        pick = rng.permutation(H * W)
        flat[pick[0:40]], flat[pick[40:80]], flat[pick[80:120]] = F(1.0), F(0.0), F(np.nan)
        leaves = np.flatnonzero(ok)
        for j in leaves[rng.permutation(len(leaves))[:max(1, len(leaves) // 8)]]:
            d = F(t["my"][j] - F(bias))
            if F(d + F(bias)) == t["my"][j]:
                flat[cell[j]] = d
    return img


def own_position_flags(b, alpha, parent, first, camera_position, focal_px, tau_px, near, frustum, depth, bias=BIAS):
    """the rule the pin does NOT use: the plain cut masked by every selected node's own frustum and depth test (what m2s_prepass with
    depth_test_mesh = 1 does to a cut)"""
    return lr.select(b, parent, first, camera_position, focal_px, tau_px, near)["flags"] & inside(b, alpha, frustum, depth, bias)
