"""numpy restatement of the cuts over a view frustum (m2s_lod_select_frustum, m2s_lod_select_budget_frustum; the pin is in include/m2s.h),
on top of tests/lod_ref.py and tests/lod_budget_ref.py: the prepass's frustum test per leaf with a guard band, the visibility of every
node (a leaf below it is inside), the masked cut, the masked intervals (L := H for an invisible node) and the search over them.
Integer logic and float32 arithmetic with one rounding per operation: the device is compared for equality."""
import numpy as np

import lod_budget_ref as br
import lod_ref as lr

F = np.float32


def _m4_mul(m, x, y, z, w):
    """mat4 * vec4 in glm's association; m: 16 float32 scalars, column-major"""
    return [(m[0 + i] * x + m[4 + i] * y) + (m[8 + i] * z + m[12 + i] * w) for i in range(4)]


def inside(b, model_to_world, world_to_view, view_to_clip, guard_band=1.05):
    """pin 1 per bound (for every node handed in, not just leaves): bool per row"""
    b = np.asarray(b, F).reshape(-1, 4)
    M, V, P = ([F(v) for v in np.asarray(m, F).reshape(16)] for m in (model_to_world, world_to_view, view_to_clip))
    one = F(1.0)
    with np.errstate(all="ignore"):
        ws = _m4_mul(M, b[:, 0], b[:, 1], b[:, 2], one)
        vs = _m4_mul(V, ws[0], ws[1], ws[2], one)
        c = _m4_mul(P, vs[0], vs[1], vs[2], vs[3])
        clip = F(guard_band) * c[3]
        assert clip.dtype == F
        return ~((c[2] < -clip) | (c[0] < -clip) | (c[0] > clip) | (c[1] < -clip) | (c[1] > clip))


def visibility(b, parent, first, frustum):
    """pin 2.  frustum: (model_to_world, world_to_view, view_to_clip, guard_band).  -> bool per node"""
    parent = np.asarray(parent, np.uint32)
    vis = np.zeros(first[-1], bool)
    vis[:first[1]] = inside(np.asarray(b, F).reshape(-1, 4)[:first[1]], *frustum)
    for l in range(len(first) - 2):
        sl = slice(first[l], first[l + 1])
        np.logical_or.at(vis, parent[sl][vis[sl]], True)
    return vis


def select(b, parent, first, camera_position, focal_px, tau_px, near, frustum, vis=None):
    """pin 3: lod_ref.select's dict with the flags, nodes, per_level and the selected counts masked, "refine" as it was, and
    "vis", "plain" (the unmasked flags), "visible_leaves", "culled" beside them.  vis: visibility() of this frustum, where the caller has it"""
    sel = lr.select(b, parent, first, camera_position, focal_px, tau_px, near)
    if vis is None:
        vis = visibility(b, parent, first, frustum)
    flags = sel["flags"] & vis
    per_level = [int(flags[first[l]:first[l + 1]].sum()) for l in range(len(first) - 1)]
    counts = dict(sel["counts"], selected=int(flags.sum()), selected_leaves=per_level[0])
    return {"flags": flags, "refine": sel["refine"], "open": sel["open"], "nodes": np.flatnonzero(flags).astype(np.uint32), "per_level": per_level,
            "counts": counts, "vis": vis, "plain": sel["flags"], "visible_leaves": int(vis[:first[1]].sum()),
            "culled": int(sel["flags"].sum()) - int(flags.sum())}


def cut_ok(parent, first, flags, vis):
    """every inside leaf has exactly one selected ancestor-or-self, and every selected node has an inside leaf below it (is visible)"""
    parent = np.asarray(parent, np.uint32).astype(np.int64)
    flags, vis = np.asarray(flags, bool), np.asarray(vis, bool)
    hits = np.zeros(first[1], np.int64)
    cur = np.arange(first[1], dtype=np.int64)
    alive = np.ones(first[1], bool)
    for _ in range(len(first) - 1):
        hits[alive] += flags[cur[alive]]
        nxt = parent[cur[alive]]
        cur[alive] = nxt
        alive[alive] = nxt != int(lr.NO_PARENT)
    return not alive.any() and bool((hits[vis[:first[1]]] == 1).all()) and not bool((flags & ~vis).any())


def intervals(b, parent, first, camera_position, focal_px, near, frustum):
    """pin 5: lod_budget_ref.intervals with L := H where the node is not visible.  -> (L, H, T, vis)"""
    L, H, T = br.intervals(b, parent, first, camera_position, focal_px, near)
    vis = visibility(b, parent, first, frustum)
    return np.where(vis, L, H), H, T, vis


def search(L, H, first, vis, max_records, tau_min_px=0.0):
    """lod_budget_ref.search over masked intervals, with N_eff = max(max_records, visible nodes of the last level)"""
    assert max_records >= 1
    last_vis = int(np.count_nonzero(vis[first[-2]:]))
    n_eff = max(int(max_records), last_vis)
    floor_key = br.key_of(tau_min_px)
    key = 0
    if first[-1]:
        ok = L < H
        keys, lo, hi = np.array(br.endpoints(L, H), np.int64), np.sort(L[ok].astype(np.int64)), np.sort(H[ok].astype(np.int64))
        counts = np.searchsorted(lo, keys, "right") - np.searchsorted(hi, keys, "right")  # count(key) at every endpoint, in ascending order
        key = int(keys[np.flatnonzero(counts <= n_eff)[0]])
    by_floor = floor_key > key
    key = max(key, floor_key)
    selected = br.count(L, H, key) if first[-1] else 0
    finer = selected if key == 0 or by_floor else br.count(L, H, key - 1)
    return {"key": key, "tau_px": br.tau_of(key), "met": selected <= max_records, "selected": selected, "selected_finer": finer, "by_floor": by_floor,
            "n_eff": n_eff}


def budgets(L, H, first, vis):
    """as lod_budget_ref.budgets, around the visible part of the last level and the masked cut at key 0"""
    last, last_vis, c0 = first[-1] - first[-2], int(np.count_nonzero(vis[first[-2]:])), br.count(L, H, 0)
    vals = [1, last_vis - 1, last_vis, last_vis + 1, last, (last_vis + c0) // 2, c0 - 1, c0, first[-1]]
    return sorted({v for v in vals if v >= 1})


def own_position_flags(b, parent, first, camera_position, focal_px, tau_px, near, frustum):
    """the rule the pin does NOT use: the plain cut masked by every selected node's own frustum test"""
    return lr.select(b, parent, first, camera_position, focal_px, tau_px, near)["flags"] & inside(b, *frustum)
