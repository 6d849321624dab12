"""numpy restatement of the level-of-detail tree's links and bounds and of its per-camera cut (m2s_lod_build, m2s_lod_select; the pins
are in include/m2s.h).  The merges themselves are tests/merge_ref.py's business.  Everything here is integer logic and float32
arithmetic with one rounding per operation (numpy's float32 array operations do not contract), so the device is compared for equality."""
import numpy as np

F = np.float32
NO_PARENT = np.uint32(0xFFFFFFFF)


def link(maps, counts):
    """maps[l]: the merge map from tree level l to level l + 1 (a uint32 per node of level l: its parent's index within level l + 1);
    counts[l]: the nodes of level l = 0 .. len(maps).  -> (parent (nodes,) uint32, first: list of len(counts) + 1)"""
    assert len(counts) == len(maps) + 1
    first = [0]
    for c in counts:
        first.append(first[-1] + int(c))
    parent = np.full(first[-1], NO_PARENT, np.uint32)
    for l, m in enumerate(maps):
        m = np.asarray(m, np.uint32)
        assert len(m) == counts[l] and (len(m) == 0 or int(m.max()) < counts[l + 1])
        parent[first[l]:first[l + 1]] = np.uint32(first[l + 1]) + m
    return parent, first


def bounds(rec):
    """(x, y, z, e) per record: its position and e = fmaxf(|scale[0]|, |scale[1]|), fmaxf returning its other operand for a NaN"""
    rec = np.ascontiguousarray(rec, F).reshape(-1, 24)
    out = np.empty((len(rec), 4), F)
    out[:, 0:3] = rec[:, 0:3]
    out[:, 3] = np.fmax(np.abs(rec[:, 8]), np.abs(rec[:, 9]))
    return out


def refine(b, camera_position, focal_px, tau_px, near):
    """the pinned comparison per bound"""
    b = np.asarray(b, F).reshape(-1, 4)
    c = [F(v) for v in camera_position]
    with np.errstate(all="ignore"):
        dx, dy, dz = b[:, 0] - c[0], b[:, 1] - c[1], b[:, 2] - c[2]
        d2 = np.fmax((dx * dx + dy * dy) + dz * dz, F(near) * F(near))
        s = b[:, 3] * F(focal_px)
        out = s * s > (F(tau_px) * F(tau_px)) * d2
    assert d2.dtype == F and s.dtype == F
    return out


def select(b, parent, first, camera_position, focal_px, tau_px=1.0, near=1e-3):
    """-> {"flags": selected per node (bool), "refine": per node, "open": per node (every ancestor-or-self refines), "nodes": the selected
    node indices in order, "per_level", "counts": m2s_lod_select's out_counts by name}"""
    parent = np.asarray(parent, np.uint32)
    n, levels = first[-1], len(first) - 1
    ref = refine(b, camera_position, focal_px, tau_px, near)
    opened, flags = np.zeros(n, bool), np.zeros(n, bool)
    for l in range(levels - 1, -1, -1):
        sl = slice(first[l], first[l + 1])
        above = np.ones(first[l + 1] - first[l], bool) if l == levels - 1 else opened[parent[sl]]
        flags[sl] = above & (~ref[sl] if l else np.ones_like(above))
        opened[sl] = above & ref[sl]
    per_level = [int(flags[first[l]:first[l + 1]].sum()) for l in range(levels)]
    counts = {"nodes": int(n), "selected": int(flags.sum()), "selected_leaves": per_level[0], "refine": int(ref.sum())}
    return {"flags": flags, "refine": ref, "open": opened, "nodes": np.flatnonzero(flags).astype(np.uint32), "per_level": per_level, "counts": counts}


def cut_ok(parent, first, selected):
    """every leaf has exactly one selected ancestor-or-self"""
    parent = np.asarray(parent, np.uint32).astype(np.int64)
    selected = np.asarray(selected, bool)
    cur = np.arange(first[1], dtype=np.int64)
    hits = np.zeros(first[1], np.int64)
    alive = np.ones(first[1], bool)
    for _ in range(len(first) - 1):
        hits[alive] += selected[cur[alive]]
        nxt = parent[cur[alive]]
        cur[alive] = nxt
        alive[alive] = nxt != int(NO_PARENT)
    return not alive.any() and bool((hits == 1).all())


def gated(parent, first, sel):
    """nodes that are fine enough themselves (a leaf, or not refining) but sit below an ancestor that does not refine: not selected"""
    ok = ~sel["refine"]
    ok[:first[1]] = True
    return np.flatnonzero(ok & ~sel["flags"])
