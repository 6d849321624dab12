"""numpy restatement of the cut that fits a record budget (m2s_lod_select_budget; the pin is in include/m2s.h), on top of tests/lod_ref.py:
the threshold key of every node by a bisection that calls lod_ref.refine, the interval [L, H) of keys on which a node is selected, the
count of a key, and the search, done plainly over the sorted distinct keys at which the count can change.  A key is the bits of a
non-negative finite float32.  Integer logic and the float32 arithmetic of lod_ref.refine: the device is compared for equality."""
import numpy as np

import lod_ref as lr

F = np.float32
KEY_MAX = 0x7F7FFFFF
NEVER = np.uint32(0xFFFFFFFF)


def tau_of(key):
    return np.array([key], np.uint32).view(F)[0]


def key_of(tau):
    tau = F(tau)
    return int(np.array([tau], F).view(np.uint32)[0]) if tau > 0 else 0


def thresholds(b, camera_position, focal_px, near):
    """T per node: the smallest key at which the pinned comparison is false.  It is true below T and false from T on, so T >= c exactly
    when key c - 1 refines: T is built from its top bit down, 31 calls of lod_ref.refine with a tau per node."""
    b = np.asarray(b, F).reshape(-1, 4)
    T = np.zeros(len(b), np.uint32)
    for bit in range(30, -1, -1):
        c = T | np.uint32(1 << bit)
        r = lr.refine(b, camera_position, focal_px, (c - np.uint32(1)).view(F), near)
        T = np.where(r, c, T)
    return T


def intervals(b, parent, first, camera_position, focal_px, near):
    """-> (L, H, T) per node, uint32: the node is selected at key k iff L <= k < H"""
    parent = np.asarray(parent, np.uint32)
    levels = len(first) - 1
    T = thresholds(b, camera_position, focal_px, near)
    H = np.full(first[-1], NEVER, np.uint32)
    for l in range(levels - 2, -1, -1):
        p = parent[first[l]:first[l + 1]]
        H[first[l]:first[l + 1]] = np.minimum(H[p], T[p])
    L = T.copy()
    L[:first[1]] = 0
    return L, H, T


def flags_at(L, H, key):
    return (L <= np.uint32(key)) & (np.uint32(key) < H)


def count(L, H, key):
    ok = L < H
    return int(np.count_nonzero(ok & (L <= np.uint32(key)))) - int(np.count_nonzero(ok & (H <= np.uint32(key))))


def endpoints(L, H):
    """the sorted distinct keys at which the count can change, 0 among them"""
    ok = L < H
    keys = np.unique(np.concatenate([[0], L[ok].astype(np.int64), H[ok].astype(np.int64)]))
    return [int(k) for k in keys if k <= KEY_MAX]


def search(L, H, first, max_records, tau_min_px=0.0):
    """-> {"key", "tau_px" (float32), "met", "selected", "selected_finer", "by_floor", "n_eff"}; an empty tree: the floor, met, 0"""
    assert max_records >= 1
    last = first[-1] - first[-2]
    n_eff = max(int(max_records), last)
    floor_key = key_of(tau_min_px)
    if first[-1] == 0:
        return {"key": floor_key, "tau_px": tau_of(floor_key), "met": True, "selected": 0, "selected_finer": 0, "by_floor": floor_key > 0, "n_eff": n_eff}
    ok = L < H
    keys, lo, hi = np.array(endpoints(L, H), np.int64), np.sort(L[ok].astype(np.int64)), np.sort(H[ok].astype(np.int64))
    counts = np.searchsorted(lo, keys, "right") - np.searchsorted(hi, keys, "right")     # count(key) at every endpoint, in ascending order
    key = int(keys[np.flatnonzero(counts <= n_eff)[0]])
    assert count(L, H, key) == int(counts[np.flatnonzero(counts <= n_eff)[0]])
    by_floor = floor_key > key
    key = max(key, floor_key)
    selected = count(L, H, key)
    finer = selected if key == 0 or by_floor else count(L, H, key - 1)
    return {"key": key, "tau_px": tau_of(key), "met": selected <= max_records, "selected": selected, "selected_finer": finer, "by_floor": by_floor,
            "n_eff": n_eff}


def budgets(L, H, first):
    """the budgets every tree is asked for: around the last level, a middle value, around the leaves' cut, every node"""
    last, c0 = first[-1] - first[-2], count(L, H, 0)
    vals = [1, last - 1, last, last + 1, (last + c0) // 2, c0 - 1, c0, first[-1]]
    return sorted({v for v in vals if v >= 1})
