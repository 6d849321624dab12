"""numpy restatement of m2s_prune_budget (include/m2s.h): keys with np.float32 arithmetic, so the bits are the device's; candidates; the
threshold key T, the tie quota, the kept indices and the six counts of m2s_last_budget_counts — once as the pin words it (T, then the
first ties by index), once through a stable argsort (select_by_sort), which the first is checked against."""
import numpy as np

COUNTS = ("before", "candidates", "kept", "threshold_key", "ties_kept", "ties")


def _bits(p):
    """p > 0 ? bits(p) : 0 — a NaN and a zero of either sign give 0."""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore"):
        pos = p > np.float32(0)
    return np.where(pos, p.view(np.uint32), np.uint32(0)).astype(np.uint32)


def keys_views(wmax_bits, npix):
    """The bits of the fp32 product (float)npix * wmax: uint32 -> float32 rounds to nearest even once, the multiply rounds once."""
    w = np.ascontiguousarray(wmax_bits, np.uint32).view(np.float32)
    k = np.ascontiguousarray(npix, np.uint32).astype(np.float32)
    return _bits(k * w)


def candidates_views(wmax_bits, npix, min_weight, min_pixels):
    """m2s_prune's test: wmax > min_weight compared as floats, npix >= min_pixels."""
    w = np.ascontiguousarray(wmax_bits, np.uint32).view(np.float32)
    return (w > np.float32(min_weight)) & (np.ascontiguousarray(npix, np.uint32) >= np.uint32(min_pixels))


def keys_area(rec):
    """a = fminf(fmaxf(color[3], 0), 1), s = |scale[0]| * |scale[1]|, p = s * a (np.fmax / np.fmin return the other operand for a NaN, as
    fmaxf / fminf do)."""
    rec = np.asarray(rec, np.float32).reshape(-1, 24)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.fmin(np.fmax(rec[:, 7], np.float32(0)), np.float32(1)).astype(np.float32)
        s = (np.abs(rec[:, 8]) * np.abs(rec[:, 9])).astype(np.float32)
        p = (s * a).astype(np.float32)
    return _bits(p)


def select(keys, cand, max_records):
    """-> (kept indices ascending, the six counts by name).  The pin's wording: T = the max_records-th largest key among the candidates;
    every candidate above T, and the first max_records - #{key > T} candidates with key == T in index order."""
    keys = np.asarray(keys, np.uint32)
    cand = np.asarray(cand, bool)
    n, B = keys.size, int(max_records)
    assert B >= 1 and cand.size == n
    idx = np.flatnonzero(cand)
    if idx.size <= B:
        return idx, dict(zip(COUNTS, (n, int(idx.size), int(idx.size), 0, 0, 0)))
    ck = keys[idx]
    T = np.sort(ck)[ck.size - B]                        # ascending: position size - B holds the B-th largest
    gt = idx[ck > T]
    ties = idx[ck == T]
    quota = B - gt.size
    assert 1 <= quota <= ties.size
    kept = np.sort(np.concatenate([gt, ties[:quota]]))
    return kept, dict(zip(COUNTS, (n, int(idx.size), B, int(T), int(quota), int(ties.size))))


def select_by_sort(keys, cand, max_records):
    """The same kept set, independently: stable-sort the candidates by key descending, take the first max_records, restore index order."""
    keys = np.asarray(keys, np.uint32)
    idx = np.flatnonzero(np.asarray(cand, bool))
    order = np.argsort(-keys[idx].astype(np.int64), kind="stable")
    return np.sort(idx[order[:int(max_records)]])
