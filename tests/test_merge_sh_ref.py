"""CPU: the restatement of pin 5s (tests/merge_sh_ref.py) against what can be known without it — the linearity of the 3DGS colour in the
coefficients, the colour rule of merge_ref.parent, passthrough, both fallbacks, the tree's planes and a cut's rows — and the symbols and
the NULL handling of the new entry points (no compute calls)."""
import ctypes as C

import numpy as np

import compact_ref as cr
import lod_ref as lr
import merge_ref as mr
import merge_sh_ref as ms
from mesh2splat_amd import _lib
from mesh2splat_amd import bake as bk

F = np.float32
NEW = ("m2s_set_carry_sh", "m2s_carry_sh", "m2s_upload_sh", "m2s_sh_plane_info", "m2s_device_lod_sh", "m2s_download_lod_sh", "m2s_last_merge_sh_ms")
CONFIGS = ((10, 4, 0.5), (3, 5, 0.5), (10, 64, -2.0))


def test_symbols_exported(hiplib):
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(hiplib, name), name


def test_null_context_and_signatures(hiplib):
    rows, degree, plane = C.c_uint64(7), C.c_uint32(7), (C.c_float * 48)()
    assert hiplib.m2s_set_carry_sh(None, 1) == 1 and hiplib.m2s_carry_sh(None) == 0
    assert hiplib.m2s_upload_sh(None, plane, 1, 3) == 1
    assert hiplib.m2s_sh_plane_info(None, C.byref(rows), C.byref(degree)) == 1 and rows.value == 0 and degree.value == 0
    assert not hiplib.m2s_device_lod_sh(None)
    degree.value = 7
    assert hiplib.m2s_download_lod_sh(None, plane, 1, C.byref(degree)) == 1 and degree.value == 0
    assert hiplib.m2s_last_merge_sh_ms(None) == 0.0
    assert hiplib.m2s_last_merge_sh_ms.restype is C.c_float and hiplib.m2s_device_lod_sh.restype is C.c_void_p


def _case(level, max_group, dot, n=300, seed=11, nonfinite=False):
    rec = mr.crafted_records(n, seed)
    sh = ms.random_plane(n, seed, nonfinite, cr.valid_mask(rec))
    perm, heads = ms.heads_of(rec, level, max_group, dot)
    plane, info = ms.merge_plane(rec, sh, perm, heads)
    return rec, sh, perm, heads, plane, info


def test_the_parents_colour_is_the_weighted_mean_of_its_members_colours_in_every_direction():
    """0.5 + sum sh_k B_k(dir) is linear in sh: in float64, before the final rounding, the parent's colour along a direction equals the
    a_i-weighted mean of the members' colours along it, within 1e-12 of the largest member colour's magnitude (a dozen fp64 roundings of
    48-term sums whose terms are bounded by it)."""
    rng = np.random.default_rng(3)
    checked = 0
    for level, max_group, dot in CONFIGS:
        rec, sh, perm, heads, _, info = _case(level, max_group, dot)
        ends = np.append(heads[1:], len(rec))
        for s in np.flatnonzero((info["members"] >= 2) & ~info["by_area"]):
            idx = perm[heads[s]:ends[s]]
            r = rec[idx].astype(np.float64)
            w = np.ones(len(idx)) if info["unit"][s] else r[:, 8] * r[:, 9]
            a = w * r[:, 7]
            d = rng.normal(0, 1, 3)
            d /= np.sqrt(d @ d)
            dirs = np.repeat(d[None], len(idx), 0)
            cols = bk.eval_sh(sh[idx], dirs)                                         # (m, 3) float64
            want = (a[:, None] * cols).sum(0) / a.sum()
            got = bk.eval_sh(info["exact"][s][None], d[None])[0]
            B = np.abs(bk.sh_basis(d[None])[0])
            scale = 0.5 + max((np.abs(sh[idx, 3 * 0:3].astype(np.float64)) * B[0]).max(),
                              (np.abs(sh[idx, 3:].astype(np.float64)).reshape(len(idx), 3, 15) * B[1:]).sum(-1).max())
            assert np.abs(got - want).max() <= 1e-12 * max(scale, np.abs(cols).max()), (s, got, want)
            checked += 1
    assert checked > 100


def test_a_plane_that_holds_the_colour_follows_the_colour_rule():
    """dc = (rgb - 0.5) / C0 and rest 0: the merged dc gives back merge_ref.parent's rgb.  Within 2 fp32 ulps of a colour in [0.5, 1)
    (2^-23): the stored dc_i are rounded (C0 |dc_i| 2^-24 <= 2^-25 in colour), the merged dc is rounded once (2^-25), and so is rgb' (2^-25)."""
    rec = mr.crafted_records(300, 11)
    sh = np.zeros((300, 48), F)
    sh[:, 0:3] = ((rec[:, 4:7].astype(np.float64) - 0.5) / bk.C0).astype(F)
    for level, max_group, dot in CONFIGS:
        want, _, _, info, plane, pinfo = ms.merge(rec, sh, level, max_group, dot)
        multi = np.flatnonzero(pinfo["members"] >= 2)
        assert multi.size and all(info[s] is not None for s in multi)
        back = 0.5 + bk.C0 * plane[multi, 0:3].astype(np.float64)
        assert np.abs(back - want[multi, 4:7].astype(np.float64)).max() <= 2.0 ** -23
        assert not plane[:, 3:].any()                                                # columns of zeros stay zero


def test_singletons_and_invalid_records_are_copied_by_bits():
    rec, sh, perm, heads, plane, info = _case(3, 5, 0.5, nonfinite=True)
    bad = np.flatnonzero(~cr.valid_mask(rec))
    assert bad.size == 3
    sh[bad[0], 7] = np.float32(np.nan)                                               # a row of an invalid record: copied whatever it holds
    sh[bad[1], :] = F(-0.0)
    plane, info = ms.merge_plane(rec, sh, perm, heads)
    single = np.flatnonzero(info["members"] == 1)
    assert single.size > 50
    assert np.array_equal(plane[single].view(np.uint32), sh[perm[heads[single]]].view(np.uint32))
    S = len(heads)
    assert list(perm[heads[S - 3:]]) == list(bad) and (info["members"][S - 3:] == 1).all()   # the invalid ones, last, in index order


def test_both_fallbacks_are_hit():
    rec, sh, perm, heads, plane, info = _case(10, 4, 0.5)
    multi = info["members"] >= 2
    assert int(multi.sum()) == 61 and int(info["unit"].sum()) == 2 and int(info["by_area"].sum()) == 1
    ends = np.append(heads[1:], len(rec))
    for s in np.flatnonzero(info["unit"]):                                           # W == 0: the plain (alpha-weighted) mean
        idx = perm[heads[s]:ends[s]]
        al = rec[idx, 7].astype(np.float64)
        x = sh[idx].astype(np.float64)
        want = (al[:, None] * x).sum(0) / al.sum() if al.sum() != 0 else x.sum(0) / len(idx)
        assert np.allclose(plane[s], want, rtol=1e-6, atol=0)
    for s in np.flatnonzero(info["by_area"] & ~info["unit"]):                        # A == 0: the area-weighted mean
        idx = perm[heads[s]:ends[s]]
        w = rec[idx, 8].astype(np.float64) * rec[idx, 9].astype(np.float64)
        assert (w * rec[idx, 7] == 0).all() and w.sum() > 0
        assert np.allclose(plane[s], (w[:, None] * sh[idx]).sum(0) / w.sum(), rtol=1e-6, atol=0)
    assert np.isfinite(plane[multi]).all()
    _, _, _, _, _, info = _case(10, 64, -2.0)
    assert int(info["members"].max()) == 64


def test_nonfinite_coefficients_stay_in_their_class():
    rec, sh, perm, heads, plane, info = _case(10, 64, -2.0, nonfinite=True)
    assert np.isinf(sh).sum() == 1 and np.isnan(sh).sum() == 1
    bad = ~np.isfinite(plane)
    assert 1 <= bad[:, 5].sum() and 1 <= bad[:, 17].sum() and bad.sum() == bad[:, 5].sum() + bad[:, 17].sum()
    assert ms.compare(plane, plane, info) == 0.0


def test_a_chain_of_merges_is_the_trees_plane_and_a_cut_takes_its_rows():
    rec = mr.crafted_records(300, 11)
    sh = ms.random_plane(300, 11)
    levels = (3, 10)
    recs, planes, parent, first = ms.chain(rec, sh, levels)
    assert len(recs) == 3 and first[-1] == sum(len(p) for p in planes)
    # the same merges run one by one
    r1, _, _, _, p1, _ = ms.merge(rec, sh, 3)
    r2, _, _, _, p2, _ = ms.merge(r1, p1, 10)
    assert np.array_equal(planes[0].view(np.uint32), sh.view(np.uint32))
    assert np.array_equal(planes[1].view(np.uint32), p1.view(np.uint32)) and np.array_equal(planes[2].view(np.uint32), p2.view(np.uint32))
    assert np.array_equal(recs[2].view(np.uint32), r2.view(np.uint32))
    tree_rec, tree_sh = np.concatenate(recs), np.concatenate(planes)
    sel = lr.select(lr.bounds(tree_rec), parent, first, (0.0, 0.0, 4.0), 300.0, tau_px=8.0)
    assert 0 < sel["per_level"][0] < first[1] and sum(sel["per_level"][1:]) > 0       # a cut through more than one level
    rows = ms.cut_plane(tree_sh, sel["nodes"])
    assert rows.shape == (sel["counts"]["selected"], 48)
    assert np.array_equal(rows.view(np.uint32), tree_sh[sel["flags"]].view(np.uint32))
    # a step that merges nothing adds no rows
    _, planes2, _, first2 = ms.chain(rec, sh, (10, 10), 64, -2.0)
    _, planes3, _, first3 = ms.chain(rec, sh, (10, 10, 10), 64, -2.0)                # (one run of valid records: the third step finds one parent)
    assert len(first2) == 4 and first3 == first2 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(planes3, planes2))


def test_three_hundred_thousand_records_cost_seconds():
    n = 300003
    rng = np.random.default_rng(5)
    base = mr.crafted_records(4099, 77)
    rec = base[rng.integers(0, len(base), n)]
    rec[:, 0:3] = rng.normal(0, 1, (n, 3)).astype(F)
    sh = ms.random_plane(n, 5)
    perm, heads = ms.heads_of(rec, 10, 64, -2.0)
    plane, info = ms.merge_plane(rec, sh, perm, heads)
    assert len(plane) == len(heads) and int(info["members"].max()) == 64
    multi = info["members"] >= 2
    assert np.isfinite(plane[multi]).all() and (np.abs(plane[multi]) <= info["mag"][multi] * (1 + 1e-6)).all()   # a convex combination
