"""CPU: the restatement of m2s_lod_blend (tests/lod_blend_ref.py) against what the blend is for — the eight turns of a frame leave the
covariance alone, the weight is a monotone value in [0, 1], and one key below a parent's threshold its children ARE the parent, up to
rounding — and the entry points' interface (no device needed)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import lod_blend_ref as br
import lod_budget_ref as lb
import lod_ref as lr
import merge_ref as mr
from mesh2splat_amd import lod
from test_lod_ref import random_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CAMERAS = ((0.5, 0.5, 3.0), (3.0, 0.5, -2.0))
FOCAL, NEAR = 512.0, 0.05


def tree_of(rec, levels, max_group=4, dot=0.5):
    """rec through merge_ref.merge at `levels` -> (tree (nodes, 24), parent, first, bounds); a step that merges nothing adds no level"""
    out, maps = [np.ascontiguousarray(rec, F)], []
    for lv in levels:
        nxt, mp, _, _ = mr.merge(out[-1], lv, max_group, dot)
        if len(nxt) == len(out[-1]):
            continue
        out.append(nxt)
        maps.append(mp)
    parent, first = lr.link(maps, [len(v) for v in out])
    tree = np.concatenate(out)
    return tree, parent, first, lr.bounds(tree)


@pytest.fixture(scope="module")
def grid_tree():
    tree, parent, first, b = tree_of(mr.grid_records(8), (8, 9, 10))
    assert first == [0, 64, 80, 84, 85]
    return tree, parent, first, b


@pytest.fixture(scope="module")
def crafted_tree():
    tree, parent, first, b = tree_of(mr.crafted_records(600, 3, invalid=False), (3, 6, 10))
    assert len(first) == 5
    return tree, parent, first, b


def random_unit(rng, n):
    q = rng.normal(0, 1, (n, 4))
    return (q / np.linalg.norm(q, axis=1)[:, None]).astype(F)


def record_with(q, sx, sy, sz=1e-3):
    rec = np.zeros(24, F)
    rec[8:11] = (sx, sy, sz)
    rec[16:20] = q
    return rec


def cov_rel(a, b):
    """the largest difference of two records' viewer covariances, relative to the largest entry of b's"""
    ca, cb = mr.viewer_cov(a), mr.viewer_cov(b)
    return float(np.abs(ca - cb).max() / np.abs(cb).max())


# ---- (a) candidates -------------------------------------------------------------------------------------------------------------------
def test_every_candidate_draws_the_parents_covariance():
    rng = np.random.default_rng(7)
    quats = random_unit(rng, 200)
    worst = 0.0
    for q in quats:
        sx, sy = np.exp(rng.normal(-2, 1, 2))
        want = record_with(q, sx, sy)
        for k, cand in enumerate(br.candidates(q)):
            got = record_with(cand, *((sy, sx) if k & 1 else (sx, sy)))
            worst = max(worst, cov_rel(got, want))
    print(f"lod blend candidates: covariance within {worst:.3g} of the parent's largest entry")
    assert worst < 1e-6


def test_each_turn_wins_where_the_child_is_that_turn_and_a_non_unit_parent_is_not_turned():
    rng = np.random.default_rng(8)
    seen = set()
    for q in random_unit(rng, 20):
        cands = br.candidates(q)
        for k in range(8):
            for sign in (1, -1):
                child = (F(sign) * cands[k]).astype(F)
                got_k, cand = br.frame(child[None], q[None])
                assert got_k[0] == k, (k, sign, got_k)
                assert np.abs(cand[0] - child).max() < 1e-6                       # the candidate, with the child's sign
                seen.add(k)
            big = (q * F(1.1)).astype(F)                                          # |q|^2 = 1.21: not unit
            assert not br.is_unit(big) and br.frame(br.candidates(big)[k][None], big[None])[0][0] == 0
    assert seen == set(range(8))
    nan = np.array([[np.nan, 0, 0, 1]], F)                                         # a NaN parent: not unit, k = 0; a NaN child: no score wins
    assert br.frame(random_unit(rng, 1), nan)[0][0] == 0 and br.frame(nan, random_unit(rng, 1))[0][0] == 0
    assert br.is_unit(np.array([1, 0, 0, 0], F)) and br.is_unit(np.array([1 + 2.0 ** -12, 0, 0, 0], F))


# ---- (b) weight -----------------------------------------------------------------------------------------------------------------------
def test_the_weight_on_random_trees():
    rng = np.random.default_rng(19)
    inside = 0
    for _ in range(200):
        b, parent, first = random_tree(rng)
        cam, focal = rng.normal(0, 2, 3), float(rng.uniform(50, 2000))
        tau, band = float(rng.choice([0.0, 0.5, 1.0, 4.0, 30.0])), float(rng.choice([1.0, 0.25, 2.0 ** -20]))
        ids = np.arange(first[-1], dtype=np.uint32)
        info = {}
        t = br.weights(b, parent, ids, cam, focal, tau, NEAR, band, info)
        assert t.dtype == F and (t >= 0).all() and (t <= 1).all() and not np.signbit(t).any()
        assert (t[first[-2]:] == 0).all() and np.isnan(info["den"][first[-2]:]).all()
        assert (t[:first[-2]][~(info["den"][:first[-2]] > 0)] == 0).all()
        inside += int(np.count_nonzero((t > 0) & (t < 1)))
        c = b.copy()                                                                 # NaN bounds, of a node and of a parent: 0
        c[0, 3], c[1, 0], c[int(parent[2]), 3] = np.nan, np.nan, np.nan
        tn = br.weights(c, parent, ids, cam, focal, tau, NEAR, band)
        assert tn[0] == 0 and tn[2] == 0 and 0 <= tn[1] <= 1                        # (a NaN position is `near` away: a value, not a NaN)
        assert (tn[np.flatnonzero(parent == parent[2])] == 0).all()                  # every child of the NaN parent
        # t does not decrease with the bits of tau_px, over the keys at which a cut can change
        L, H, _ = lb.intervals(b, parent, first, cam, focal, NEAR)
        keys = np.array(lb.endpoints(L, H), np.uint32)
        tk = br.weights(b, parent, ids, cam, focal, keys.view(F)[:, None], NEAR, band)
        assert tk.shape == (len(keys), first[-1]) and (np.diff(tk, axis=0) >= 0).all()
    assert inside > 100                                                              # (the cases reach the inside of the interval)


# ---- (c) continuity -------------------------------------------------------------------------------------------------------------------
def children_before_the_switch(tree, parent, first, b, cam, band=1.0):
    """for every node P above the leaves: the cut one key below T(P), and of its records the children of P, blended -> a list of
    (P, child nodes, t, blended records)"""
    T = lb.thresholds(b, cam, FOCAL, NEAR)
    out = []
    for P in range(first[1], first[-1]):
        if T[P] == 0:
            continue
        tau = lb.tau_of(int(T[P]) - 1)
        ids = lr.select(b, parent, first, cam, FOCAL, tau, NEAR)["nodes"]
        res = br.blend(tree, parent, b, ids, cam, FOCAL, tau, NEAR, band)
        mine = np.flatnonzero(parent[ids] == P)
        out.append((P, ids[mine], res["t"][mine], res["records"][mine], res["den"][mine]))
    return out


def field_rel(got, want):
    return float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max() / np.abs(want.astype(np.float64)).max())


@pytest.mark.parametrize("cam", CAMERAS)
def test_one_key_below_the_switch_the_children_are_the_parent_on_the_quadtree(grid_tree, cam):
    tree, parent, first, b = grid_tree
    n, t_min, worst_f, worst_c = 0, 1.0, 0.0, 0.0
    for P, kids, t, rec, _ in children_before_the_switch(tree, parent, first, b, cam):
        n += len(kids)
        for tj, r in zip(t, rec):
            t_min = min(t_min, float(tj))
            worst_f = max(worst_f, field_rel(r[0:3], tree[P, 0:3]), field_rel(r[4:8], tree[P, 4:8]))
            worst_c = max(worst_c, cov_rel(r, tree[P]))
    print(f"lod blend continuity cam={cam}: {n} children, min t {t_min:.9g}, position/colour within {worst_f:.3g}, covariance within {worst_c:.3g}")
    assert n == 84
    assert t_min >= 1 - 2.0 ** -20 and worst_f <= 2.0 ** -18 and worst_c <= 1e-5


def test_sizes_that_go_down_along_a_chain_give_no_blend(crafted_tree):
    """crafted records: a parent may project no larger than its child (den <= 0), and the same minimum is 0"""
    tree, parent, first, b = crafted_tree
    t_min, shrinking = 1.0, 0
    for cam in CAMERAS:
        for P, kids, t, rec, den in children_before_the_switch(tree, parent, first, b, cam):
            if len(kids):
                t_min = min(t_min, float(t.min()))
            off = ~(den > 0)
            shrinking += int(off.sum())
            assert (t[off] == 0).all() and np.array_equal(rec[off].view(np.uint32), tree[kids[off]].view(np.uint32))
    assert t_min == 0 and shrinking > 0


# ---- (d) forced t = 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("grid", "crafted"))
def test_at_t_one_a_record_is_its_parent(grid_tree, crafted_tree, which):
    tree, parent, first, b = grid_tree if which == "grid" else crafted_tree
    ids = np.arange(first[-2], dtype=np.uint32)
    rec, k = br.blend_records(tree, parent, ids, np.ones(len(ids), F))
    par = tree[parent[ids]]
    assert np.array_equal(rec[:, br.LERPED], par[:, br.LERPED])
    assert np.array_equal(rec[:, br.KEPT].view(np.uint32), tree[ids][:, br.KEPT].view(np.uint32))
    same = k == 0
    assert np.array_equal(rec[same][:, br.ROT], par[same][:, br.ROT]) and np.array_equal(rec[same][:, br.EDGES], par[same][:, br.EDGES])
    unit = br.is_unit(par[:, br.ROT])
    assert not (k[~unit] != 0).any()
    worst = max([cov_rel(r, p) for r, p in zip(rec[~same], par[~same])], default=0.0)
    print(f"lod blend t = 1 ({which}): {int((~same).sum())} of {len(ids)} turned, covariance within {worst:.3g}")
    assert worst <= 1e-6
    if which == "crafted":
        assert (~same).any() and same.any()


# ---- (e) copies -----------------------------------------------------------------------------------------------------------------------
def test_copies_and_the_sh_rows(crafted_tree):
    tree, parent, first, b = crafted_tree
    rng = np.random.default_rng(3)
    sh = rng.normal(0, 1, (first[-1], 48)).astype(F)
    cam = CAMERAS[1]
    L, H, _ = lb.intervals(b, parent, first, cam, FOCAL, NEAR)
    keys = lb.endpoints(L, H)
    copies = total = 0
    for key in keys[1::max(1, len(keys) // 12)]:
        tau = lb.tau_of(key)
        ids = lr.select(b, parent, first, cam, FOCAL, tau, NEAR)["nodes"]
        wide = br.blend(tree, parent, b, ids, cam, FOCAL, tau, NEAR, 1.0, sh)
        off = wide["t"] == 0
        assert np.array_equal(wide["records"][off].view(np.uint32), tree[ids[off]].view(np.uint32))
        assert np.array_equal(wide["sh"][off].view(np.uint32), sh[ids[off]].view(np.uint32))
        on = ~off
        assert wide["counts"]["blended"] == int(on.sum()) and wide["counts"]["records"] == len(ids)
        assert np.array_equal(wide["sh"][on], br.lerp(wide["t"][on][:, None], sh[ids[on]], sh[parent[ids[on]]]))
        full = wide["t"] == 1
        assert np.array_equal(wide["sh"][full], sh[parent[ids[full]]])
        thin = br.blend(tree, parent, b, ids, cam, FOCAL, tau, NEAR, 2.0 ** -20, sh)
        assert (thin["t"] <= wide["t"]).all()
        copies += int((thin["t"] == 0).sum())
        total += len(ids)
        assert np.array_equal(thin["records"][thin["t"] == 0].view(np.uint32), tree[ids[thin["t"] == 0]].view(np.uint32))
    print(f"lod blend band 2^-20: {copies} of {total} records are copies")
    assert total > 1000 and copies >= 0.98 * total


# ---- (f) interface --------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_the_header(tmp_path):
    assert C.sizeof(lod.LodBlendParamsC) == 32
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    fields = [f[0] for f in lod.LodBlendParamsC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "m2s.h"\nint main(void){\nprintf("%zu\\n", sizeof(m2s_lod_blend_params));\n' +
                   "".join('printf("%%zu\\n", offsetof(m2s_lod_blend_params, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [32] + [getattr(lod.LodBlendParamsC, f).offset for f in fields]


def test_symbols_null_contexts_and_blend_to_c(hiplib):
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    p = lod.blend_to_c((1, 2, 3), 500.0, 2.0, 0.1, 0.25)
    assert (list(p.camera_position), p.focal_px, p.tau_px, p.band, p.reserved) == ([1.0, 2.0, 3.0], 500.0, 2.0, 0.25, 0)
    assert abs(p.near - 0.1) < 1e-8 and lod.blend_to_c((0, 0, 0), 1.0, 0.0).band == 1.0
    assert hiplib.m2s_lod_blend(None, C.byref(p), out) == 1 and list(out) == [0, 0, 0, 0]
    n = C.c_uint64(5)
    assert hiplib.m2s_download_lod_blend_t(None, None, 0, C.byref(n)) == 1 and n.value == 0
    assert hiplib.m2s_device_lod_blend_t(None) is None and hiplib.m2s_last_lod_blend_ms(None) == 0.0
    assert hiplib.m2s_last_lod_blend_counts(None, None) == 1 and hiplib.m2s_last_lod_blend_stage_ms(None, None) == 1
    for band in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            lod.blend_to_c((0, 0, 0), 500.0, 1.0, 0.1, band)
