"""CPU: the restatement of the cuts over a frustum (tests/lod_frustum_ref.py) held to the pin in include/m2s.h, to the restatements it
stands on (tests/lod_ref.py, tests/lod_budget_ref.py) and to the oracle's prepass: visibility is "a leaf below is inside", the masked
interval rule is the masked cut at every key where anything changes, the count never increases, the search is tight.  Then why the pin
is not "test every selected node's own position", the struct against the C compiler's layout, the symbols and the NULL checks."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import camera
import lod_budget_ref as br
import lod_frustum_ref as fr
import lod_ref as lr
import merge_ref as mr
from mesh2splat_amd import lod
from mesh2splat_amd.prepass import PrepassParams
from test_lod_budget_ref import random_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PROJ = camera.perspective(45.0, 16 / 9, 0.01, 100.0)
EYE = np.eye(4, dtype=F)


def frustum_tree(rng, k):
    """random_tree with a leaf whose position is NaN in every fifth tree, and a camera per tree: a look-at camera from the cut's own
    camera position towards a point of the cloud, every third looking away from it; every seventh tree a far camera that looks at
    the cloud and sees all of it (the random ones do not give that class by themselves)"""
    b, parent, first, cam, focal, near = random_tree(rng, k)
    if k % 5 == 0:
        b[int(rng.integers(0, first[1])), 1] = np.nan
    eye = np.asarray(cam, np.float64)
    target = rng.normal(0, 0.5, 3)
    if k % 3 == 0:
        target = eye + (eye - target)
    if k % 7 == 0:
        eye, target = np.array([0.3, -0.2, 40.0]), np.zeros(3)
    guard = (1.0, 1.05, 4.0)[k % 3] if k % 2 else 1.05
    return b, parent, first, cam, focal, near, (EYE, camera.look_at(eye, target), PROJ, guard)


def visible_by_walking(b, parent, first, frustum):
    """pin 2 said the other way round: every inside leaf marks its whole chain of ancestors"""
    vis = np.zeros(first[-1], bool)
    for leaf in np.flatnonzero(fr.inside(b[:first[1]], *frustum)):
        i = int(leaf)
        while i != int(lr.NO_PARENT):
            vis[i] = True
            i = int(parent[i])
    return vis


@pytest.fixture(scope="module")
def classes():
    seen = {"all_inside": 0, "none_inside": 0, "partly_inside": 0, "inner_dropped": 0, "mean_passes_no_leaf": 0, "nan_leaf_inside": 0}
    yield seen
    print(f"lod frustum restatement, classes: {seen}")
    assert all(v > 0 for v in seen.values()), seen


def test_masked_cut_interval_rule_and_search_on_random_trees(classes):
    rng = np.random.default_rng(23)
    seen = {"finer_than_plain": 0, "unmet": 0, "raised": 0}
    for k in range(200):
        b, parent, first, cam, focal, near, frustum = frustum_tree(rng, k)
        n0, last = first[1], first[-1] - first[-2]
        L, H, T, vis = fr.intervals(b, parent, first, cam, focal, near, frustum)
        assert np.array_equal(vis, visible_by_walking(b, parent, first, frustum)), k
        ins = vis[:n0]
        classes["all_inside"] += bool(ins.all())
        classes["none_inside"] += not ins.any()
        classes["partly_inside"] += bool(ins.any() and not ins.all())
        classes["nan_leaf_inside"] += int(np.count_nonzero(np.isnan(b[:n0, 0:3]).any(axis=1) & ins))
        classes["mean_passes_no_leaf"] += int(np.count_nonzero(fr.inside(b[n0:], *frustum) & ~vis[n0:]))
        assert (np.isnan(b[:n0, 0:3]).any(axis=1) <= ins).all()
        Lp, Hp, _ = br.intervals(b, parent, first, cam, focal, near)
        assert np.array_equal(H, Hp) and np.array_equal(L[vis], Lp[vis]) and np.array_equal(L[~vis], H[~vis])
        prev = None
        for e in br.endpoints(L, H):
            for key in ((e - 1, e) if e else (e,)):
                sel = fr.select(b, parent, first, cam, focal, br.tau_of(key), near, frustum, vis)
                assert np.array_equal(br.flags_at(L, H, key), sel["flags"]), (k, key)
                assert fr.cut_ok(parent, first, sel["flags"], vis), (k, key)
                assert sel["counts"]["refine"] == int(sel["refine"].sum()) and sel["visible_leaves"] == int(ins.sum())
                assert sel["culled"] == int((sel["plain"] & ~vis).sum())
                classes["inner_dropped"] += int((sel["plain"] & ~vis)[n0:].sum())
                c = br.count(L, H, key)
                assert c == sel["counts"]["selected"] == sum(sel["per_level"]) and (prev is None or c <= prev), (k, key)
                prev = c
        last_vis = int(vis[first[-2]:].sum())
        assert br.count(L, H, br.KEY_MAX) == last_vis
        for budget in fr.budgets(L, H, first, vis):
            got = fr.search(L, H, first, vis, budget)
            n_eff = max(budget, last_vis)
            assert got["n_eff"] == n_eff and got["selected"] == br.count(L, H, got["key"]) <= n_eff
            assert got["key"] == 0 or br.count(L, H, got["key"] - 1) > n_eff
            assert got["met"] == (got["selected"] <= budget) and got["met"] == (budget >= last_vis)
            assert got["selected_finer"] == (got["selected"] if got["key"] == 0 else br.count(L, H, got["key"] - 1))
            sel = fr.select(b, parent, first, cam, focal, got["tau_px"], near, frustum)
            assert sel["counts"]["selected"] == got["selected"] and fr.cut_ok(parent, first, sel["flags"], vis)
            seen["unmet"] += not got["met"]
            seen["raised"] += n_eff > budget
            if budget >= last:
                plain = br.search(Lp, Hp, first, budget)
                assert got["key"] <= plain["key"], (k, budget)
                seen["finer_than_plain"] += got["key"] < plain["key"]
            fl = fr.search(L, H, first, vis, budget, br.tau_of(got["key"] + 1000))
            assert fl["by_floor"] and fl["key"] == got["key"] + 1000 and fl["selected_finer"] == fl["selected"] <= got["selected"]
        if not ins.any():
            got = fr.search(L, H, first, vis, 5, 0.5)
            assert (got["tau_px"], got["selected"], got["met"], got["selected_finer"]) == (F(0.5), 0, True, 0)
            assert fr.search(L, H, first, vis, 5)["key"] == 0
    print(f"lod frustum restatement, over 200 trees: {seen}")
    assert all(v > 0 for v in seen.values()), seen


def test_the_own_position_rule_lets_the_count_rise_with_the_key():
    """Why pin 2 tests leaves only: with every selected node tested at its own position, a parent inside the frustum can replace
    children that are all outside, and the number of selected nodes goes UP while tau grows.  A radix descent over monotone counts has
    no defined answer then."""
    rng = np.random.default_rng(23)
    rising = 0
    for k in range(200):
        b, parent, first, cam, focal, near, frustum = frustum_tree(rng, k)
        Lp, Hp, _ = br.intervals(b, parent, first, cam, focal, near)
        counts = [int(fr.own_position_flags(b, parent, first, cam, focal, br.tau_of(key), near, frustum).sum()) for key in br.endpoints(Lp, Hp)]
        rising += any(c1 > c0 for c0, c1 in zip(counts, counts[1:]))
    print(f"own-position rule: the count rises with the key in {rising} of 200 trees")
    assert rising > 0


def test_inside_with_the_prepass_guard_is_what_the_oracle_prepass_keeps(oracle):
    """merge_ref.grid_records(4): 16 tiles on z = 0, through a camera that looks past one corner of the grid"""
    rec = mr.grid_records(4)
    model = camera.trs((0.1, -0.05, 0.0), (0, 0, 1), 20.0, (1.5, 1.5, 1.5))
    pp = PrepassParams(view_mat=camera.look_at((0.2, 0.3, 1.0), (-0.2, -0.1, 0.0)), proj_mat=PROJ, model_mat=model, renderer_resolution=(640, 360),
                       resolution_target=1)
    kept = np.array([oracle.prepass(pp, rec[i:i + 1])[0] == 1 for i in range(len(rec))])
    ins = fr.inside(lr.bounds(rec), pp.model_mat, pp.view_mat, pp.proj_mat, 1.05)
    assert np.array_equal(ins, kept) and 0 < ins.sum() < len(rec), (ins, kept)
    assert ins.sum() <= fr.inside(lr.bounds(rec), pp.model_mat, pp.view_mat, pp.proj_mat, 4.0).sum()


def test_a_leaf_at_nan_is_inside_and_carries_its_ancestors():
    parent, first = lr.link([np.array([0, 0, 1, 1], np.uint32), np.array([0, 0], np.uint32)], [4, 2, 1])
    b = np.zeros((7, 4), F)
    b[:, 2] = 50.0                                                       # behind a camera at the origin that looks down -z
    b[2, 0] = np.nan
    vis = fr.visibility(b, parent, first, (EYE, EYE, PROJ, 1.05))
    assert vis.tolist() == [False, False, True, False, False, True, True]


def test_struct_layout_matches_the_header(tmp_path):
    assert C.sizeof(lod.LodFrustumC) == 208
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    fields = [f[0] for f in lod.LodFrustumC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "m2s.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(m2s_lod_frustum));\n' +
                   "".join('printf("%%zu\\n", offsetof(m2s_lod_frustum, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == 208
    assert out[1:] == [getattr(lod.LodFrustumC, f).offset for f in fields] == [0, 64, 128, 192, 196]


def test_frustum_to_c():
    m, v, p = (np.arange(16, dtype=F).reshape(4, 4) + o for o in (0, 100, 200))
    c = lod.frustum_to_c(m, v, p)
    assert list(c.model_to_world) == list(range(16)) and list(c.world_to_view) == list(range(100, 116)) and list(c.view_to_clip) == list(range(200, 216))
    assert c.guard_band == float(F(1.05)) and list(c.reserved) == [0, 0, 0]
    assert lod.frustum_to_c(m, v, p, guard_band=4).guard_band == 4.0
    with pytest.raises(ValueError):
        lod.frustum_to_c(m[:3], v, p)
    pp = PrepassParams(view_mat=v, proj_mat=p, model_mat=m)
    d = lod.frustum_of(pp, 2.0)
    assert bytes(d)[:192] == bytes(c)[:192] and d.guard_band == 2.0


def test_symbols_and_null_contexts(hiplib):
    assert hiplib.m2s_lod_select_frustum and hiplib.m2s_lod_select_budget_frustum and hiplib.m2s_last_lod_frustum_counts
    f = lod.frustum_to_c(EYE, EYE, PROJ)
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    sp = lod.select_to_c((0, 0, 0), 500.0)
    assert hiplib.m2s_lod_select_frustum(None, C.byref(sp), C.byref(f), out) == 1 and list(out) == [0, 0, 0, 0]
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    res = lod.LodBudgetResultC(3.0, 9, 9)
    bp = lod.budget_to_c((0, 0, 0), 500.0, 10)
    assert hiplib.m2s_lod_select_budget_frustum(None, C.byref(bp), C.byref(f), C.byref(res), out) == 1
    assert list(out) == [0, 0, 0, 0] and (res.tau_px, res.met, res.selected_finer) == (0.0, 0, 0)
    assert hiplib.m2s_lod_select_budget_frustum(None, None, None, None, None) == 1
    two = (C.c_uint64 * 2)(5, 5)
    assert hiplib.m2s_last_lod_frustum_counts(None, two) == 1 and hiplib.m2s_last_lod_frustum_ms(None) == 0.0
