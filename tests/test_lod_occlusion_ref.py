"""CPU: the restatement of the cuts behind an occluder (tests/lod_occlusion_ref.py) held to the pin in include/m2s.h, to the frustum
restatement it stands on and to the oracle's prepass with its depth test: visibility is "a leaf below is inside", the masked interval
rule is the masked cut at every key where anything changes, the count never increases, the search is tight and never coarser than the
frustum search.  Then why the pin is not "depth-test every selected node's own position", the struct against the C compiler's layout,
the symbols and the NULL checks."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import camera
import lod_budget_ref as br
import lod_frustum_ref as fr
import lod_occlusion_ref as oc
import lod_ref as lr
import merge_ref as mr
from mesh2splat_amd import lod
from mesh2splat_amd.prepass import PrepassParams
from test_lod_frustum_ref import EYE, PROJ, frustum_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ALPHAS = np.array([0.5, 0.95, np.nextafter(F(0.95), F(1)), 1.0, np.nan], F)


def occlusion_tree(rng, k):
    """test_lod_frustum_ref's tree and camera number k (the same 200 for the same generator), an alpha per node (1 but for every third,
    which takes one of ALPHAS in turn) and a small depth image made from the restatement's own depths for that camera"""
    b, parent, first, cam, focal, near, frustum = frustum_tree(rng, k)
    alpha = np.ones(first[-1], F)
    alpha[::3] = ALPHAS[np.arange(len(alpha[::3])) % len(ALPHAS)]
    depth = oc.median_depth_image(b, alpha, first, frustum, 16, 9, rng=np.random.default_rng(1000 + k) if k % 4 else None)
    if k % 10 == 1:                                          # an occluder in front of everything, and nothing translucent
        alpha[:], depth[:] = 1.0, 0.0
    return b, alpha, parent, first, cam, focal, near, frustum, depth


def visible_by_walking(b, alpha, parent, first, frustum, depth):
    vis = np.zeros(first[-1], bool)
    for leaf in np.flatnonzero(oc.inside(b[:first[1]], alpha[:first[1]], frustum, depth)):
        i = int(leaf)
        while i != int(lr.NO_PARENT):
            vis[i] = True
            i = int(parent[i])
    return vis


def test_masked_cut_interval_rule_and_search_on_random_trees():
    rng = np.random.default_rng(23)
    seen = {"occluded": 0, "kept": 0, "partly": 0, "none_visible": 0, "finer_than_frustum": 0, "unmet": 0, "inner_dropped": 0, "nan_leaf_inside": 0}
    for k in range(200):
        b, alpha, parent, first, cam, focal, near, frustum, depth = occlusion_tree(rng, k)
        n0, last = first[1], first[-1] - first[-2]
        L, H, T, vis = oc.intervals(b, alpha, parent, first, cam, focal, near, frustum, depth)
        assert np.array_equal(vis, visible_by_walking(b, alpha, parent, first, frustum, depth)), k
        Lf, Hf, _, visf = fr.intervals(b, parent, first, cam, focal, near, frustum)
        assert not (vis & ~visf).any() and np.array_equal(H, Hf)
        cnt = oc.counts(b, alpha, first, frustum, depth)
        ins = vis[:n0]
        assert cnt["visible_leaves"] == int(visf[:n0].sum()) == int(ins.sum()) + cnt["occluded_leaves"]
        seen["occluded"] += cnt["occluded_leaves"]
        seen["kept"] += cnt["translucent_kept"]
        seen["partly"] += bool(ins.any() and cnt["occluded_leaves"])
        seen["none_visible"] += bool(visf[:n0].any() and not ins.any())
        seen["nan_leaf_inside"] += int(np.count_nonzero(np.isnan(b[:n0, 0:3]).any(axis=1) & ins))
        assert (np.isnan(b[:n0, 0:3]).any(axis=1) <= ins).all()
        prev = None
        for e in br.endpoints(L, H):
            for key in ((e - 1, e) if e else (e,)):
                sel = oc.select(b, alpha, parent, first, cam, focal, br.tau_of(key), near, frustum, depth, vis=vis)
                assert np.array_equal(br.flags_at(L, H, key), sel["flags"]), (k, key)
                assert oc.cut_ok(parent, first, sel["flags"], vis), (k, key)        # restricted to the inside leaves
                assert sel["culled"] == int((sel["plain"] & ~vis).sum())
                seen["inner_dropped"] += int((sel["plain"] & ~vis)[n0:].sum())
                c = br.count(L, H, key)
                assert c == sel["counts"]["selected"] == sum(sel["per_level"]) and (prev is None or c <= prev), (k, key)
                prev = c
        last_vis = int(vis[first[-2]:].sum())
        assert br.count(L, H, br.KEY_MAX) == last_vis
        for budget in oc.budgets(L, H, first, vis):
            got = oc.search(L, H, first, vis, budget)
            n_eff = max(budget, last_vis)
            assert got["n_eff"] == n_eff and got["selected"] == br.count(L, H, got["key"]) <= n_eff
            assert got["key"] == 0 or br.count(L, H, got["key"] - 1) > n_eff
            assert got["met"] == (got["selected"] <= budget) and got["met"] == (budget >= last_vis)
            seen["unmet"] += not got["met"]
            if budget >= last:
                wide = fr.search(Lf, Hf, first, visf, budget)
                assert got["key"] <= wide["key"], (k, budget)
                seen["finer_than_frustum"] += got["key"] < wide["key"]
    print(f"lod occlusion restatement, over 200 trees: {seen}")
    assert all(v > 0 for v in seen.values()), seen


def test_the_own_position_depth_test_drops_visible_surface():
    """Why the leaf rule: a caller who runs the prepass's depth test on a cut tests every selected node at its own position.  Over the
    200 trees, at the endpoints of the plain intervals: the trees in which a selected node above the leaves fails the test itself while
    a leaf below it passes: the prepass would remove surface that the camera sees."""
    rng = np.random.default_rng(23)
    trees = 0
    for k in range(200):
        b, alpha, parent, first, cam, focal, near, frustum, depth = occlusion_tree(rng, k)
        n0 = first[1]
        vis = oc.visibility(b, alpha, parent, first, frustum, depth)
        own = oc.inside(b, alpha, frustum, depth)
        Lp, Hp, _ = br.intervals(b, parent, first, cam, focal, near)
        hit = False
        for key in br.endpoints(Lp, Hp):
            flags = lr.select(b, parent, first, cam, focal, br.tau_of(key), near)["flags"]
            hit = hit or bool((flags & ~own & vis)[n0:].any())
        trees += hit
    print(f"own-position depth test: a selected inner node fails it over a visible leaf in {trees} of 200 trees")
    assert trees > 0


@pytest.mark.parametrize("with_model", (False, True))
def test_inside_with_the_prepass_constants_is_what_the_oracle_prepass_keeps(oracle, with_model):
    """guard 1.05 and bias 2e-5 against the oracle's prepass with depth_test_mesh = 1 and the same image, record by record"""
    rec = mr.crafted_records(400, 5, invalid=False)
    rec[:, 8:10] = np.maximum(rec[:, 8:10], F(1e-3))
    rec[::3, 7] = ALPHAS[np.arange(len(rec[::3])) % len(ALPHAS)]
    rec[1::3, 7] = 1.0
    model = camera.trs((0.1, -0.05, 0.0), (0, 0, 1), 20.0, (1.5, 1.5, 1.5)) if with_model else EYE
    view = camera.look_at((0.4, 0.3, 4.0), (0.0, 0.1, 0.0))
    frustum = (model, view, PROJ, 1.05)
    b = lr.bounds(rec)
    first = [0, len(rec)]
    depth = oc.median_depth_image(b, rec[:, 7], first, frustum, 16, 9, rng=np.random.default_rng(3))
    pp = PrepassParams(view_mat=view, proj_mat=PROJ, model_mat=model, renderer_resolution=(640, 360), resolution_target=1,
                       perform_mesh_depth_test=True, mesh_depth=depth)
    kept = np.array([oracle.prepass(pp, rec[i:i + 1])[0] == 1 for i in range(len(rec))])
    t = oc.leaf_test(b, rec[:, 7], frustum, depth)
    assert np.array_equal(t["inside"], kept), np.flatnonzero(t["inside"] != kept)
    assert t["occluded"].sum() > 20 and t["kept"].sum() > 0 and t["inside"].sum() > 20
    assert (t["in_frustum"] & ~t["behind"] & (t["my"] == t["d"] + F(oc.BIAS))).sum() > 0           # ties: equality does not occlude


def test_texel_clamp_nan_and_ties():
    """one leaf per case, through the identity matrices (clip = position, w = 1): inside a texel, on the right and top border, beyond
    them under a wide guard, NaN; a tie with the bias; NaN texel and NaN alpha keep the leaf"""
    depth = np.full((2, 4), 0.5, F)
    depth[1, 3], depth[0, 0] = 0.9, np.nan
    fru = (EYE, EYE, EYE, 4.0)
    b = np.zeros((8, 4), F)
    b[0, 0:3] = (0.1, 0.1, 0.5)                              # u = .55 -> ti 2, v -> tj 1; my = .75 > .5: behind
    b[1, 0:3] = (1.0, 1.0, 0.7)                              # u = 1 -> floor(4) = 4 -> clamp 3; tj clamp 1; my = .85 <= .9: not behind
    b[2, 0:3] = (3.0, 3.0, 0.9)                              # guard 4: inside; clamped to (3, 1); my = .95 > .9
    b[3, 0:3] = (-3.0, -3.0, 0.0)                            # clamped to (0, 0): a NaN texel, never behind
    b[4, 0:3] = (np.nan, 0.0, 0.9)                           # NaN position: inside, texel 0 of its row
    b[5, 0:3] = (0.1, 0.1, 0.9)                              # behind, alpha .5: kept
    b[6, 0:3] = (0.1, 0.1, 0.9)                              # behind, alpha NaN: kept
    b[7, 0:3] = (0.1, 0.1, 0.0)                              # my = .5 == d + 0: a tie at bias 0
    alpha = np.array([1, 1, 1, 1, 1, 0.5, np.nan, 1], F)
    t = oc.leaf_test(b, alpha, fru, depth, 0.0)
    assert t["in_frustum"].all()
    assert (t["ti"][:4].tolist(), t["tj"][:4].tolist()) == ([2, 3, 3, 0], [1, 1, 1, 0])
    assert t["occluded"].tolist() == [True, False, True, False, False, False, False, False]
    assert t["kept"].tolist() == [False, False, False, False, False, True, True, False]
    assert t["inside"].tolist() == [False, True, False, True, True, True, True, True]
    assert not oc.leaf_test(b, alpha, fru, np.nextafter(depth, F(0)), 0.0)["inside"][7]


def test_struct_layout_matches_the_header(tmp_path):
    assert C.sizeof(lod.LodOccluderC) == 32
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    fields = [f[0] for f in lod.LodOccluderC._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "m2s.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(m2s_lod_occluder));\n' +
                   "".join('printf("%%zu\\n", offsetof(m2s_lod_occluder, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == 32
    assert out[1:] == [getattr(lod.LodOccluderC, f).offset for f in fields] == [0, 8, 12, 16, 20, 24]


def test_occluder_to_c():
    img = np.arange(12, dtype=np.float64).reshape(3, 4)[:, ::1] / 12
    c = lod.occluder_to_c(img)
    assert (c.depth_w, c.depth_h, c.depth_on_device) == (4, 3, 0) and c.depth_bias == float(F(2e-5)) and list(c.reserved) == [0, 0]
    kept = c._keep
    assert kept.dtype == F and c.depth == kept.ctypes.data and np.array_equal(kept, img.astype(F))
    assert np.array_equal(np.ctypeslib.as_array(C.cast(c.depth, C.POINTER(C.c_float)), (12,)), img.astype(F).reshape(-1))
    assert lod.occluder_to_c(img.astype(F)[:, ::2], depth_bias=0.5).depth_bias == 0.5         # (made contiguous)
    for bad in (np.zeros(4, F), np.zeros((0, 4), F), np.zeros((2, 2, 2), F)):
        with pytest.raises(ValueError):
            lod.occluder_to_c(bad)
    m = lod.occluder_of_mesh_depth(None)
    assert (m.depth, m.depth_w, m.depth_h) == (None, 0, 0) and m.depth_bias == float(F(2e-5))
    assert lod.occluder_of_mesh_depth(None, depth_bias=0.0).depth_bias == 0.0
    assert lod.OCCLUSION_COUNTS == ("visible_leaves", "occluded_leaves", "translucent_kept", "culled")


def test_symbols_and_null_contexts(hiplib):
    assert hiplib.m2s_lod_select_occluded and hiplib.m2s_lod_select_budget_occluded and hiplib.m2s_last_lod_occlusion_counts
    f = lod.frustum_to_c(EYE, EYE, PROJ)
    o = lod.occluder_to_c(np.ones((2, 2), F))
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    sp = lod.select_to_c((0, 0, 0), 500.0)
    assert hiplib.m2s_lod_select_occluded(None, C.byref(sp), C.byref(f), C.byref(o), out) == 1 and list(out) == [0, 0, 0, 0]
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    res = lod.LodBudgetResultC(3.0, 9, 9)
    bp = lod.budget_to_c((0, 0, 0), 500.0, 10)
    assert hiplib.m2s_lod_select_budget_occluded(None, C.byref(bp), C.byref(f), C.byref(o), C.byref(res), out) == 1
    assert list(out) == [0, 0, 0, 0] and (res.tau_px, res.met, res.selected_finer) == (0.0, 0, 0)
    assert hiplib.m2s_lod_select_budget_occluded(None, None, None, None, None, None) == 1
    four = (C.c_uint64 * 4)(5, 5, 5, 5)
    assert hiplib.m2s_last_lod_occlusion_counts(None, four) == 1


def test_occluder_without_frustum_is_a_value_error():
    from mesh2splat_amd.converter import Converter
    conv = Converter.__new__(Converter)                      # no context: the check comes first
    o = lod.occluder_to_c(np.ones((2, 2), F))
    with pytest.raises(ValueError):
        Converter.lod_select(conv, (0, 0, 0), 500.0, occluder=o)
    with pytest.raises(ValueError):
        Converter.lod_select_budget(conv, (0, 0, 0), 500.0, 10, occluder=o)
