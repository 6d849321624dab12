"""-m gpu: m2s_lod_select_occluded and m2s_lod_select_budget_occluded (Converter.lod_select / .lod_select_budget with frustum= and
occluder=) against their numpy restatement (tests/lod_occlusion_ref.py, held to the pin and to the oracle's prepass by
tests/test_lod_occlusion_ref.py), against each other on a second context, against the frustum cuts they stand on and against the frame
the prepass draws afterwards.  Everything is compared for equality: flags through node ids, record bytes, counts, per-level counts, the
four occlusion counts, the bits of tau_px, met, selected_finer."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import camera
import lod_budget_ref as br
import lod_frustum_ref as fr
import lod_occlusion_ref as oc
import lod_ref as lr
import merge_ref as mr
import merge_sh_ref as ms
from mesh2splat_amd import lod, synth
from mesh2splat_amd._lib import M2SError
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.prepass import PrepassParams
from test_gpu_lod_budget import CHAINS, FOCAL, NEAR, bits, download_tree, special_records
from test_gpu_lod_frustum import EYE, PROJ, cameras

pytestmark = pytest.mark.gpu
F = np.float32
ALPHAS = np.array([0.5, 0.95, np.nextafter(F(0.95), F(1)), 1.0, np.nan], F)
W, H = 64, 36
# over the module, computed from the restatement alone: asserted by the last test
SEEN = {"cuts": 0, "partly_occluded": 0, "none_visible": 0, "translucent_kept": 0, "tie": 0, "clamped_at_guard_4": 0, "nan_leaf_inside": 0,
        "inner_dropped_own_passes": 0}


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(hiplib):
    c = Converter(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def holder(hiplib):
    c = Converter(0)
    yield c
    c.close()


def with_alphas(rec):
    """every third record's alpha takes one of ALPHAS in turn"""
    rec = rec.copy()
    rec[::3, 7] = ALPHAS[np.arange(len(rec[::3])) % len(ALPHAS)]
    return rec


def fc(frustum):
    return lod.frustum_to_c(*frustum)


def tally(tree, b, first, frustum, depth, bias, vis, sel):
    n0 = first[1]
    t = oc.leaf_test(b[:n0], tree[:n0, 7], frustum, depth, bias)
    SEEN["cuts"] += 1
    SEEN["partly_occluded"] += bool(t["occluded"].any() and t["inside"].any())
    SEEN["none_visible"] += bool(t["in_frustum"].any() and not t["inside"].any())
    SEEN["translucent_kept"] += int(t["kept"].sum())
    SEEN["tie"] += int(t["tie"].sum())
    SEEN["clamped_at_guard_4"] += int(t["clamped"].sum()) if frustum[3] == 4.0 else 0
    SEEN["nan_leaf_inside"] += int(np.count_nonzero(np.isnan(b[:n0, 0:3]).any(axis=1) & t["inside"]))
    own = oc.inside(b, tree[:, 7], frustum, depth, bias)                             # every node's own position and alpha through the leaf test
    SEEN["inner_dropped_own_passes"] += int((sel["plain"] & sel["vis_frustum"] & ~vis & own)[n0:].sum())


def check_cut(conv, tree, parent, b, first, frustum, depth, bias, vis, visf, cam, tau, got, focal=FOCAL, near=NEAR):
    """what `conv` holds after an occluded cut that returned `got`, against the restatement at tau"""
    sel = oc.select(b, tree[:, 7], parent, first, cam, focal, tau, near, frustum, depth, bias, vis=vis)
    sel["vis_frustum"] = visf
    assert {k: got[k] for k in lod.SELECT_COUNTS} == sel["counts"] and got["per_level"] == sel["per_level"]
    want4 = {k: sel[k] for k in lod.OCCLUSION_COUNTS}
    assert {k: got[k] for k in lod.OCCLUSION_COUNTS} == want4 == conv.last_lod_occlusion_counts()
    two = (C.c_uint64 * 2)()
    assert conv._L.m2s_last_lod_frustum_counts(conv._h, two) == 0 and list(two) == [sel["visible_leaves"], sel["culled"]]
    assert conv.num_stored == len(sel["nodes"])
    if len(sel["nodes"]):
        ids = conv.download_lod_nodes()
        assert ids.dtype == np.uint32 and np.array_equal(ids, sel["nodes"])
        assert np.array_equal(bits(conv.download()), bits(tree[ids]))
    else:
        assert conv.device_lod_nodes == 0 and conv.download().shape == (0, 24)
    tally(tree, b, first, frustum, depth, bias, vis, sel)
    return sel


def check_select(conv, tree, parent, b, first, frustum, occ, vis, visf, cam, tau):
    depth, bias, occ_c = occ
    got = conv.lod_select(cam, FOCAL, tau, NEAR, frustum=fc(frustum), occluder=occ_c)
    return got, check_cut(conv, tree, parent, b, first, frustum, depth, bias, vis, visf, cam, tau, got)


def check_budget(conv, ref, tree, parent, b, first, frustum, occ, LHvis, visf, cam, budget, tau_min):
    depth, bias, occ_c = occ
    L, Hh, vis = LHvis
    want = oc.search(L, Hh, first, vis, budget, tau_min)
    got = conv.lod_select_budget(cam, FOCAL, budget, tau_min, NEAR, frustum=fc(frustum), occluder=occ_c)
    print(f"lod occluded budget nodes={first[-1]} guard={frustum[3]} budget={budget} floor={tau_min}: {got} want key {want['key']:#x}")
    assert br.key_of(got["tau_px"]) == want["key"] and got["met"] == want["met"] and got["selected_finer"] == want["selected_finer"]
    assert got["selected"] == want["selected"]
    sel = check_cut(conv, tree, parent, b, first, frustum, depth, bias, vis, visf, cam, want["tau_px"], got)
    assert np.array_equal(sel["nodes"], np.flatnonzero(br.flags_at(L, Hh, want["key"])))
    if ref is not None:                                                              # the returned tau on a second context: the same bytes
        other = ref.lod_select(cam, FOCAL, got["tau_px"], NEAR, frustum=fc(frustum), occluder=occ_c)
        assert other == {k: got[k] for k in other}
        assert ref.num_stored == conv.num_stored and np.array_equal(bits(ref.download()), bits(conv.download()))
        if conv.num_stored:
            assert np.array_equal(ref.download_lod_nodes(), conv.download_lod_nodes())
    return got


def occluder_for(tree, b, first, frustum, seed, bias=oc.BIAS, sprinkle=True):
    depth = oc.median_depth_image(b, tree[:, 7], first, frustum, W, H, bias, rng=np.random.default_rng(seed) if sprinkle else None)
    return depth, bias, lod.occluder_to_c(depth, bias)


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257, 4099))
def test_occluded_cuts_and_budgets_against_the_restatement(conv, ref, holder, n):
    rec = with_alphas(special_records(n, n))
    on_device = 0
    for levels in CHAINS:
        for max_group in (2, 64):
            for unsigned in (False, True):
                conv.upload_records(rec)
                out = conv.lod_build(levels, max_group, 0.5, unsigned_axis=unsigned)
                ref.upload_records(rec)
                assert ref.lod_build(levels, max_group, 0.5, unsigned_axis=unsigned) == out
                tree, parent, b, first = download_tree(conv)
                for ci, (frustum, cam) in enumerate(cameras(b, first)):
                    bias = oc.BIAS if ci != 3 else 0.0
                    occ = occluder_for(tree, b, first, frustum, 100 * n + ci, bias)
                    if ci == 1 and not on_device:                                    # once per n: the same image as a device pointer
                        holder.upload_records(occ[0].reshape(-1, 24))                 # (64 x 36 floats are 96 records: a third context keeps the bytes)
                        assert np.array_equal(bits(holder.download()), bits(occ[0].reshape(-1, 24)))
                        occ = (occ[0], bias, lod.occluder_on_device(holder.device_records, W, H, bias))
                        on_device += 1
                    L, Hh, _, vis = oc.intervals(b, tree[:, 7], parent, first, cam, FOCAL, NEAR, frustum, occ[0], bias)
                    visf = fr.visibility(b, parent, first, frustum)
                    ends = br.endpoints(L, Hh)
                    for key in sorted({0, ends[len(ends) // 2], ends[-1]}):
                        check_select(conv, tree, parent, b, first, frustum, occ, vis, visf, cam, br.tau_of(key))
                    for budget in oc.budgets(L, Hh, first, vis):
                        check_budget(conv, ref, tree, parent, b, first, frustum, occ, (L, Hh, vis), visf, cam, budget, 0.0)
                    check_budget(conv, ref, tree, parent, b, first, frustum, occ, (L, Hh, vis), visf, cam, max(1, first[-1] // 2), 2.0)
    assert on_device == 1


def opaque_tree(conv, n=600, seed=21, levels=(3, 6, 10), min_scale=0.0, alphas=False):
    """records without a NaN position whose alpha is 1 (alphas: every third takes one of ALPHAS)"""
    rec = mr.crafted_records(n, seed, invalid=False)
    rec[:, 8:10] = np.maximum(rec[:, 8:10], F(min_scale))
    rec[:, 7] = 1.0
    conv.upload_records(with_alphas(rec) if alphas else rec)
    conv.lod_build(levels, 4, 0.5, unsigned_axis=True)
    return download_tree(conv)


def test_an_image_of_ones_gives_the_frustum_cut_and_an_image_of_zeros_nothing(conv, ref):
    tree, parent, b, first = opaque_tree(conv)
    ref.upload_records(tree[:first[1]])
    ref.lod_build((3, 6, 10), 4, 0.5, unsigned_axis=True)
    frustum, cam = cameras(b, first)[0]                                              # far: every leaf lies well past the near plane
    visf = fr.visibility(b, parent, first, frustum)
    assert 0 < visf[:first[1]].sum()
    ones = (np.ones((H, W), F), oc.BIAS, lod.occluder_to_c(np.ones((H, W), F)))
    for tau in (0.0, 1.0, 8.0):
        got, _ = check_select(conv, tree, parent, b, first, frustum, ones, visf, visf, cam, tau)
        other = ref.lod_select(cam, FOCAL, tau, NEAR, frustum=fc(frustum))
        assert other == {k: got[k] for k in other} and got["occluded_leaves"] == 0 == got["translucent_kept"]
        assert np.array_equal(bits(ref.download()), bits(conv.download())) and np.array_equal(ref.download_lod_nodes(), conv.download_lod_nodes())
    gb = conv.lod_select_budget(cam, FOCAL, 50, near=NEAR, frustum=fc(frustum), occluder=ones[2])
    ob = ref.lod_select_budget(cam, FOCAL, 50, near=NEAR, frustum=fc(frustum))
    assert ob == {k: gb[k] for k in ob} and np.array_equal(bits(ref.download()), bits(conv.download()))
    # every alpha 1 behind an image of zeros: no leaf is inside (my > 2e-5 for everything past the near plane)
    zeros = (np.zeros((H, W), F), oc.BIAS, lod.occluder_to_c(np.zeros((H, W), F)))
    L, Hh, _, vis = oc.intervals(b, tree[:, 7], parent, first, cam, FOCAL, NEAR, frustum, zeros[0])
    assert not vis.any()
    got, _ = check_select(conv, tree, parent, b, first, frustum, zeros, vis, visf, cam, 1.0)
    plain = lr.select(b, parent, first, cam, FOCAL, 1.0, NEAR)
    assert got["selected"] == 0 and got["per_level"] == [0] * (len(first) - 1) and got["visible_leaves"] == got["occluded_leaves"] == int(visf[:first[1]].sum())
    assert got["culled"] == plain["counts"]["selected"] and got["refine"] == plain["counts"]["refine"] and got["translucent_kept"] == 0
    assert conv.num_stored == 0 and conv.device_lod_nodes == 0 and len(conv.download_lod_nodes()) == 0
    for tau_min, key in ((0.0, 0), (2.0, br.key_of(2.0))):
        got = check_budget(conv, None, tree, parent, b, first, frustum, zeros, (L, Hh, vis), visf, cam, 10, tau_min)
        assert (br.key_of(got["tau_px"]), got["selected"], got["met"], got["selected_finer"]) == (key, 0, True, 0) and conv.num_stored == 0
    after = conv.lod_select(cam, FOCAL, 1.0, NEAR)                                   # the tree is whole: the plain cut works
    assert {k: after[k] for k in lod.SELECT_COUNTS} == plain["counts"] and set(after) == set(lod.SELECT_COUNTS) | {"per_level"}
    assert np.array_equal(conv.download_lod_nodes(), plain["nodes"]) and np.array_equal(bits(conv.download()), bits(tree[plain["nodes"]]))
    fa = conv.lod_select(cam, FOCAL, 1.0, NEAR, frustum=fc(frustum))                 # ... and the frustum cut keeps its field set
    assert set(fa) == set(lod.SELECT_COUNTS) | {"per_level", "visible_leaves", "culled"}


def test_a_tree_of_one_level_and_more_nodes_than_the_sweeps_lanes(conv):
    rec = mr.crafted_records(700, 4, invalid=False)
    rec[:, 0:3] = np.random.default_rng(4).normal(0, 1, (700, 3)).astype(F)          # no two in one place: level 0 merges nothing
    conv.upload_records(with_alphas(rec))
    assert conv.lod_build((0,), 4, 0.5)["levels"] == 1
    tree, parent, b, first = download_tree(conv)
    frustum, cam = cameras(b, first)[2]
    occ = occluder_for(tree, b, first, frustum, 9)
    L, Hh, _, vis = oc.intervals(b, tree[:, 7], parent, first, cam, FOCAL, NEAR, frustum, occ[0])
    visf = fr.visibility(b, parent, first, frustum)
    assert 0 < vis.sum() < visf.sum() < len(vis)
    check_select(conv, tree, parent, b, first, frustum, occ, vis, visf, cam, 1.0)
    got = check_budget(conv, None, tree, parent, b, first, frustum, occ, (L, Hh, vis), visf, cam, 1, 0.0)
    assert got["selected"] == int(vis.sum()) and not got["met"]
    n = 300003
    rng = np.random.default_rng(5)
    base = mr.crafted_records(4099, 77)
    rec = base[rng.integers(0, len(base), n)]
    rec[:, 0:3] = rng.normal(0, 1, (n, 3)).astype(F)
    rec[:, 7] = 1.0
    conv.upload_records(with_alphas(rec))
    out = conv.lod_build(tuple(range(1, 11)), 4, -2.0, unsigned_axis=True)
    assert out["levels"] >= 4 and out["nodes"] > 1024 * 256
    tree, parent, b, first = download_tree(conv)
    frustum, cam = (EYE, camera.look_at((0.3, -0.2, 0.1), (2.0, 1.0, -1.0)), PROJ, 1.05), (0.3, -0.2, 0.1)
    occ = occluder_for(tree, b, first, frustum, 10)
    L, Hh, _, vis = oc.intervals(b, tree[:, 7], parent, first, cam, FOCAL, NEAR, frustum, occ[0])
    visf = fr.visibility(b, parent, first, frustum)
    got, sel = check_select(conv, tree, parent, b, first, frustum, occ, vis, visf, cam, 1.5)
    assert sum(1 for v in got["per_level"] if v) >= 2 and got["occluded_leaves"] > 1000 and got["translucent_kept"] > 0
    got = check_budget(conv, None, tree, parent, b, first, frustum, occ, (L, Hh, vis), visf, cam, 20000, 0.0)
    wide = conv.lod_select_budget(cam, FOCAL, 20000, near=NEAR, dry_run=True, frustum=fc(frustum))
    print(f"300 003 leaves, budget 20 000: tau {got['tau_px']} behind the occluder, {wide['tau_px']} over the frustum")
    assert got["met"] and br.key_of(got["tau_px"]) <= br.key_of(wide["tau_px"])       # never coarser: vis is a subset of the frustum's


def test_dry_runs_change_nothing(conv):
    tree, parent, b, first = opaque_tree(conv, 300, 11, alphas=True)
    rec2 = mr.crafted_records(50, 3)
    conv.upload_records(rec2)                                                        # the tree survives other records
    ptr, n2 = conv.device_records, conv.num_stored
    frustum, cam = cameras(b, first)[2]
    occ = occluder_for(tree, b, first, frustum, 12)
    L, Hh, _, vis = oc.intervals(b, tree[:, 7], parent, first, cam, FOCAL, NEAR, frustum, occ[0])
    want = oc.select(b, tree[:, 7], parent, first, cam, FOCAL, 1.0, NEAR, frustum, occ[0], vis=vis)
    dry = conv.lod_select(cam, FOCAL, 1.0, NEAR, dry_run=True, frustum=fc(frustum), occluder=occ[2])
    assert {k: dry[k] for k in lod.SELECT_COUNTS} == want["counts"] and dry["per_level"] == want["per_level"]
    assert {k: dry[k] for k in lod.OCCLUSION_COUNTS} == {k: want[k] for k in lod.OCCLUSION_COUNTS} == conv.last_lod_occlusion_counts()
    assert want["occluded_leaves"] > 0
    budget = max(1, want["counts"]["selected"] // 2)
    bw = oc.search(L, Hh, first, vis, budget)
    dryb = conv.lod_select_budget(cam, FOCAL, budget, near=NEAR, dry_run=True, frustum=fc(frustum), occluder=occ[2])
    assert br.key_of(dryb["tau_px"]) == bw["key"] and dryb["selected"] == bw["selected"] and dryb["selected_finer"] == bw["selected_finer"]
    assert conv.device_records == ptr and conv.num_stored == n2 and np.array_equal(bits(conv.download()), bits(rec2)) and conv.device_lod_nodes == 0
    with pytest.raises(M2SError):
        conv.download_lod_nodes()
    real = conv.lod_select_budget(cam, FOCAL, budget, near=NEAR, frustum=fc(frustum), occluder=occ[2])
    assert real == dryb
    ids, out = conv.download_lod_nodes(), bits(conv.download()).copy()
    assert conv.lod_select_budget(cam, FOCAL, budget, near=NEAR, frustum=fc(frustum), occluder=occ[2]) == real   # again: the same result and bytes
    assert np.array_equal(conv.download_lod_nodes(), ids) and np.array_equal(bits(conv.download()), out)
    for x, y in zip(download_tree(conv)[:3], (tree, parent, b)):                     # the tree is untouched
        assert np.array_equal(bits(x), bits(y))


def test_the_frame_after_the_occluded_cut_is_the_depth_tested_frame_after_the_plain_cut(conv):
    """tau 0 (leaves only), guard 1.05, bias 2e-5: the prepass without a depth test after the occluded cut draws the quads, byte for
    byte, that the prepass with the depth test and the same image draws after the plain cut"""
    tree, parent, b, first = opaque_tree(conv, 3000, 8, (2, 4, 6, 10), min_scale=1e-3, alphas=True)
    frames = 0
    for ci, (frustum, cam) in enumerate(cameras(b, first)):
        if frustum[3] != 1.05:
            continue
        occ = occluder_for(tree, b, first, frustum, 40 + ci)
        pp = PrepassParams(view_mat=frustum[1], proj_mat=PROJ, model_mat=frustum[0], renderer_resolution=(1280, 720), resolution_target=1)
        got = conv.lod_select(cam, FOCAL, 0.0, NEAR, frustum=fc(frustum), occluder=occ[2])
        assert got["selected"] == got["selected_leaves"] == got["visible_leaves"] - got["occluded_leaves"]
        ids = conv.download_lod_nodes() if got["selected"] else np.zeros(0, np.uint32)
        vis_o, quads_o, depths_o = conv.prepass(pp)
        plain = conv.lod_select(cam, FOCAL, 0.0, NEAR)
        assert plain["selected"] == first[1]
        vis_p, quads_p, depths_p = conv.prepass(replace(pp, perform_mesh_depth_test=True, mesh_depth=occ[0]))
        print(f"frame test camera {ci}: {got}, {vis_o} quads after the occluded cut, {vis_p} depth-tested after the plain cut")
        assert vis_o == vis_p and np.array_equal(bits(quads_o), bits(quads_p)) and np.array_equal(bits(depths_o), bits(depths_p))
        assert vis_o <= len(ids)
        frames += got["occluded_leaves"] > 0 and vis_o > 0
    assert frames >= 2


def test_the_sh_plane_is_carried_through_an_occluded_cut(hiplib):
    c = Converter(0)
    try:
        c.carry_sh = True
        rec = mr.crafted_records(500, 6, invalid=False)
        rec[:, 7] = 1.0
        sh = ms.random_plane(500, 6)
        c.upload_records(rec)
        c.upload_sh(sh, 3)
        out = c.lod_build((3, 6, 10), 4, 0.5)
        plane, deg = c.download_lod_sh()
        assert deg == 3 and plane.shape == (out["nodes"], 48)
        tree, parent, b, first = download_tree(c)
        frustum, cam = cameras(b, first)[2]
        occ = occluder_for(tree, b, first, frustum, 60)
        got = c.lod_select(cam, FOCAL, 2.0, NEAR, frustum=fc(frustum), occluder=occ[2])
        want = oc.select(b, tree[:, 7], parent, first, cam, FOCAL, 2.0, NEAR, frustum, occ[0])
        assert got["selected"] == len(want["nodes"]) > 0 and got["occluded_leaves"] == want["occluded_leaves"] > 0
        ids = c.download_lod_nodes()
        assert np.array_equal(ids, want["nodes"]) and c.sh_plane_info() == {"rows": len(ids), "degree": 3}
        assert np.array_equal(bits(c.download_sh()), bits(plane[ids]))
    finally:
        c.close()


def test_the_context_s_mesh_depth_image_as_occluder(hiplib):
    """a converted sphere seen from outside: the far half is occluded by the mesh itself, and the budget buys a cut no coarser"""
    c = Converter(0)
    try:
        Wm, Hm = 160, 90
        c.upload_scene(synth.cube_sphere(12, tex_size=32))
        assert c.convert(32) > 500
        c.to_world_units()
        c.lod_build((4, 5, 6, 7), 4, 0.5, unsigned_axis=True)
        proj = camera.perspective(60.0, Wm / Hm, 0.1, 50.0)
        eye = (0.3, 0.4, 2.6)
        view = camera.look_at(eye, (0, 0, 0))
        pp = PrepassParams(view_mat=view, proj_mat=proj, renderer_resolution=(Wm, Hm), near_plane=0.1, far_plane=50.0, resolution_target=1)
        cam, focal = lod.camera_position(view), lod.focal_px(proj, Hm)
        frustum = lod.frustum_of(pp)
        with pytest.raises(M2SError):                                                # no image yet
            c.lod_select(cam, focal, 1.0, 0.1, frustum=frustum, occluder=lod.occluder_of_mesh_depth(c))
        img, _ = c.mesh_depth(pp)
        o = lod.occluder_of_mesh_depth(c)
        got = c.lod_select(cam, focal, 1.0, 0.1, dry_run=True, frustum=frustum, occluder=o)
        tree, parent, b, first = download_tree(c)
        want = oc.select(b, tree[:, 7], parent, first, cam, focal, 1.0, 0.1, (pp.model_mat, view, proj, 1.05), img)
        print(f"sphere behind its own depth image: {got}")
        assert {k: got[k] for k in lod.OCCLUSION_COUNTS} == {k: want[k] for k in lod.OCCLUSION_COUNTS} and got["selected"] == want["counts"]["selected"]
        assert got["occluded_leaves"] > 0 and got["visible_leaves"] > got["occluded_leaves"]
        budget = max(1, got["visible_leaves"] // 8)
        fb = c.lod_select_budget(cam, focal, budget, near=0.1, dry_run=True, frustum=frustum)
        ob = c.lod_select_budget(cam, focal, budget, near=0.1, dry_run=True, frustum=frustum, occluder=o)
        assert br.key_of(ob["tau_px"]) <= br.key_of(fb["tau_px"])
        sized = lod.occluder_of_mesh_depth(c)
        sized.depth_w, sized.depth_h = Wm, Hm
        assert c.lod_select(cam, focal, 1.0, 0.1, dry_run=True, frustum=frustum, occluder=sized) == got
        sized.depth_h = Hm + 1
        with pytest.raises(M2SError):
            c.lod_select(cam, focal, 1.0, 0.1, dry_run=True, frustum=frustum, occluder=sized)
    finally:
        c.close()


def test_stage_time_with_profiling(conv):
    tree, parent, b, first = opaque_tree(conv, 4099, 2)
    frustum, cam = cameras(b, first)[2]
    occ = occluder_for(tree, b, first, frustum, 70)
    conv.set_profiling(True)
    try:
        conv.lod_select(cam, FOCAL, 1.0, NEAR, frustum=fc(frustum), occluder=occ[2])
        a = conv.last_lod_frustum_ms()
        conv.lod_select_budget(cam, FOCAL, 1000, near=NEAR, frustum=fc(frustum), occluder=occ[2])
        print(f"lod occluded visibility stage, 4 099 leaves: {a} ms, {conv.last_lod_frustum_ms()} ms in front of the budget search")
        assert a > 0 and conv.last_lod_frustum_ms() > 0
    finally:
        conv.set_profiling(False)


def test_errors(hiplib):
    c = Converter(0)
    try:
        out = (C.c_uint64 * 4)()
        res = lod.LodBudgetResultC()
        nan, inf = float("nan"), float("inf")
        f = lod.frustum_to_c(EYE, camera.look_at((0, 0, 5), (0, 0, 0)), PROJ)
        img = np.ones((4, 4), F)

        def occluder(**kw):
            o = lod.occluder_to_c(img)
            for name, v in kw.items():
                if name == "reserved":
                    o.reserved[v[0]] = v[1]
                else:
                    setattr(o, name, v)
            return o

        def select(o, fr_=f, cam=(0.0, 0.0, 5.0), focal=500.0, tau=1.0, near=0.1, flags=0):
            p = lod.select_to_c(cam, focal, tau, near)
            p.flags = flags
            return hiplib.m2s_lod_select_occluded(c._h, C.byref(p), C.byref(fr_) if fr_ is not None else None, C.byref(o) if o is not None else None, out)

        def budget(o, fr_=f, cam=(0.0, 0.0, 5.0), focal=500.0, n=10, tau_min=0.0, near=0.1, flags=0):
            p = lod.budget_to_c(cam, focal, n, tau_min, near)
            p.flags = flags
            return hiplib.m2s_lod_select_budget_occluded(c._h, C.byref(p), C.byref(fr_) if fr_ is not None else None, C.byref(o) if o is not None else None,
                                                         C.byref(res), out)

        assert select(occluder()) == 7 and budget(occluder()) == 7                   # no tree
        rec = mr.crafted_records(40, 1, invalid=False)
        c.upload_records(rec)
        c.lod_build((3, 10), 4, 0.5)
        before = c.download()
        for call in (select, budget):
            assert call(None) == 1 and call(occluder(), fr_=None) == 1
            for bad in (dict(depth_bias=nan), dict(depth_bias=inf), dict(depth_bias=-1e-9), dict(reserved=(0, 1)), dict(reserved=(1, 7)),
                        dict(depth_w=0), dict(depth_h=0)):
                assert call(occluder(**bad)) == 1, bad
            assert call(occluder(depth=None, depth_w=0, depth_h=0)) == 7             # NULL image and no m2s_mesh_depth has run
            assert call(occluder(depth=None)) == 7                                   # (a size is compared once there is an image)
            # the errors of the frustum forms and of the plain functions
            bad_f = lod.frustum_to_c(EYE, EYE, PROJ, 0.5)
            assert call(occluder(), fr_=bad_f) == 1
            for bad in (dict(cam=(nan, 0, 0)), dict(focal=0.0), dict(focal=inf), dict(near=0.0), dict(near=nan), dict(flags=2)):
                assert call(occluder(), **bad) == 1, bad
        assert select(occluder(), tau=-1.0) == 1 and select(occluder(), tau=nan) == 1
        assert budget(occluder(), n=0) == 1 and budget(occluder(), tau_min=-1.0) == 1
        assert hiplib.m2s_lod_select_occluded(c._h, None, C.byref(f), C.byref(occluder()), None) == 1
        assert np.array_equal(bits(c.download()), bits(before))
        assert select(occluder(depth_bias=0.0), flags=1) == 0 and np.array_equal(bits(c.download()), bits(before))
        four = (C.c_uint64 * 4)()
        assert hiplib.m2s_last_lod_occlusion_counts(c._h, four) == 0 and hiplib.m2s_last_lod_occlusion_counts(c._h, None) == 1
        p = lod.budget_to_c((0.0, 0.0, 5.0), 500.0, 10, near=0.1)
        o = occluder()
        assert hiplib.m2s_lod_select_budget_occluded(c._h, C.byref(p), C.byref(f), C.byref(o), None, None) == 0   # (both outputs may be NULL)
        with pytest.raises(ValueError):
            c.lod_select((0, 0, 5), 500.0, occluder=o)
        # an empty tree: the floor, met, nothing selected, nothing inside, no image read
        c.upload_records(np.zeros((0, 24), F))
        c.lod_build((1,))
        got = c.lod_select_budget((0, 0, 0), 500.0, 5, tau_min_px=2.0, frustum=f, occluder=occluder())
        assert got == {"nodes": 0, "selected": 0, "selected_leaves": 0, "refine": 0, "per_level": [0], "tau_px": 2.0, "met": True, "selected_finer": 0,
                       "visible_leaves": 0, "culled": 0, "occluded_leaves": 0, "translucent_kept": 0}
        assert c.lod_select((0, 0, 0), 500.0, frustum=f, occluder=occluder())["selected"] == 0 and c.num_stored == 0
        c.lod_release()
        assert select(occluder()) == 7 and budget(occluder()) == 7
    finally:
        c.close()


def test_zz_the_cases_exercise_every_class():
    """Runs last in this module: over the cuts above some cameras saw a part of their leaves behind the image and some all of them;
    translucent leaves behind it were kept; a leaf's depth met its texel plus the bias exactly; texel indices were clamped under the
    guard band of 4; leaves at NaN were inside; nodes above the leaves were dropped with every leaf below them occluded while their
    own position passes the test."""
    print(f"lod occlusion, over the module: {SEEN}")
    assert SEEN["cuts"] > 1000 and all(v > 0 for v in SEEN.values()), SEEN
