"""-m gpu: the SH plane of the level-of-detail tree and of its cuts (pins 4s and 3s of include/m2s.h; Converter.carry_sh,
.download_lod_sh) against the same merges run one by one on a second context and against the tree's own rows.  Everything is compared
for equality: a level's plane byte for byte, a cut's plane = the tree's rows at the selected node indices.  What a merge does to a plane
is tests/test_gpu_merge_sh.py's business; the cuts themselves are tests/test_gpu_lod*.py's."""
import ctypes as C

import numpy as np
import pytest

import camera
import lod_ref as lr
import merge_ref as mr
import merge_sh_ref as ms
from mesh2splat_amd import lod, synth
from mesh2splat_amd._lib import M2SError
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.score import orbit_cameras

pytestmark = pytest.mark.gpu
F = np.float32
FOCAL, NEAR = 600.0, 0.05
PROJ = camera.perspective(45.0, 16 / 9, 0.01, 100.0)
EYE = np.eye(4, dtype=F)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    c.carry_sh = True
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(hiplib):
    c = Converter(0)
    c.carry_sh = True
    yield c
    c.close()


def build(conv, rec, sh, levels, max_group=4, dot=0.5, degree=3):
    conv.carry_sh = True
    conv.upload_records(rec)
    conv.upload_sh(sh, degree)
    out = conv.lod_build(levels, max_group, dot)
    plane, deg = conv.download_lod_sh()
    assert deg == degree and plane.shape == (out["nodes"], 48) and conv.device_lod_sh
    return out, conv.download_lod(0), conv.download_lod(1), conv.download_lod(2), plane


def levels_one_by_one(ref, rec, sh, levels, max_group, dot):
    """the steps as single merges with the switch on, on another context -> the planes of the tree levels"""
    ref.carry_sh = True
    ref.upload_records(rec)
    ref.upload_sh(sh)
    planes = [sh]
    for lv in levels:
        before = ref.num_stored
        if ref.merge_count(lv, max_group, dot) == before:                            # (a step that merges nothing is not applied)
            continue
        ref.merge(lv, max_group, dot)
        planes.append(ref.download_sh())
    return planes


def check_cut(conv, tree, plane, want_nodes):
    ids = conv.download_lod_nodes()
    assert np.array_equal(ids, want_nodes) and conv.num_stored == len(ids)
    assert np.array_equal(bits(conv.download()), bits(tree[ids]))
    assert conv.sh_plane_info()["rows"] == len(ids)
    got = conv.download_sh()
    assert got.shape == (len(ids), 48) and np.array_equal(bits(got), bits(plane[ids]))
    return ids


@pytest.mark.parametrize("n,levels,max_group,dot", ((300, (3, 10), 4, 0.5), (300, (0, 3, 3, 10), 5, 0.5), (700, (0,), 4, 0.5)))
def test_tree_planes_and_the_four_cuts(conv, ref, n, levels, max_group, dot):
    rec = mr.crafted_records(n, 11 if n == 300 else 4, invalid=(n == 300))
    if n == 700:
        rec[:, 0:3] = np.random.default_rng(4).normal(0, 1, (n, 3)).astype(F)        # no two in one place: a tree of one level
    sh = ms.random_plane(n, n)
    out, tree, parent, b, plane = build(conv, rec, sh, levels, max_group, dot, degree=2)
    first = out["first"]
    want = levels_one_by_one(ref, rec, sh, levels, max_group, dot)
    assert len(want) == out["levels"] and (out["levels"] == 1) == (n == 700)
    for l, w in enumerate(want):
        assert np.array_equal(bits(plane[first[l]:first[l + 1]]), bits(w)), ("level", l)
    # the context's plane afterwards: the last level's, or untouched where no step merged
    assert conv.sh_plane_info() == {"rows": len(want[-1]), "degree": 2} and np.array_equal(bits(conv.download_sh()), bits(want[-1]))
    leaves = b[:first[1], 0:3].astype(np.float64)
    ok = np.isfinite(leaves).all(1)
    ctr = leaves[ok].mean(0)
    eye = leaves[ok][ok.sum() // 2] + 0.02
    cam = tuple(float(F(v)) for v in eye)
    frustum = lod.frustum_to_c(EYE, camera.look_at(eye, ctr), PROJ, 1.05)
    for tau in (0.0, 0.5, 4.0, 1e9):
        sel = lr.select(b, parent, first, cam, FOCAL, tau, NEAR)
        conv.upload_records(rec)                                                     # (other records, no plane: the tree's property decides)
        conv.carry_sh = False
        assert conv.lod_select(cam, FOCAL, tau, NEAR)["selected"] == sel["counts"]["selected"]
        conv.carry_sh = True
        check_cut(conv, tree, plane, sel["nodes"])
        assert conv.sh_plane_info()["degree"] == 2
        got = conv.lod_select(cam, FOCAL, tau, NEAR, frustum=frustum)
        ids = check_cut(conv, tree, plane, conv.download_lod_nodes())
        assert got["selected"] == len(ids) <= sel["counts"]["selected"] and np.isin(ids, sel["nodes"]).all()
    for budget in (1, max(1, first[1] // 3), first[-1]):
        got = conv.lod_select_budget(cam, FOCAL, budget, near=NEAR)
        sel = lr.select(b, parent, first, cam, FOCAL, got["tau_px"], NEAR)
        check_cut(conv, tree, plane, sel["nodes"])
        got = conv.lod_select_budget(cam, FOCAL, budget, near=NEAR, frustum=frustum)
        ids = check_cut(conv, tree, plane, conv.download_lod_nodes())
        assert got["selected"] == len(ids)


def test_a_tree_with_a_plane_that_outgrows_its_first_reservation(ref):
    """The twin of tests/test_gpu_lod.py's case with the switch on, on a fresh context: 1031 leaves under the chain 1..10 in pairs, 8921
    nodes against a first reservation of 1546 — the four planes grow three times, each time with the rows written so far kept.  The
    tree's plane against tests/merge_sh_ref.py's chain by that file's comparison, and against the single merges byte for byte."""
    n, levels = 1031, tuple(range(1, 11))
    rec = mr.crafted_records(n, n)
    sh = ms.random_plane(n, n)
    recs, planes, wparent, wfirst = ms.chain(rec, sh, levels, 2, 0.5)
    assert len(recs) == len(levels) + 1                                              # (every step merges: step s made level s + 1)
    conv = Converter(0)
    try:
        out, tree, parent, b, plane = build(conv, rec, sh, levels, 2, 0.5)
        first = out["first"]
        print(f"lod build with a plane n={n} chain={levels} group=2 dot=0.5 on a fresh context: {out}")
        assert out["nodes"] > n + n // 2
        assert out["nodes"] == 8921 and first == wfirst and np.array_equal(parent, wparent)
        assert np.array_equal(bits(plane[:n]), bits(sh))
        for s, lv in enumerate(levels):
            perm, heads = ms.heads_of(recs[s], lv, 2, 0.5)
            wplane, pinfo = ms.merge_plane(recs[s], planes[s], perm, heads)
            assert np.array_equal(bits(wplane), bits(planes[s + 1]))
            ulps = ms.compare(plane[first[s + 1]:first[s + 2]], planes[s + 1], pinfo)
            print(f"  level {s + 1}: plane within {ulps:.4f} ulp of max|sh|")
            assert ulps <= ms.PLANE_ULPS_BAR
        want = levels_one_by_one(ref, rec, sh, levels, 2, 0.5)
        assert len(want) == out["levels"]
        for l, w in enumerate(want):
            assert np.array_equal(bits(plane[first[l]:first[l + 1]]), bits(w)), ("level", l)
        cam = (0.4, 0.1, -0.3)
        conv.lod_select(cam, FOCAL, 0.5, NEAR)
        check_cut(conv, tree, plane, lr.select(b, parent, first, cam, FOCAL, 0.5, NEAR)["nodes"])
    finally:
        conv.close()


def test_nothing_inside_gives_an_empty_plane_and_a_plain_cut_follows(conv):
    rec = mr.crafted_records(600, 21, invalid=False)
    sh = ms.random_plane(600, 21)
    out, tree, parent, b, plane = build(conv, rec, sh, (3, 6, 10))
    first = out["first"]
    leaves = b[:first[1], 0:3].astype(np.float64)
    ctr = leaves.mean(0)
    far = ctr + np.array([0.3, 0.2, 1.0]) * 6.0 * max(float(np.linalg.norm(leaves - ctr, axis=1).max()), 0.5)
    cam = tuple(float(F(v)) for v in far)
    away = lod.frustum_to_c(EYE, camera.look_at(far, far + (far - ctr)), PROJ, 1.05)
    got = conv.lod_select(cam, FOCAL, 1.0, NEAR, frustum=away)
    assert got["selected"] == 0 and conv.num_stored == 0
    assert conv.sh_plane_info() == {"rows": 0, "degree": 3} and conv.download_sh().shape == (0, 48)
    sel = lr.select(b, parent, first, cam, FOCAL, 1.0, NEAR)
    conv.lod_select(cam, FOCAL, 1.0, NEAR)
    check_cut(conv, tree, plane, sel["nodes"])


def test_a_dry_run_leaves_the_plane(conv):
    rec = mr.crafted_records(300, 11)
    sh = ms.random_plane(300, 11)
    out, tree, parent, b, plane = build(conv, rec, sh, (3, 10))
    conv.upload_records(rec)
    conv.upload_sh(sh, 1)
    ptr = conv.device_records
    cam = (0.4, 0.1, -0.3)
    dry = conv.lod_select(cam, FOCAL, 0.5, NEAR, dry_run=True)
    assert dry["selected"] > 0 and conv.device_records == ptr and conv.num_stored == 300
    assert conv.sh_plane_info() == {"rows": 300, "degree": 1} and np.array_equal(bits(conv.download_sh()), bits(sh))
    conv.lod_select_budget(cam, FOCAL, 50, near=NEAR, dry_run=True)
    assert conv.sh_plane_info() == {"rows": 300, "degree": 1} and np.array_equal(bits(conv.download_sh()), bits(sh))
    conv.lod_select(cam, FOCAL, 0.5, NEAR)
    assert conv.sh_plane_info()["degree"] == 3                                       # the tree's


def test_a_tree_built_with_the_switch_off_has_no_plane_and_release_then_a_second_build(conv, hiplib):
    rec = mr.crafted_records(300, 11)
    sh = ms.random_plane(300, 11)
    for why in ("off", "no plane"):
        conv.carry_sh = why != "off"
        conv.upload_records(rec)
        if why == "off":
            conv.upload_sh(sh)
        out = conv.lod_build((3, 10), 4, 0.5)
        assert out["levels"] == 3 and conv.device_lod_sh == 0 and conv.device_sh == 0   # (the merges dropped the context's plane, as ever)
        deg = C.c_uint32(9)
        buf = np.empty((out["nodes"], 48), F)
        assert hiplib.m2s_download_lod_sh(conv._h, buf.ctypes.data, out["nodes"], C.byref(deg)) == 7 and deg.value == 0
        with pytest.raises(M2SError):
            conv.download_lod_sh()
        conv.carry_sh = True                                                         # ... whatever the switch says at the time of the cut
        conv.upload_records(rec)
        conv.upload_sh(sh)
        tree, parent, b = conv.download_lod(0), conv.download_lod(1), conv.download_lod(2)
        sel = lr.select(b, parent, out["first"], (0.4, 0.1, -0.3), FOCAL, 0.5, NEAR)
        conv.lod_select((0.4, 0.1, -0.3), FOCAL, 0.5, NEAR)
        assert np.array_equal(conv.download_lod_nodes(), sel["nodes"]) and np.array_equal(bits(conv.download()), bits(tree[sel["nodes"]]))
        assert conv.device_sh == 0                                                   # the context's plane is dropped as today
        with pytest.raises(M2SError):
            conv.sh_plane_info()
    out, tree, parent, b, plane = build(conv, rec, sh, (3, 10))
    small = np.empty((1, 48), F)
    assert hiplib.m2s_download_lod_sh(conv._h, small.ctypes.data, out["nodes"] - 1, None) == 5
    assert hiplib.m2s_download_lod_sh(conv._h, None, out["nodes"], None) == 1
    conv.lod_release()
    assert conv.device_lod_sh == 0 and hiplib.m2s_download_lod_sh(conv._h, small.ctypes.data, 1, None) == 7
    out2, _, _, _, plane2 = build(conv, rec, sh, (3, 10))
    assert out2 == out and np.array_equal(bits(plane2), bits(plane))
    conv.upload_records(np.zeros((0, 24), F))                                        # an empty tree with a plane: no device pointer, an empty cut
    conv.upload_sh(np.zeros((0, 48), F))
    assert conv.lod_build((1,))["nodes"] == 0 and conv.device_lod_sh == 0 and conv.download_lod_sh()[0].shape == (0, 48)
    assert conv.lod_select((0, 0, 0), 500.0)["selected"] == 0 and conv.sh_plane_info()["rows"] == 0


def test_more_than_one_workgroup_per_level(conv, ref):
    """300 003 leaves under the chain 1..10: every level's plane against the single merges, a cut of several levels against the tree's rows"""
    n = 300003
    rng = np.random.default_rng(5)
    base = mr.crafted_records(4099, 77)
    rec = base[rng.integers(0, len(base), n)]
    rec[:, 0:3] = rng.normal(0, 1, (n, 3)).astype(F)
    sh = ms.random_plane(n, 5)
    levels = tuple(range(1, 11))
    out, tree, parent, b, plane = build(conv, rec, sh, levels, 4, -2.0)
    first = out["first"]
    assert out["levels"] >= 4 and np.array_equal(bits(plane[:n]), bits(sh))
    want = levels_one_by_one(ref, rec, sh, levels, 4, -2.0)
    assert len(want) == out["levels"]
    for l, w in enumerate(want):
        assert np.array_equal(bits(plane[first[l]:first[l + 1]]), bits(w)), ("level", l)
    for cam, tau in (((0.3, -0.2, 0.1), 1.0), ((4.0, 3.0, 5.0), 8.0)):
        sel = lr.select(b, parent, first, cam, FOCAL, tau, NEAR)
        conv.lod_select(cam, FOCAL, tau, NEAR)
        check_cut(conv, tree, plane, sel["nodes"])
        assert sum(1 for v in sel["per_level"] if v) >= 2


def test_render_baked_after_a_cut(conv, ref):
    """the unit quad at R = 64, baked, a tree with the plane, the cut of tests/test_gpu_lod.py's frame test (tau_px = 75 goes through
    the middle of the tree): render_baked runs on the cut and equals render_baked of the same records and plane uploaded elsewhere"""
    scene = synth.unit_quad()
    conv.carry_sh = True
    conv.upload_scene(scene)
    n = conv.convert(64)
    cam = orbit_cameras(scene, 1, 160, 120)[0]
    pp, lp = cam.frame_params(64, (1.0, 2.0, 3.0), 30.0, shadow_resolution=128)
    conv.bake_light(BakeParams(n_theta=4, n_phi=8, use_shadows=False), lp, download=False)
    out = conv.lod_build(unsigned_axis=True)
    assert out["leaves"] == n and out["levels"] > 2 and conv.download_lod_sh()[1] == 3
    eye, focal = lod.camera_position(cam.view_mat), lod.focal_px(cam.proj_mat, 120)
    cut = conv.lod_select(eye, focal, 75.0, cam.near)
    assert 0 < cut["selected"] < n and sum(1 for v in cut["per_level"] if v) >= 2
    rec, sh = conv.download(), conv.download_sh()
    assert np.array_equal(bits(sh), bits(conv.download_lod_sh()[0][conv.download_lod_nodes()]))
    a = np.array(conv.render_baked(pp), copy=True)
    assert a.any()
    ref.upload_records(rec)
    ref.upload_sh(sh)
    b = np.array(ref.render_baked(pp), copy=True)
    assert np.array_equal(a, b)
