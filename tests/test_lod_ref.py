"""CPU: the restatement of the level-of-detail cut (tests/lod_ref.py) against cases derived by hand, the property every cut must have, the
parameter structs against the C compiler's layout, and the entry points' NULL checks (no device needed)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import lod_ref as lr
import merge_ref as mr
from mesh2splat_amd import lod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def grid_tree():
    """merge_ref.grid_records(8) through merges at levels 8, 9, 10: a perfect quadtree of 64 / 16 / 4 / 1 nodes, edges 0.125 .. 1.0"""
    rec = mr.grid_records(8)
    levels, maps = [rec], []
    for lv in (8, 9, 10):
        out, mp, _, _ = mr.merge(levels[-1], lv, 4, 0.5)
        levels.append(out)
        maps.append(mp)
    counts = [len(v) for v in levels]
    assert counts == [64, 16, 4, 1]
    parent, first = lr.link(maps, counts)
    b = lr.bounds(np.concatenate(levels))
    for l, e in enumerate((0.125, 0.25, 0.5, 1.0)):
        assert (b[first[l]:first[l + 1], 3] == F(e)).all()
    assert np.array_equal(b[-1, 0:3], np.array([0.5, 0.5, 0.0], F))
    return b, parent, first


@pytest.mark.parametrize("D, want, level", ((100, 64, 0), (200, 16, 1), (300, 4, 2), (512, 1, 3), (511, 4, 2)))
def test_grid_quadtree_table(grid_tree, D, want, level):
    """focal 512, tau 1, camera above the centre: level l (edge 2^l / 8) refines iff (64 * 2^l)^2 > d2.  All operands are dyadic: at
    D = 200 the leaves' parents are 200.0x away (d2 up to 40000.03 > 16384), at D = 512 the root has s^2 == d2 and equality does not
    refine, at D = 511 it does and its children (256^2 = 65536 against more than 261121) do not."""
    b, parent, first = grid_tree
    sel = lr.select(b, parent, first, (0.5, 0.5, float(D)), 512.0, 1.0, 1.0)
    assert sel["counts"]["selected"] == want
    assert sel["per_level"] == [want if l == level else 0 for l in range(4)]
    assert lr.cut_ok(parent, first, sel["flags"])


def test_tau_zero_gives_the_leaves_and_a_huge_tau_the_top_level(grid_tree):
    b, parent, first = grid_tree
    for cam in ((0.5, 0.5, 3.0), (10.0, -4.0, 0.0), (0.0625, 0.0625, 0.0)):
        lo = lr.select(b, parent, first, cam, 512.0, 0.0, 1.0)
        assert lo["per_level"] == [64, 0, 0, 0] and lo["counts"]["refine"] == 85     # (s^2 > 0 for every node)
        hi = lr.select(b, parent, first, cam, 512.0, 1e9, 1.0)
        assert hi["per_level"] == [0, 0, 0, 1] and hi["counts"]["refine"] == 0


def test_a_node_without_extent_or_with_a_nan_never_refines(grid_tree):
    b, parent, first = grid_tree
    for e in (0.0, np.nan):
        c = b.copy()
        c[first[3], 3] = e                                                           # the root
        sel = lr.select(c, parent, first, (0.5, 0.5, 0.5), 512.0, 0.0, 1e-3)
        assert sel["per_level"] == [0, 0, 0, 1] and not sel["refine"][first[3]] and sel["counts"]["refine"] == 84
    c = b.copy()
    c[first[3], 0] = np.nan                                                          # a NaN position counts as `near` away
    assert lr.select(c, parent, first, (0.5, 0.5, 1e6), 512.0, 1.0, 1.0)["refine"][first[3]]
    assert not lr.select(c, parent, first, (0.5, 0.5, 1e6), 512.0, 1.0, 1024.0)["refine"][first[3]]
    c[first[3], 0:3] = np.inf                                                        # an infinite distance: inf on the right, never below it
    assert not lr.select(c, parent, first, (0.5, 0.5, 0.5), 512.0, 1.0, 1.0)["refine"][first[3]]


def random_tree(rng):
    levels = int(rng.integers(2, 6))
    counts = [int(rng.integers(20, 60))]
    for _ in range(levels - 1):
        counts.append(max(1, int(counts[-1] * rng.uniform(0.3, 0.9))))
    maps = [np.sort(np.concatenate([np.arange(counts[l + 1]), rng.integers(0, counts[l + 1], counts[l] - counts[l + 1])])).astype(np.uint32)
            for l in range(levels - 1)]
    parent, first = lr.link(maps, counts)
    b = np.empty((first[-1], 4), F)
    b[:, 0:3] = rng.normal(0, 1, (first[-1], 3))
    b[:, 3] = np.exp(rng.normal(-2, 1.5, first[-1])) * (rng.random(first[-1]) > 0.1)   # sizes that go up and down along a chain
    b[first[-2] + int(rng.integers(0, counts[-1])), 3] = 0                            # one node of the last level never refines
    return b, parent, first


def test_every_leaf_is_covered_exactly_once_on_random_trees():
    rng = np.random.default_rng(19)
    mixed = 0
    for _ in range(200):
        b, parent, first = random_tree(rng)
        cam = rng.normal(0, 2, 3)
        sel = lr.select(b, parent, first, cam, float(rng.uniform(50, 2000)), float(rng.choice([0.0, 0.5, 1.0, 4.0, 30.0])), 0.05)
        assert lr.cut_ok(parent, first, sel["flags"])
        assert sum(sel["per_level"]) == sel["counts"]["selected"] == len(sel["nodes"])
        # the gating: a node fine enough itself below an ancestor that does not refine is not selected
        g = lr.gated(parent, first, sel)
        assert g.size and not sel["open"][parent[g]].any()
        mixed += sum(1 for v in sel["per_level"] if v) >= 2
        # ... and selecting every fine-enough node instead would draw leaves twice
        naive = ~sel["refine"]
        naive[:first[1]] = True
        assert not lr.cut_ok(parent, first, naive)
    assert mixed > 100


def test_cut_ok_notices_holes_and_doubles(grid_tree):
    b, parent, first = grid_tree
    sel = lr.select(b, parent, first, (0.5, 0.5, 200.0), 512.0, 1.0, 1.0)["flags"]
    assert lr.cut_ok(parent, first, sel)
    hole, double = sel.copy(), sel.copy()
    hole[np.flatnonzero(sel)[0]] = False
    double[0] = True
    assert not lr.cut_ok(parent, first, hole) and not lr.cut_ok(parent, first, double)


def test_camera_helpers():
    from mesh2splat_amd.score import camera_from_eye
    cam = camera_from_eye((1.5, -2.25, 3.0), (0.1, 0.2, 0.3), 0.1, 100.0, 1920, 1080)
    eye = lod.camera_position(cam.view_mat)
    assert np.abs(np.array(eye) - np.array(cam.eye)).max() < 1e-6
    assert eye == tuple(float(F(v)) for v in eye)                                    # float32 values
    f = lod.focal_px(cam.proj_mat, 1080)
    assert f == float(F(cam.proj_mat.reshape(-1)[5] * F(1080)) / F(2)) and abs(f - 540 / np.tan(np.pi / 8)) < 1e-3


def test_struct_layouts_match_the_header(tmp_path):
    assert C.sizeof(lod.LodBuildParamsC) == 80 and C.sizeof(lod.LodSelectParamsC) == 32
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    fields = {"m2s_lod_build_params": [f[0] for f in lod.LodBuildParamsC._fields_], "m2s_lod_select_params": [f[0] for f in lod.LodSelectParamsC._fields_]}
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "m2s.h"\nint main(void){\n'
                   'printf("%zu %zu %d %u\\n", sizeof(m2s_lod_build_params), sizeof(m2s_lod_select_params), M2S_LOD_MAX_STEPS, M2S_LOD_NO_PARENT);\n' +
                   "".join('printf("%%zu\\n", offsetof(%s, %s));\n' % (s, f) for s, fs in fields.items() for f in fs) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out[:4]] == [80, 32, lod.MAX_STEPS, lod.NO_PARENT]
    want = [getattr(lod.LodBuildParamsC, f).offset for f in fields["m2s_lod_build_params"]] + \
           [getattr(lod.LodSelectParamsC, f).offset for f in fields["m2s_lod_select_params"]]
    assert [int(v) for v in out[4:]] == want


def test_null_contexts(hiplib):
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    bp, sp = lod.build_to_c((1, 2)), lod.select_to_c((0, 0, 0), 500.0)
    assert hiplib.m2s_lod_build(None, C.byref(bp), out) == 1 and list(out) == [0, 0, 0, 0]
    out[:] = (7, 7, 7, 7)
    assert hiplib.m2s_lod_select(None, C.byref(sp), out) == 1 and list(out) == [0, 0, 0, 0]
    n, first = C.c_uint32(9), (C.c_uint64 * 18)()
    assert hiplib.m2s_lod_levels(None, C.byref(n), first) == 1 and n.value == 0
    assert hiplib.m2s_download_lod(None, 0, None, 0) == 1 and hiplib.m2s_lod_release(None) == 1
    assert hiplib.m2s_device_lod(None, 0) is None and hiplib.m2s_device_lod_nodes(None) is None
    assert hiplib.m2s_last_lod_build_ms(None) == 0.0
    assert hiplib.m2s_last_lod_level_counts(None, None) == 1 and hiplib.m2s_last_lod_select_stage_ms(None, None) == 1
    k = C.c_uint64(5)
    assert hiplib.m2s_download_lod_nodes(None, None, 0, C.byref(k)) == 1 and k.value == 0
    with pytest.raises(ValueError):
        lod.build_to_c(range(17))
