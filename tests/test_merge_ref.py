"""CPU: the numpy restatement of the merge pass (tests/merge_ref.py) against what can be known without it — the axes of a conversion's
records, the tiling property, an L of three tiles in closed form, passthrough, the colour rule — and the symbols, the struct layout and
the NULL handling of m2s_merge (no compute calls)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import compact_ref as cr
import merge_ref as mr
import pyref
from mesh2splat_amd import _lib
from mesh2splat_amd.merge import COUNTS, DRY_RUN, MergeParamsC, to_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("m2s_merge", "m2s_last_merge_counts", "m2s_last_merge_stage_ms", "m2s_device_merge_map", "m2s_download_merge_map")
F = np.float32


def test_symbols_exported(hiplib):
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(hiplib, name), name


def test_ctypes_mirror_layout():
    assert C.sizeof(MergeParamsC) == 24 and [getattr(MergeParamsC, f).offset for f, _ in MergeParamsC._fields_] == [0, 4, 8, 12, 16]
    assert COUNTS == mr.COUNTS and DRY_RUN == 1
    p = to_c(3, dry_run=True)
    assert (p.level, p.max_group, p.min_axis_dot, p.flags, list(p.reserved)) == (3, 4, 0.5, 1, [0, 0])


def test_struct_layout_matches_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    fields = ("level", "max_group", "min_axis_dot", "flags", "reserved")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "m2s.h"\nint main(void){printf("%zu ' + "%zu " * len(fields) + '%d\\n", '
                   "sizeof(m2s_merge_params), " + ", ".join(f"offsetof(m2s_merge_params, {f})" for f in fields) +
                   ", (int)M2S_MERGE_DRY_RUN);return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(MergeParamsC)] + [getattr(MergeParamsC, f).offset for f in fields] + [1] and out[0] == 24


def test_null_context(hiplib):
    mp = to_c(0)
    out4, out3, words, n = (C.c_uint64 * 4)(), (C.c_float * 3)(), (C.c_uint32 * 1)(), C.c_uint64()
    assert hiplib.m2s_merge(None, C.byref(mp), out4) == 1
    assert hiplib.m2s_last_merge_counts(None, out4) == 1 and hiplib.m2s_last_merge_stage_ms(None, out3) == 1
    assert not hiplib.m2s_device_merge_map(None)
    assert hiplib.m2s_download_merge_map(None, words, 1, C.byref(n)) == 1


# ---- the axis reading ------------------------------------------------------------------------------------------------------------
def _flat_triangles():
    """three triangles in general position, vertex normals = the face normal: rows of 12 floats (position, normal, tangent, uv)"""
    tris = [((0.1, 0.2, 0.3), (0.9, 0.25, 0.4), (0.3, 0.8, 0.2)), ((0.2, 0.1, 0.1), (0.25, 0.9, 0.5), (0.3, 0.2, 0.95)),
            ((0.8, 0.1, 0.2), (0.1, 0.15, 0.9), (0.7, 0.85, 0.6))]
    verts = np.zeros((9, 12), F)
    for t, tri in enumerate(tris):
        p = np.array(tri, np.float64)
        nrm = np.cross(p[1] - p[0], p[2] - p[0])
        verts[3 * t:3 * t + 3, 0:3] = p
        verts[3 * t:3 * t + 3, 3:6] = nrm / np.linalg.norm(nrm)
    return verts


def test_axes_of_conversion_records_are_the_viewers_rows():
    """For records the conversion emits, r_3 (third row of castQuatToMat3 of the stored floats) is the triangle's normal and r_1 its
    longest edge — the x axis the geometry stage hands quat_cast — with r_2 = r_3 x r_1: the rows, not the columns.  (Scale is
    (|Ju|, |Jv|), the UV Jacobian's columns, which run along r_1, r_2 only where the longest edge lies along the projection's u axis.)"""
    verts = _flat_triangles()
    rec = pyref.convert_untextured(verts, (0, 0, 0), (1, 1, 1), (1, 1, 1, 1), 24)
    assert len(rec) > 60
    r1, r2, r3 = mr.rows_f64(rec[:, 16:20])
    seen = set()
    for i in range(len(rec)):
        nrm = rec[i, 12:15].astype(np.float64)
        t = int(np.argmax([abs(nrm @ verts[3 * k, 3:6]) for k in range(3)]))
        seen.add(t)
        p = verts[3 * t:3 * t + 3, 0:3].astype(np.float64)
        edges = [p[1] - p[0], p[2] - p[0], p[2] - p[1]]
        xa = max(edges, key=lambda e: e @ e)
        xa = xa / np.linalg.norm(xa)
        assert abs(abs(r3[i] @ nrm) - 1) < 1e-5 and abs(abs(r1[i] @ xa) - 1) < 1e-5
        assert np.abs(np.cross(r3[i], r1[i]) - r2[i]).max() < 1e-5
        # ... and the columns are NOT those: the transposed reading fails on a rotation in general position
        cols = np.stack([r1[i], r2[i], r3[i]], 0).T
        assert abs(abs(cols[2] @ nrm) - 1) > 1e-3
        # the viewer's covariance is sum s_i^2 r_i r_i^T: flat along the normal
        assert abs(nrm @ mr.viewer_cov(rec[i]) @ nrm) < 1e-12
    assert seen == {0, 1, 2}


# ---- the tiling property -----------------------------------------------------------------------------------------------------------
def test_grid_cells_are_what_the_pin_says():
    rec = mr.grid_records(8)
    p = rec[:, 0:3]
    assert cr.omin(p)[0] == F(1 / 16) and cr.omax(p)[0] == F(15 / 16)
    ext = F(15 / 16) - F(1 / 16)
    cells = np.floor(((rec[:8, 0] - F(1 / 16)) / ext) * F(1024)).clip(0, 1023).astype(int)
    assert list(cells) == [0, 146, 292, 438, 585, 731, 877, 1023]
    assert list(cells >> 8) == [0, 0, 1, 1, 2, 2, 3, 3]


def test_two_by_two_blocks_give_the_record_of_half_the_density():
    rec = mr.grid_records(8)
    out, mp, counts, info = mr.merge(rec, 8, 4, 0.5)
    assert counts == {"before": 64, "after": 16, "merged": 16, "invalid": 0}
    iy, ix = np.divmod(np.arange(64), 8)
    block = (iy // 2) * 4 + ix // 2
    # the map sends the four tiles of a block, and nothing else, to one parent
    assert all(np.unique(mp[block == b]).size == 1 for b in range(16)) and np.unique(mp).size == 16
    for b in range(16):
        s = mp[block == b][0]
        members = rec[block == b]
        assert np.allclose(out[s, 0:2], ((b % 4) * 0.25 + 0.125, (b // 4) * 0.25 + 0.125), atol=1e-7) and out[s, 2] == 0 and out[s, 3] == 1
        assert out[s, 8] == F(0.25) and out[s, 9] == F(0.25) and out[s, 10] == F(1e-7)
        assert np.allclose(mr.viewer_cov(out[s]), np.diag([0.0625, 0.0625, 1e-14]), atol=1e-9)
        assert np.allclose(out[s, 4:7], members[:, 4:7].mean(0), atol=1e-7) and out[s, 7] == 1
        assert tuple(out[s, 12:15]) == (0, 0, 1) and np.allclose(out[s, 20:24], (0.1, 0.5, 0, 1))
        assert abs(np.linalg.norm(out[s, 16:20]) - 1) < 1e-6 and out[s, 16] >= 0
    # a level finer pairs nothing across the cell boundaries of 2^7: fewer merges; a level coarser still cuts at max_group
    assert mr.merge(rec, 10, 4, 0.5)[2]["after"] == 16
    assert mr.merge(rec, 0, 4, 0.5)[2]["after"] == 64


def test_counts_are_monotone_in_level():
    rec = cr.hostile(cr.make_records(700, 5))
    for g, dot in ((2, -2.0), (4, 0.5), (64, 0.0)):
        after = [mr.merge(rec, lv, g, dot)[2]["after"] for lv in range(11)]
        assert all(a >= b for a, b in zip(after, after[1:])), after
        assert after[0] > after[-1]


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
def _tile(x, y, h=1.0, colour=(0.2, 0.4, 0.6), alpha=1.0):
    r = np.zeros(24, F)
    r[0:4] = (x, y, 0, 1)
    r[4:8] = (*colour, alpha)
    r[8:12] = (h, h, 1e-7, 0)
    r[12:16] = (0, 0, 1, 0)
    r[16] = 1
    r[20:24] = (0.1, 0.5, 0, 1)
    return r


def test_l_shape_against_its_analytic_second_moment():
    """three unit tiles at (0.5, 0.5), (1.5, 0.5), (0.5, 1.5): M = [[11/36, -1/9], [-1/9, 11/36]], eigenvalues 15/36 along (1, -1) and
    7/36 along (1, 1): edges sqrt(5) and sqrt(7/3)"""
    L = np.stack([_tile(0.5, 0.5), _tile(1.5, 0.5), _tile(0.5, 1.5)])
    out, info = mr.parent(L)
    assert np.allclose(info["M"][:2, :2], [[11 / 36, -1 / 9], [-1 / 9, 11 / 36]], atol=1e-15) and np.abs(info["M"][2]).max() == 0
    assert np.allclose(out[0:3], (5 / 6, 5 / 6, 0), atol=1e-7)
    assert out[8] == F(np.sqrt(5.0)) and out[9] == F(np.sqrt(7.0 / 3.0))
    assert abs(abs(info["e1"] @ np.array([1, -1, 0]) / np.sqrt(2)) - 1) < 1e-12
    want = 12 * np.array([[11 / 36, -1 / 9, 0], [-1 / 9, 11 / 36, 0], [0, 0, 0]])
    assert np.abs(mr.viewer_cov(out) - want).max() < 1e-5 * 5
    # through merge(): one run, one segment whatever the order, because the centroid and the moment are symmetric in the members
    out2, mp, counts, _ = mr.merge(L, 10, 64, -2.0)
    assert counts == {"before": 3, "after": 1, "merged": 1, "invalid": 0} and list(mp) == [0, 0, 0]
    assert np.allclose(out2[0, 8:10], out[8:10], rtol=1e-6) and np.allclose(out2[0, 0:3], out[0:3], atol=1e-6)


def test_singletons_and_invalid_records_pass_through():
    rec = cr.make_records(40, 3)
    rec[:, 0:3] = np.arange(40, dtype=F)[:, None] * F(10.0)           # far apart: every record is alone in its cell at level 0
    rec[7, 0] = np.nan
    rec[20, 16:20] = 0
    rec[33, 9] = -1
    out, mp, counts, info = mr.merge(rec, 0, 4, -2.0)
    assert counts == {"before": 40, "after": 40, "merged": 0, "invalid": 3} and all(i is None for i in info)
    assert np.array_equal(out[mp].view(np.uint32), rec.view(np.uint32))
    assert list(mp[[7, 20, 33]]) == [37, 38, 39]                      # behind every valid record, in index order
    # at the coarsest level everything valid merges, and the invalid ones are still three untouched records at the end
    out, mp, counts, info = mr.merge(rec, 10, 64, -2.0)
    assert counts == {"before": 40, "after": 4, "merged": 1, "invalid": 3}
    assert np.array_equal(out[1:].view(np.uint32), rec[[7, 20, 33]].view(np.uint32))


def test_colour_rule_with_a_zero_alpha_member():
    a, b = _tile(0.5, 0.5, colour=(1, 0, 0), alpha=0.0), _tile(1.5, 0.5, colour=(0, 0, 1), alpha=0.5)
    out, _ = mr.parent(np.stack([a, b]))
    assert tuple(out[4:7]) == (0, 0, 1) and out[7] == F(0.25)         # the transparent member does not tint the parent
    b[7] = 0
    out, _ = mr.parent(np.stack([a, b]))
    assert tuple(out[4:8]) == (0.5, 0, 0.5, 0)                        # nothing opaque: the plain weighted mean
    # weights are areas: a tile of twice the edge counts four times
    big = _tile(0.0, 0.0, h=2.0, colour=(1, 1, 1), alpha=1.0)
    out, _ = mr.parent(np.stack([big, _tile(3.0, 0.0, colour=(0, 0, 0), alpha=1.0)]))
    assert np.allclose(out[4:7], 0.8) and np.allclose(out[0], 0.6)
    # no area at all: every member weighs 1
    z0, z1 = _tile(0.0, 0.0, h=0.0), _tile(2.0, 0.0, h=0.0)
    out, info = mr.parent(np.stack([z0, z1]))
    assert out[0] == 1 and out[8] == F(np.sqrt(12.0)) and out[9] == 0
