"""CPU: what M2S_MERGE_UNSIGNED_AXIS is for, shown with the oracle and the restatements (tests/merge_unsigned_ref.py on top of
merge_ref.py, lod_ref.py, worldunits_ref.py).  A conversion stores the two triangles of a flat quad with third rows +n and -n (the viewer's
covariance does not see the sign), pin 2 breaks a run on every seam between them, and the hierarchy stops getting coarser (DESIGN 5.18,
5.19).  With the sign ignored (pins 2u, 5u) the oracle's unit quad becomes the quadtree the merge pass was built for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lod_ref as lr
import merge_ref as mr
import merge_unsigned_ref as mu
import worldunits_ref as wr
from mesh2splat_amd import lod, merge, synth
from test_worldunits_ref import CAMERAS, CHAIN, FOCAL, TAUS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
R = 64


def longest(level):
    return lr.bounds(level)[:, 3]


def flipped_grid(k=8):
    """merge_ref.grid_records(k) with every other record turned half a turn about r_1: stored (0, 1, 0, 0), r_1 = +x, r_2 = -y, r_3 = -z;
    the viewer's covariance is the same"""
    rec = mr.grid_records(k)
    rec[1::2, 16:20] = (0, 1, 0, 0)
    return rec


@pytest.fixture(scope="module")
def quad_world(oracle):
    total, rec, _ = oracle.convert(synth.unit_quad(), R)
    assert total == len(rec) == R * R
    return wr.to_world_units(np.ascontiguousarray(rec, F), R)


@pytest.fixture(scope="module")
def quad_tree(quad_world):
    return mu.chain(quad_world, CHAIN)


def test_the_quads_two_triangles_store_opposite_third_rows(quad_world):
    """the cause: half the records' r_3 points against the normal, triangle by triangle"""
    r3 = mr.rows_f64(quad_world[:, 16:20])[2]
    against = (r3 * quad_world[:, 12:15]).sum(1) < 0
    print("unit quad at R = 64: records with r_3 against the normal:", int(against.sum()), "of", len(r3))
    # (one triangle of the two, and the texels of the diagonal go to one of them: half the records and at most a row more)
    assert np.allclose(np.abs(r3[:, 2]), 1, atol=1e-6) and R * R // 2 - R <= int(against.sum()) <= R * R // 2 + R
    stored = {tuple(np.round(q, 5)) for q in quad_world[:, 16:20].astype(np.float64)}
    print("stored rotations of the quad:", sorted(stored))
    assert len(stored) == 2


def test_quad_chain_is_a_quadtree_with_the_sign_ignored(quad_world, quad_tree):
    levels, parent, first = quad_tree
    signed = [len(v) for v in mu.chain(quad_world, CHAIN, merge_fn=mr.merge)[0]]
    print("quad, signed:  ", signed)
    print("quad, unsigned:", [len(v) for v in levels])
    assert signed == [4096, 1088, 352, 176, 136, 128, 127]
    assert [len(v) for v in levels] == [4096, 1024, 256, 64, 16, 4, 1]
    h = F(1) / F(R)
    worst = 0.0
    for k, lv in enumerate(levels):
        want = F(2 ** k) * h
        e = longest(lv).astype(np.float64)
        worst = max(worst, float(np.abs(e - float(want)).max() / float(np.spacing(want))))
        assert np.abs(e - float(want)).max() <= mr.SCALAR_ULPS_GUARD * float(np.spacing(want)), k
        # both edges: the parents are squares
        assert np.abs(lv[:, 8:10].astype(np.float64) - float(want)).max() <= mr.SCALAR_ULPS_GUARD * float(np.spacing(want)), k
    print("quad, largest deviation of a longest edge from 2^k h, in fp32 ulps:", worst)
    assert (longest(levels[1]) == F(2) * h).all() and (longest(levels[2]) == F(4) * h).all()      # dyadic operands: equality
    assert float(longest(levels[-1])[0]) == pytest.approx(1.0, abs=4 * float(np.spacing(F(1))))


def test_flipped_grid_merges_only_with_the_sign_ignored():
    rec = flipped_grid(8)
    for a, b in zip(rec, mr.grid_records(8)):
        assert np.allclose(mr.viewer_cov(a), mr.viewer_cov(b), atol=0, rtol=0)
    assert [mr.merge(rec, lv)[2]["after"] for lv in (8, 9, 10)] == [64, 64, 64]
    levels, parent, first = mu.chain(rec, (8, 9, 10))
    assert [len(v) for v in levels] == [64, 16, 4, 1]
    assert [len(v) for v in mu.chain(rec, (8, 9, 10), merge_fn=mr.merge)[0]] == [64]
    top = levels[-1][0]
    assert top[8] == top[9] == F(1) and np.array_equal(top[0:3], np.array([0.5, 0.5, 0], F))
    # the parent lies on its first member's side, level after level
    for lv in levels[1:]:
        assert np.array_equal(mr.rows_f64(lv[:, 16:20])[2], np.tile([0.0, 0.0, 1.0], (len(lv), 1)))


def test_cube_sphere_half_the_axes_point_inwards_and_the_chain_gets_coarse(oracle):
    total, rec, _ = oracle.convert(synth.cube_sphere(8), 128)
    rec = wr.to_world_units(np.ascontiguousarray(rec, F), 128)
    r3 = mr.rows_f64(rec[:, 16:20])[2]
    against = (r3 * rec[:, 12:15]).sum(1) < 0
    print("cube_sphere(8) at R = 128:", len(rec), "records,", int(against.sum()), "with r_3 against the normal")
    assert len(rec) == 42600 and 2 * int(against.sum()) == len(rec)
    levels = (3, 4, 5, 6, 7, 8, 9, 10)
    signed = [len(v) for v in mu.chain(rec, levels, merge_fn=mr.merge)[0]]
    unsigned_levels = mu.chain(rec, levels)[0]
    unsigned = [len(v) for v in unsigned_levels]
    print("cube_sphere(8), chain (3 .. 10), signed:  ", signed)
    print("cube_sphere(8), chain (3 .. 10), unsigned:", unsigned)
    print("cube_sphere(8), unsigned, median longest edge per level:", [float(np.median(longest(v))) for v in unsigned_levels])
    assert 4 * unsigned[-1] <= signed[-1]


def _record(pos, r3, scale=(0.1, 0.1)):
    """a record at pos whose third row is the unit vector r3 (any in-plane turn)"""
    r3 = np.asarray(r3, np.float64)
    helper = np.array([1.0, 0, 0]) if abs(r3[0]) < 0.9 else np.array([0, 1.0, 0])
    e1 = np.cross(r3, helper)
    e1 /= np.linalg.norm(e1)
    rec = np.zeros(24, F)
    rec[0:3], rec[3] = pos, 1
    rec[4:8] = (0.5, 0.5, 0.5, 1)
    rec[8:11] = (scale[0], scale[1], 1e-7)
    rec[12:15] = r3
    rec[16:20] = mr.quat_cast_wxyz(e1, np.cross(r3, e1), r3)
    return rec


def test_a_pair_of_opposite_sign_on_a_curved_patch_gets_the_oriented_mean():
    a = np.array([0.0, 0.0, 1.0])
    b = np.array([np.sin(0.2), 0.0, np.cos(0.2)])
    members = np.stack([_record((0, 0, 0), a), _record((0.01, 0, 0), -b)])
    r3 = mr.rows_f64(members[:, 16:20])[2]
    assert r3[0] @ r3[1] < -0.9
    o, flipped = mu.orient(r3)
    assert list(flipped) == [False, True]
    want = (o[0] + o[1]) / np.linalg.norm(o[0] + o[1])
    got = mu.parent(members)[1]["nb"]
    assert np.abs(got - want).max() <= 4 * np.finfo(np.float64).eps
    assert got @ np.array([np.sin(0.1), 0, np.cos(0.1)]) > 1 - 1e-6                  # the bisector of the two oriented normals
    # the signed pin sums +a and -b: along their difference, at right angles to the surface normal
    signed = mr.parent(members)[1]["nb"]
    assert abs(signed @ want) < 0.01
    # ... and the stored parent has the oriented mean as its third row, on the first member's side
    out = mu.parent(members)[0]
    assert mr.rows_f64(out[16:20])[2] @ want > 1 - 1e-6 and mr.rows_f64(out[16:20])[2] @ a > 0


def test_a_zero_dot_and_a_nan_do_not_flip():
    z, x = np.array([0.0, 0, 1]), np.array([1.0, 0, 0])
    o, flipped = mu.orient(np.stack([z, x, -x, -z]))
    assert list(flipped) == [False, False, True, False]                               # 0 against z; -1 against o_1 = x; 0 against o_2 = x
    assert np.array_equal(o, np.stack([z, x, x, -z]))
    nan = np.array([np.nan, 0, 1])
    o, flipped = mu.orient(np.stack([z, nan, -z]))
    assert not flipped.any() and np.array_equal(o[2], -z)                             # a NaN does not flip, nor does the member behind it
    # in a parent: members +z, +x, -x.  The zero dot leaves +x, -x is turned: nb is the normalised z + 2 x, not z
    members = np.stack([_record((0, 0, 0), z), _record((0.01, 0, 0), x), _record((0.02, 0, 0), -x)])
    out, info = mu.parent(members)
    assert list(info["flipped"]) == [False, False, True]
    assert np.abs(info["nb"] - np.array([2, 0, 1]) / np.sqrt(5)).max() < 1e-6         # (the stored quaternions are fp32)
    assert np.abs(mr.parent(members)[1]["nb"] - z).max() < 1e-6                       # signed: +x and -x cancel


def test_a_nan_dot_breaks_the_run_and_no_threshold_below_zero_does():
    """two valid records of one cell whose fp32 third rows are finite and whose dot is inf - inf"""
    z, x = np.array([0.0, 0, 1]), np.array([1.0, 0, 0])
    rec = np.stack([_record((0, 0, 0), z), _record((1e-4, 0, 0), z)])
    s = F(3e9)
    rec[0, 16:20] = (s, s, s, s)          # r_3 = (4 s^2, 0, 1 - 4 s^2) = (3.6e19, 0, -3.6e19)
    rec[1, 16:20] = (-s, s, s, -s)        # r_3 = (-4 s^2, 0, 1 - 4 s^2)
    perm, keys = mr.order(rec)
    assert (keys != mr.INVALID_KEY).all()
    a = mr.axis3_f32(rec[perm][:, 16:20])
    with np.errstate(all="ignore"):
        d = ((a[1, 0] * a[0, 0]) + a[1, 1] * a[0, 1]) + a[1, 2] * a[0, 2]
    assert np.isfinite(a).all() and np.isnan(d)
    for dot in (0.5, 0.0, -2.0):
        assert len(mu.segment_heads(rec, 10, 4, dot)[1]) == 2, dot                    # !(NaN >= t) for every t
    # a number never breaks at min_axis_dot <= 0: |d| >= 0 >= t
    both = np.stack([_record((0, 0, 0), z), _record((1e-4, 0, 0), x), _record((2e-4, 0, 0), -z)])
    assert len(mu.segment_heads(both, 10, 4, 0.0)[1]) == 1 and len(mu.segment_heads(both, 10, 4, -2.0)[1]) == 1
    assert len(mu.segment_heads(both, 10, 4, 0.5)[1]) == 3
    assert len(mu.segment_heads(both[[0, 2]], 10, 4, 0.5)[1]) == 1 and len(mr.segment_heads(both[[0, 2]], 10, 4, 0.5)[1]) == 2


def test_without_a_negative_neighbour_dot_the_bytes_are_merge_refs():
    rng = np.random.default_rng(5)
    rec = mr.crafted_records(600, seed=3)
    ang = rng.uniform(0, 2 * np.pi, len(rec))
    for i in range(len(rec)):
        if np.any(rec[i, 16:20] != 0):                                                # (the crafted zero quaternion stays invalid)
            e1 = np.array([np.cos(ang[i]), np.sin(ang[i]), 0.0])
            rec[i, 16:20] = mr.quat_cast_wxyz(e1, np.cross([0, 0, 1.0], e1), np.array([0, 0, 1.0]))
    for level, g, dot in ((0, 2, 0.5), (3, 5, 0.5), (10, 64, -2.0), (10, 4, 0.5)):
        a, b = mr.merge(rec, level, g, dot), mu.merge(rec, level, g, dot)
        assert a[2] == b[2] and a[2]["merged"] > 0
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        assert not any(i["flipped"].any() for i in b[3] if i is not None)


def test_unsigned_breaks_are_a_subset_so_after_is_never_larger():
    strictly = 0
    for seed in range(200):
        rec = mr.crafted_records(30 + 7 * (seed % 23), seed=seed, invalid=seed % 3 == 0)
        level, g, dot = (0, 3, 10)[seed % 3], (2, 4, 5, 64)[seed % 4], (0.5, -2.0, 0.5, 0.99)[seed % 4]
        ps, hs = mr.segment_heads(rec, level, g, dot)
        pu, hu = mu.segment_heads(rec, level, g, dot)
        assert np.array_equal(ps, pu) and len(hu) <= len(hs), seed
        # the run starts themselves (max_group as large as the input: a segment is a run)
        rs, ru = mr.segment_heads(rec, level, len(rec) + 1, dot)[1], mu.segment_heads(rec, level, len(rec) + 1, dot)[1]
        assert set(ru.tolist()) <= set(rs.tolist()), seed
        strictly += len(hu) < len(hs)
    print("inputs of 200 on which the unsigned rule leaves fewer records:", strictly)
    assert strictly > 0


def test_every_cut_of_the_unsigned_quad_tree_covers_each_leaf_once(quad_tree):
    levels, parent, first = quad_tree
    b = lr.bounds(np.concatenate(levels))
    for cam in CAMERAS:
        for tau in TAUS:
            sel = lr.select(b, parent, first, cam, FOCAL, tau)
            print(f"unsigned quad cam={cam} tau={tau}: per level {sel['per_level']}")
            assert lr.cut_ok(parent, first, sel["flags"])


def test_the_flag_is_bit_2_and_the_words_keep_their_place():
    header = open(os.path.join(ROOT, "include", "m2s.h")).read()
    assert re.search(r"enum \{ M2S_MERGE_DRY_RUN = 1, M2S_MERGE_UNSIGNED_AXIS = 4 \};", header)
    assert merge.DRY_RUN == mu.DRY_RUN == 1 and merge.UNSIGNED_AXIS == lod.UNSIGNED_AXIS == mu.UNSIGNED_AXIS == 4
    assert tuple(merge.VALID_FLAGS) == mu.MERGE_FLAGS_ACCEPTED == (0, 1, 4, 5)
    assert not set(mu.MERGE_FLAGS_ACCEPTED) & set(mu.MERGE_FLAGS_REFUSED) and {2, 3, 6, 8} <= set(mu.MERGE_FLAGS_REFUSED)
    assert mu.BUILD_FLAGS_ACCEPTED == (0, 4) and {1, 2, 3, 5} <= set(mu.BUILD_FLAGS_REFUSED)
    assert [merge.to_c(3, 4, 0.5, d, u).flags for d in (False, True) for u in (False, True)] == [0, 4, 1, 5]
    assert merge.to_c(3).flags == 0 and C.sizeof(merge.MergeParamsC) == 24
    assert C.sizeof(lod.LodBuildParamsC) == 80 and lod.LodBuildParamsC.reserved.offset == 76
    pc = lod.build_to_c((1, 2), 4, 0.5, unsigned_axis=True)
    assert pc.reserved == pc.flags == 4 and lod.build_to_c((1, 2)).reserved == 0
    pc.flags = 0
    assert pc.reserved == 0
    pc.reserved = 4
    assert pc.flags == 4
