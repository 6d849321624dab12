"""-m gpu: M2S_MERGE_UNSIGNED_AXIS (Converter.merge / .lod_build with unsigned_axis=True) against its numpy restatement
(tests/merge_unsigned_ref.py).  Segments, counts and map are exact; the fields lie within merge_ref's guards (4 x what the MI355X achieved
on the signed pass).  The sign decisions of pin 5u are the same fp64 expressions on both sides: a member turned on one side and not on
the other moves the parent's plane by the angle between two crafted axes — a right angle — and fails the covariance comparison, so
no case is exempt.  Then what the mode is for: the flipped grid and the unit quad's conversion as quadtrees."""
import ctypes as C

import numpy as np
import pytest

import camera
import lod_ref as lr
import merge_ref as mr
import merge_unsigned_ref as mu
from mesh2splat_amd import lod, synth
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.merge import MergeParamsC
from mesh2splat_amd.prepass import PrepassParams
from mesh2splat_amd.scene import Mesh, Scene

pytestmark = pytest.mark.gpu
F = np.float32
CHAIN = (4, 5, 6, 7, 8, 9, 10)
FOCAL = 154.51
WORST = {"scalar_ulps": 0.0, "cov_rel": 0.0, "flipped": 0}        # over the whole module: printed and guarded by the last test


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def owner(hiplib):
    c = Converter(0)
    yield c
    c.close()


def check(conv, rec, level, max_group, min_axis_dot, upload=True):
    """merge(unsigned_axis=True) on the device against the restatement -> (records after, map)"""
    want, wmap, wcounts, info = mu.merge(rec, level, max_group, min_axis_dot)
    if upload:
        conv.upload_records(rec)
    dry = conv.merge(level, max_group, min_axis_dot, dry_run=True, unsigned_axis=True)
    assert dry == wcounts, (dry, wcounts)
    assert conv.merge_count(level, max_group, min_axis_dot, unsigned_axis=True) == wcounts["after"]
    got_counts = conv.merge(level, max_group, min_axis_dot, unsigned_axis=True)
    assert got_counts == wcounts == conv.last_merge_counts(), (got_counts, wcounts)
    gmap = conv.download_merge_map()
    assert np.array_equal(gmap, wmap)
    got = conv.download()
    err = mr.compare(got, want, info)
    flipped = sum(int(i["flipped"].sum()) for i in info if i is not None)
    print(f"unsigned merge n={len(rec)} level={level} group={max_group} dot={min_axis_dot}: {wcounts} members turned {flipped}, "
          f"scalar {err['scalar_ulps']:.3f} ulp, cov {err['cov_rel']:.3e}")
    for k in err:
        WORST[k] = max(WORST[k], err[k])
    WORST["flipped"] += flipped
    assert err["scalar_ulps"] <= mr.SCALAR_ULPS_GUARD and err["cov_rel"] <= mr.COV_REL_GUARD, err
    return got, gmap


@pytest.mark.parametrize("level", (0, 3, 10))
@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257, 4099))
def test_fields_against_the_restatement(conv, n, level):
    rec = mr.crafted_records(n, n)
    for max_group in (2, 5, 64):
        for dot in (-2.0, 0.5):
            check(conv, rec, level, max_group, dot)
            signed = mr.segment_heads(rec, level, max_group, dot)[1]
            assert conv.last_merge_counts()["after"] <= len(signed)                  # the breaks are a subset of the signed rule's


def flipped_grid(k=8):
    rec = mr.grid_records(k)
    rec[1::2, 16:20] = (0, 1, 0, 0)                                                  # half a turn about r_1: r_3 = -z, the same covariance
    return rec


def test_flipped_grid_is_a_quadtree_only_with_the_flag(conv):
    rec = flipped_grid(8)
    conv.upload_records(rec)
    assert [conv.merge_count(lv) for lv in (8, 9, 10)] == [64, 64, 64]
    assert conv.lod_build((8, 9, 10), 4, 0.5)["levels"] == 1
    conv.upload_records(rec)
    out = conv.lod_build((8, 9, 10), 4, 0.5, unsigned_axis=True)
    assert list(np.diff(out["first"])) == [64, 16, 4, 1] and out["skipped"] == 0
    tree, first = conv.download_lod(0), out["first"]
    want = mu.chain(rec, (8, 9, 10))[0]
    for l in range(4):
        err = mr.compare(tree[first[l]:first[l + 1]], want[l], [None] * 64 if l == 0 else mu.merge(want[l - 1], 7 + l)[3])
        assert err["scalar_ulps"] <= mr.SCALAR_ULPS_GUARD and err["cov_rel"] <= mr.COV_REL_GUARD
    top = tree[-1]
    assert top[8] == top[9] == F(1) and np.array_equal(top[0:3], np.array([0.5, 0.5, 0], F))
    assert (mr.rows_f64(tree[64:, 16:20])[2] == np.array([0.0, 0.0, 1.0])).all()    # the first member's side, at every level
    conv.lod_release()


def chain_one_by_one(ref, rec, levels, max_group, dot):
    """the steps as single merges with the flag on another context -> (levels' records, the maps between tree levels)"""
    ref.upload_records(rec)
    out, maps, pending = [rec], [], None
    for lv in levels:
        before = ref.num_stored
        after = ref.merge(lv, max_group, dot, unsigned_axis=True)["after"]
        m = ref.download_merge_map()
        m = m if pending is None else m[pending]
        if after == before:
            pending = m
            continue
        pending = None
        maps.append(m)
        out.append(ref.download())
    return out, maps


def frame_of(conv, rec):
    lo, hi = rec[:, 0:3].min(0).astype(np.float64), rec[:, 0:3].max(0).astype(np.float64)
    at = tuple((lo + hi) / 2)
    eye = tuple((lo + hi) / 2 + 1.5 * np.linalg.norm(hi - lo) * np.array([0.5, 0.35, 0.79]))
    pp = PrepassParams(view_mat=camera.look_at(eye, at), proj_mat=camera.perspective(45.0, 16 / 9, 0.01, 100.0), renderer_resolution=(320, 180),
                       resolution_target=conv.resolution)
    vis, quads, depths = conv.prepass(pp)
    assert vis > 0
    return vis, bits(quads).copy(), bits(depths).copy()


def test_the_quads_conversion_is_a_quadtree_with_the_flag(conv, owner):
    R, h = 64, F(1) / F(64)
    conv.upload_scene(synth.unit_quad())
    n = conv.convert(R)
    assert n == R * R
    conv.to_world_units()
    rec = conv.download()
    leaves_frame = frame_of(conv, rec)
    signed = conv.lod_build(CHAIN, 4, 0.5)
    assert list(np.diff(signed["first"])) == [4096, 1088, 352, 176, 136, 128, 127]   # what the sign costs
    assert conv.convert(R) == n and conv.to_world_units()["previous_R"] == R and np.array_equal(bits(conv.download()), bits(rec))
    out = conv.lod_build(CHAIN, 4, 0.5, unsigned_axis=True)
    print(f"unsigned quad: lod build {out}")
    # (the cells of merge level 4 hold one record each at R = 64: that step merges nothing and adds no level, as without the flag)
    assert list(np.diff(out["first"])) == [4096, 1024, 256, 64, 16, 4, 1] and out["skipped"] == 1
    tree, parent, b, first = conv.download_lod(0), conv.download_lod(1), conv.download_lod(2), conv.lod_levels()
    want_levels, maps = chain_one_by_one(owner, rec, CHAIN, 4, 0.5)
    for l, want in enumerate(want_levels):
        assert np.array_equal(bits(tree[first[l]:first[l + 1]]), bits(want)), ("level", l)
    wparent, wfirst = lr.link(maps, [len(v) for v in want_levels])
    assert wfirst == first and np.array_equal(parent, wparent) and np.array_equal(bits(b), bits(lr.bounds(tree)))
    for l in range(len(first) - 1):
        e, want = b[first[l]:first[l + 1], 3].astype(np.float64), float(F(2 ** l) * h)
        print(f"level {l}: {first[l + 1] - first[l]} nodes, longest edge {e.max()!r} .. {e.min()!r} against {want!r}")
        assert np.abs(e - want).max() <= mr.SCALAR_ULPS_GUARD * float(np.spacing(F(want)))
    # cuts: every leaf covered once, equal to the restatement's cut of the device's tree
    for cam in ((0.0, 0.0, 0.3), (0.5, 0.5, 2.0), (0.5, 0.5, 8.0), (-1.0, 0.5, 0.3)):
        for tau in (1.0, 2.0, 4.0):
            want = lr.select(b, parent, first, cam, FOCAL, tau)
            got = conv.lod_select(cam, FOCAL, tau)
            per = got.pop("per_level")
            print(f"unsigned quad cut cam={cam} tau={tau}: per level {per}")
            assert got == want["counts"] and per == want["per_level"] and lr.cut_ok(parent, first, want["flags"])
            assert np.array_equal(conv.download_lod_nodes(), want["nodes"])
    far = conv.lod_select((0.5, 0.5, 8.0), FOCAL, 4.0, dry_run=True)
    assert far["per_level"][3] == far["selected"] == 64                               # a whole level: the signed tree cannot offer one
    # tau_px = 0: the cut is the leaves, and so is its frame, byte for byte
    zero = conv.lod_select((0.5, 0.5, 2.0), FOCAL, 0.0)
    assert zero["selected"] == zero["per_level"][0] == n and np.array_equal(bits(conv.download()), bits(rec))
    cut_frame = frame_of(conv, rec)
    assert cut_frame[0] == leaves_frame[0] and np.array_equal(cut_frame[1], leaves_frame[1]) and np.array_equal(cut_frame[2], leaves_frame[2])
    conv.lod_release()


def test_records_of_one_sign_give_the_same_bytes_with_and_without_the_flag(conv):
    rng = np.random.default_rng(5)
    rec = mr.crafted_records(4099, 3)
    ang = rng.uniform(0, 2 * np.pi, len(rec))
    for i in range(len(rec)):
        if np.any(rec[i, 16:20] != 0):
            e1 = np.array([np.cos(ang[i]), np.sin(ang[i]), 0.0])
            rec[i, 16:20] = mr.quat_cast_wxyz(e1, np.cross([0, 0, 1.0], e1), np.array([0, 0, 1.0]))
    for level, g, dot in ((0, 2, 0.5), (3, 5, 0.5), (10, 64, -2.0)):
        outs = []
        for flag in (False, True):
            conv.upload_records(rec)
            counts = conv.merge(level, g, dot, unsigned_axis=flag)
            outs.append((counts, conv.download(), conv.download_merge_map()))
        assert outs[0][0] == outs[1][0] and outs[0][0]["merged"] > 0
        assert np.array_equal(bits(outs[0][1]), bits(outs[1][1])) and np.array_equal(outs[0][2], outs[1][2])


def test_two_runs_are_identical(conv):
    rec = mr.crafted_records(4099, 21)
    outs = []
    for _ in range(2):
        conv.upload_records(rec)
        conv.merge(3, 5, 0.5, unsigned_axis=True)
        first = (conv.download(), conv.download_merge_map())
        conv.merge(10, 64, -2.0, unsigned_axis=True)                                 # (from the pool, through the staging buffer)
        outs.append((*first, conv.download(), conv.download_merge_map()))
    for a, b in zip(*outs):
        assert np.array_equal(bits(a), bits(b))


def test_flag_values(hiplib):
    c = Converter(0)
    try:
        rec = mr.crafted_records(300, 11)

        def call(flags):
            p = MergeParamsC(10, 4, 0.5, flags)
            out = (C.c_uint64 * 4)()
            return hiplib.m2s_merge(c._h, C.byref(p), out), {name: int(out[k]) for k, name in enumerate(mr.COUNTS)}
        c.upload_records(rec)
        want_u, want_s = mu.merge(rec, 10, 4, 0.5)[2], mr.merge(rec, 10, 4, 0.5)[2]
        assert want_u["after"] < want_s["after"]
        for bad in mu.MERGE_FLAGS_REFUSED + (16, 0x80000004):
            assert call(bad)[0] == 1, bad
        assert call(1) == (0, want_s) and call(5) == (0, want_u)                     # 5: a dry run of the unsigned rule
        assert c.num_stored == 300 and np.array_equal(bits(c.download()), bits(rec))
        assert call(4) == (0, want_u) and c.num_stored == want_u["after"]
        # the build: the word that was `reserved` takes 0 or 4
        c.upload_records(rec)
        for bad in mu.BUILD_FLAGS_REFUSED:
            pc = lod.build_to_c((3, 10), 4, 0.5)
            pc.reserved = bad
            assert hiplib.m2s_lod_build(c._h, C.byref(pc), None) == 1, bad
        assert c.num_stored == 300
        pc = lod.build_to_c((3, 10), 4, 0.5)
        pc.reserved = 4
        v = (C.c_uint64 * 4)()
        assert hiplib.m2s_lod_build(c._h, C.byref(pc), v) == 0 and v[0] == 300
        assert c.lod_levels()[-1] - c.lod_levels()[-2] == mu.chain(rec, (3, 10))[0][-1].shape[0]
    finally:
        c.close()


def test_more_than_one_trip_of_every_grid(conv):
    """300 003 records: 1 172 workgroups of 256 in the per-record kernels, a partial last wave, segments of 64 members in one run"""
    n = 300003
    rng = np.random.default_rng(5)
    base = mr.crafted_records(4099, 77)
    rec = base[rng.integers(0, len(base), n)]
    rec[:, 0:3] = rng.normal(0, 1, (n, 3)).astype(F)
    valid = int(mr.cr.valid_mask(rec).sum())
    got, m = check(conv, rec, 10, 64, -2.0)
    assert len(got) == (valid + 63) // 64 + (n - valid)


def test_nested_spheres_merge_to_budget_with_the_flag(conv):
    """The unsigned counterpart of tests/test_gpu_merge.py's row merge_to_budget(6 660) on the nested spheres of DESIGN 5.16 (R = 64,
    128 x 128, three views at 20 degrees).  Printed, not asserted: no bar was set on it."""
    from mesh2splat_amd.prune import orbit_cameras
    R, W, H = 64, 128, 128
    scene = Scene([Mesh(name="outer", vertices=synth.cube_sphere_vertices(10, 1.0), base_color=(0.8, 0.6, 0.4, 1.0)),
                   Mesh(name="inner", vertices=synth.cube_sphere_vertices(8, 0.5), base_color=(0.2, 0.4, 0.9, 1.0))])
    cams = orbit_cameras(scene, 3, W, H, (20.0,))
    conv.upload_scene(scene)
    for flag in (False, True):
        n = conv.convert(R)
        counts = conv.merge_to_budget(6660, unsigned_axis=flag)
        assert counts["before"] == n and counts["after"] == conv.num_stored and mr.cr.valid_mask(conv.download()).all()
        s = conv.score_views(cams, R, (2.0, 2.5, 3.0), 30.0, shadow_resolution=128)[1]
        print(f"nested spheres, merge_to_budget(6660) unsigned_axis={flag}: level {counts['level']}, met {counts['met']}, {counts['after']} records, "
              f"psnr {s.psnr:.2f} dB, ssim {s.ssim:.4f}")
        assert np.isfinite(s.psnr) and np.isfinite(s.ssim)


def test_zz_achieved_errors_stay_within_the_guards():
    """Runs last in this module: the largest errors of every comparison above, and that the cases did turn members."""
    print(f"unsigned merge, achieved over the module: scalar {WORST['scalar_ulps']:.3f} ulp (guard {mr.SCALAR_ULPS_GUARD}), "
          f"covariance {WORST['cov_rel']:.3e} of 12 l1 (guard {mr.COV_REL_GUARD:.1e}), members turned {WORST['flipped']}")
    assert WORST["scalar_ulps"] <= mr.SCALAR_ULPS_GUARD and WORST["cov_rel"] <= mr.COV_REL_GUARD and WORST["flipped"] > 1000
