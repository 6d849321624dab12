"""-m gpu: m2s_merge / Converter.merge against the numpy restatement (tests/merge_ref.py).  Segmentation, counts, map and copied records
are exact; a parent's scalar fields lie within 4 fp32 ulps of the field's magnitude and its viewer covariance within 1e-5 * 12 l1 of
the restatement's (the bars and what the MI355X achieves: merge_ref's docstring).  Crafted records round the wave and workgroup edges,
the exact cases of the run rule, the effect on the context, the errors, more than one trip of every grid, two merges whose maps
compose, merge_to_budget, and — printed, not asserted — merging beside dropping on the nested spheres of DESIGN 5.16."""
import ctypes as C

import numpy as np
import pytest

import merge_ref as mr
from mesh2splat_amd import synth
from mesh2splat_amd._lib import M2SError
from mesh2splat_amd.bake import BakeParams
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.light import LightParams
from mesh2splat_amd.merge import MergeParamsC
from mesh2splat_amd.prune import orbit_cameras
from mesh2splat_amd.scene import Mesh, Scene

pytestmark = pytest.mark.gpu
F = np.float32
WORST = {"scalar_ulps": 0.0, "cov_rel": 0.0}                     # over the whole module: printed by the last test, guarded there


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def check(conv, rec, level, max_group, min_axis_dot, upload=True):
    """merge() on the device against the restatement -> (records after, map)"""
    want, wmap, wcounts, info = mr.merge(rec, level, max_group, min_axis_dot)
    if upload:
        conv.upload_records(rec)
    dry = conv.merge(level, max_group, min_axis_dot, dry_run=True)
    assert dry == wcounts, (dry, wcounts)
    assert conv.merge_count(level, max_group, min_axis_dot) == wcounts["after"]
    got_counts = conv.merge(level, max_group, min_axis_dot)
    assert got_counts == wcounts == conv.last_merge_counts(), (got_counts, wcounts)
    assert conv.num_stored == wcounts["after"]
    gmap = conv.download_merge_map()
    assert gmap.dtype == np.uint32 and np.array_equal(gmap, wmap)
    got = conv.download()
    err = mr.compare(got, want, info)
    print(f"merge n={len(rec)} level={level} group={max_group} dot={min_axis_dot}: {wcounts} scalar {err['scalar_ulps']:.3f} ulp, cov {err['cov_rel']:.3e}")
    for k in WORST:
        WORST[k] = max(WORST[k], err[k])
    assert err["scalar_ulps"] <= mr.SCALAR_ULPS_BAR and err["cov_rel"] <= mr.COV_REL_BAR, err
    return got, gmap


@pytest.mark.parametrize("level", (0, 3, 10))
@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257, 4099))
def test_fields_against_the_restatement(conv, n, level):
    rec = mr.crafted_records(n, n)
    merged = 0
    for max_group in (2, 5, 64):
        for dot in (-2.0, 0.5):
            check(conv, rec, level, max_group, dot)
            merged += conv.last_merge_counts()["merged"]
    if n >= 63:
        assert merged > 0                                                           # (the cases do merge something)


def test_dot_equal_to_the_threshold_does_not_break_and_a_nan_does(conv):
    a = mr.crafted_records(2, 1, invalid=False)
    a[:, 0:3] = (0.5, 0.25, -1.0)
    a[:, 8:10] = 0.1
    a[0, 16:20] = (1, 0, 0, 0)                                                       # r_3 = (0, 0, 1) exactly
    a[1, 16:20] = (0.9, 0.3, 0.2, 0.1)
    v = mr.axis3_f32(a[:, 16:20])[1, 2]                                              # the dot product is r_3.z of the second, exactly
    assert 0 < v < 1
    for thr, after in ((float(v), 1), (float(np.nextafter(v, F(2))), 2), (float(np.nextafter(v, F(-2))), 1)):
        _, m = check(conv, a, 0, 4, thr)
        assert conv.num_stored == after
    # two valid records whose third axes are finite and whose dot product is inf - inf
    s = F(1e10)
    h = np.sqrt(0.5)
    b = a.copy()
    b[0, 16:20] = np.array(mr.quat_cast_wxyz((0, 0, -1), (-h, h, 0), (h, h, 0)), F) * s
    b[1, 16:20] = np.array(mr.quat_cast_wxyz((0, 0, -1), (h, h, 0), (h, -h, 0)), F) * s
    ax = mr.axis3_f32(b[:, 16:20])
    assert np.isfinite(ax).all() and ax[0, 0] > 1e19 and ax[1, 1] < -1e19
    with np.errstate(all="ignore"):
        assert np.isnan(((ax[0, 0] * ax[1, 0]) + ax[0, 1] * ax[1, 1]) + ax[0, 2] * ax[1, 2])
    check(conv, b, 10, 4, -2.0)
    assert conv.num_stored == 2 and conv.last_merge_counts()["merged"] == 0


def test_identical_positions_follow_index_order(conv):
    n = 150
    rec = mr.crafted_records(n, 4, invalid=False)
    rec[:, 0:3] = (1.0, 2.0, 3.0)
    _, m = check(conv, rec, 0, 5, -2.0)
    assert np.array_equal(m, np.arange(n) // 5)
    _, m = check(conv, rec, 10, 64, -2.0)
    assert np.array_equal(m, np.arange(n) // 64)


def test_grid_tiles_become_the_tiles_of_half_the_density(conv):
    rec = mr.grid_records(8)
    got, m = check(conv, rec, 8, 4, 0.5)
    assert len(got) == 16 and (got[:, 8] == F(0.25)).all() and (got[:, 9] == F(0.25)).all()
    iy, ix = np.divmod(np.arange(64), 8)
    centre = np.stack([(ix // 2) * 0.25 + 0.125, (iy // 2) * 0.25 + 0.125], 1)
    assert np.abs(got[m][:, 0:2] - centre).max() < 1e-7


def test_passthrough_is_byte_identical(conv):
    rec = mr.crafted_records(500, 9)
    got, m = check(conv, rec, 0, 4, 0.5)
    members = np.bincount(m, minlength=len(got))
    alone = np.flatnonzero(members[m] == 1)
    assert alone.size > 50
    assert np.array_equal(got[m[alone]].view(np.uint32), rec[alone].view(np.uint32))
    bad = np.flatnonzero(~mr.cr.valid_mask(rec))
    assert bad.size == 3 and list(m[bad]) == list(range(len(got) - 3, len(got)))


def test_dry_run_touches_nothing_and_the_real_call_invalidates(conv):
    rec = mr.crafted_records(300, 11)
    conv.upload_records(rec)
    conv.merge(10, 4, 0.5)                                                           # a map of some other records
    conv.upload_records(rec)
    with pytest.raises(M2SError):
        conv.download_merge_map()                                                    # ... does not survive them
    assert conv.device_merge_map == 0
    sh = conv.bake_light(BakeParams(n_theta=4, n_phi=8, use_shadows=False), LightParams(light_position=(1.5, 2.0, 2.5)))
    conv.contrib_begin()
    w = np.arange(300, dtype=np.uint32)
    conv.upload_contrib(None, w)
    conv.refit_begin()
    ptr = conv.device_records
    dry = conv.merge(3, 4, 0.5, dry_run=True)
    assert dry["before"] == 300 and dry["after"] < 300
    assert conv.device_records == ptr and conv.num_stored == 300
    assert np.array_equal(conv.download().view(np.uint32), rec.view(np.uint32))
    assert np.array_equal(conv.download_contrib()[1], w) and conv.device_refit(0) and conv.device_sh
    assert np.array_equal(conv.download_sh().view(np.uint32), sh.view(np.uint32))
    assert conv.device_merge_map == 0                                                # a dry run leaves no map
    real = conv.merge(3, 4, 0.5)
    assert real == dry and conv.num_stored == dry["after"] and conv.device_records != ptr
    with pytest.raises(M2SError):
        conv.download_contrib()
    assert conv.device_contrib(0) == 0 and conv.device_refit(0) == 0 and conv.device_sh == 0 and not conv.positions_ready
    assert conv.device_merge_map != 0 and conv.download_merge_map().size == 300


def test_adopted_memory_is_not_written_and_two_runs_agree(conv):
    rec = mr.crafted_records(1000, 13)
    owner = Converter(0)                                                             # (its uploaded records are the memory the other adopts)
    try:
        owner.upload_records(rec)
        outs = []
        for _ in range(2):
            conv.set_records(owner.device_records, len(rec), 64)
            got, m = check(conv, rec, 3, 5, 0.5, upload=False)
            assert conv.device_records != owner.device_records
            assert np.array_equal(owner.download().view(np.uint32), rec.view(np.uint32))
            outs.append((got.copy(), m.copy()))
        assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)) and np.array_equal(outs[0][1], outs[1][1])
    finally:
        owner.close()


def test_errors(hiplib):
    c = Converter(0)
    try:
        def call(level=0, max_group=4, dot=0.5, flags=0, reserved=(0, 0)):
            p = MergeParamsC(level, max_group, dot, flags)
            p.reserved[:] = reserved
            out = (C.c_uint64 * 4)()
            return hiplib.m2s_merge(c._h, C.byref(p), out)
        assert call() == 7                                                           # no records
        with pytest.raises(M2SError):
            c.download_merge_map()
        c.upload_records(mr.crafted_records(20, 1))
        before = c.download()
        for bad in (dict(level=11), dict(max_group=1), dict(max_group=0), dict(max_group=65), dict(dot=float("nan")), dict(flags=2), dict(flags=3),
                    dict(reserved=(1, 0)), dict(reserved=(0, 1))):
            assert call(**bad) == 1, bad
        assert hiplib.m2s_merge(c._h, None, None) == 1
        assert np.array_equal(c.download().view(np.uint32), before.view(np.uint32)) and c.num_stored == 20
        assert call(level=10, max_group=64, dot=float("-inf")) == 0 and c.num_stored == mr.merge(before, 10, 64, float("-inf"))[2]["after"] < 20
        n = C.c_uint64()
        small = (C.c_uint32 * 19)()
        assert hiplib.m2s_download_merge_map(c._h, small, 19, C.byref(n)) == 5 and n.value == 20
        # conversions in flight: refused, nothing touched, the conversion still delivered
        c.upload_scene(synth.cube_sphere(6, tex_size=16))
        c.submit(48)
        total = c.wait()
        c.submit(48)
        assert call() == 7 and call(flags=1) == 7 and b"in flight" in hiplib.m2s_last_error(c._h)
        assert c.wait() == total
        assert c.merge(2, 4, 0.5)["before"] == total
    finally:
        c.close()


def test_more_than_one_trip_and_two_merges_compose(conv):
    """300 003 records: 1 172 workgroups of 256 in the per-record kernels and a partial last wave; the first merge leaves its parents in
    the pool, so the second goes through the staging buffer, and the two maps compose to the restatement's."""
    n = 300003
    rng = np.random.default_rng(5)
    base = mr.crafted_records(4099, 77)
    rec = base[rng.integers(0, len(base), n)]
    rec[:, 0:3] = rng.normal(0, 1, (n, 3)).astype(F)
    valid = int(mr.cr.valid_mask(rec).sum())
    assert 0 < n - valid < 1000
    first, m1 = check(conv, rec, 10, 64, -2.0)
    assert len(first) == (valid + 63) // 64 + (n - valid)                            # one run, cut every 64; the invalid ones behind it
    want2, wmap2, _, _ = mr.merge(first, 10, 64, -2.0)
    second, m2 = check(conv, first, 10, 64, -2.0, upload=False)
    assert len(second) == len(want2) and np.array_equal(m2[m1], wmap2[m1]) and np.bincount(m2[m1], minlength=len(second)).sum() == n


def test_merge_to_budget_on_a_unit_quad(conv):
    conv.upload_scene(synth.unit_quad())
    n = conv.convert(64)
    assert n > 2000
    rec = conv.download()
    budget = n // 3                                                                  # (max_group = 4 cannot go below n / 4)
    counts = {lv: mr.merge(rec, lv, 4, 0.5)[2]["after"] for lv in range(11)}
    want = min(lv for lv in range(11) if counts[lv] <= budget)
    out = conv.merge_to_budget(budget)
    assert out["met"] and out["level"] == want and out["after"] == counts[want] == conv.num_stored <= budget
    assert want == 0 or counts[want - 1] > budget
    assert mr.cr.valid_mask(conv.download()).all()
    # already within the budget: the finest level is 0; a budget nothing meets: the coarsest level, and it says so
    again = conv.merge_to_budget(conv.num_stored)
    assert again["level"] == 0 and again["met"] and again["after"] <= again["before"]
    conv.convert(64)
    out = conv.merge_to_budget(1, max_group=2)
    assert out["level"] == 10 and not out["met"] and out["after"] > 1


def test_nested_spheres_merging_against_dropping(conv):
    """DESIGN 5.16's table with one more row: the nested spheres at R = 64, 128 x 128, three views at 20 degrees; every record, then
    merge_to_budget(6 660), then the AREA budget and the cap at the count the merge reached.  Printed, not asserted: nobody knows
    beforehand which wins.  Asserted: every record after the merge is valid and the scores are finite."""
    R, W, H = 64, 128, 128
    scene = Scene([Mesh(name="outer", vertices=synth.cube_sphere_vertices(10, 1.0), base_color=(0.8, 0.6, 0.4, 1.0)),
                   Mesh(name="inner", vertices=synth.cube_sphere_vertices(8, 0.5), base_color=(0.2, 0.4, 0.9, 1.0))])
    light = (2.0, 2.5, 3.0)
    cams = orbit_cameras(scene, 3, W, H, (20.0,))
    conv.upload_scene(scene)
    n = conv.convert(R)

    def score():
        return conv.score_views(cams, R, light, 30.0, shadow_resolution=128)[1]

    out = {"all": (n, score())}
    counts = conv.merge_to_budget(6660)
    m = counts["after"]
    assert counts["before"] == n and m == conv.num_stored and (m <= 6660 or not counts["met"])
    assert mr.cr.valid_mask(conv.download()).all()
    out[f"merge (level {counts['level']})"] = (m, score())
    assert conv.convert(R) == n
    assert conv.prune_budget(m, "area")["kept"] == m
    out["area"] = (m, score())
    conv.set_max_gaussians(m)
    try:
        assert conv.convert(R) == n and conv.num_stored == m
        out["cap"] = (m, score())
    finally:
        conv.set_max_gaussians(-1)
    for name, (k, s) in out.items():
        print(f"nested spheres, {name}: {k} records, psnr {s.psnr:.2f} dB, ssim {s.ssim:.4f}")
        assert np.isfinite(s.psnr) and np.isfinite(s.ssim)


def test_zz_achieved_errors_stay_within_four_times_the_measured():
    """Runs last in this module: the largest errors of every comparison above, against the guards at 4 x what the MI355X measured."""
    print(f"merge, achieved over the module: scalar {WORST['scalar_ulps']:.3f} ulp (guard {mr.SCALAR_ULPS_GUARD}), "
          f"covariance {WORST['cov_rel']:.3e} of 12 l1 (guard {mr.COV_REL_GUARD:.1e})")
    assert WORST["scalar_ulps"] <= mr.SCALAR_ULPS_GUARD and WORST["cov_rel"] <= mr.COV_REL_GUARD
