"""-m gpu: m2s_merge under M2S_MERGE_MODEL_GAUSSIAN (Converter.set_merge_model) against its numpy restatement (tests/merge_gauss_ref.py:
pins 2g, 5g, 5sg).  Segmentation, counts, map and copied records are exact; a parent's scalar fields lie within 4 fp32 ulps of the
field's magnitude and the covariance it draws within 1e-5 l1 of the restatement's moment (merge_ref's bars, carried over).  Then the
switch itself: back to the footprint and the bytes are merge_ref's, the unsigned flag changes nothing, the errors, what a call
invalidates, the SH plane with the weights of 5sg, and 300 003 records."""
import ctypes as C

import numpy as np
import pytest

import merge_gauss_ref as mg
import merge_ref as mr
import merge_sh_ref as ms
from mesh2splat_amd import synth
from mesh2splat_amd._lib import M2SError
from mesh2splat_amd.converter import Converter
from mesh2splat_amd.merge import MergeParamsC

pytestmark = pytest.mark.gpu
F = np.float32
WORST = {"scalar_ulps": 0.0, "cov_rel": 0.0}                     # over the whole module: printed by the last test, guarded there


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def conv(hiplib):
    c = Converter(0)
    yield c
    c.close()


def check(conv, rec, level, max_group, min_axis_dot, sigma, upload=True):
    """merge() under the Gaussian model on the device against the restatement -> (records after, map)"""
    want, wmap, wcounts, info = mg.merge(rec, level, max_group, min_axis_dot, sigma)
    conv.set_merge_model("gaussian", sigma)
    assert conv.merge_model == ("gaussian", float(F(sigma)))
    if upload:
        conv.upload_records(rec)
    ptr = conv.device_records
    dry = conv.merge(level, max_group, min_axis_dot, dry_run=True)
    assert dry == wcounts, (dry, wcounts)
    assert conv.device_records == ptr and conv.num_stored == len(rec)               # a dry run changes nothing
    if upload:
        assert np.array_equal(bits(conv.download()), bits(rec))
    got_counts = conv.merge(level, max_group, min_axis_dot)
    assert got_counts == wcounts == conv.last_merge_counts(), (got_counts, wcounts)
    assert conv.num_stored == wcounts["after"]
    gmap = conv.download_merge_map()
    assert gmap.dtype == np.uint32 and np.array_equal(gmap, wmap)
    got = conv.download()
    err = mg.compare(got, want, info, sigma)
    print(f"gauss merge n={len(rec)} level={level} group={max_group} dot={min_axis_dot} sigma={sigma}: {wcounts} "
          f"scalar {err['scalar_ulps']:.3f} ulp, cov {err['cov_rel']:.3e}")
    for k in WORST:
        WORST[k] = max(WORST[k], err[k])
    assert err["scalar_ulps"] <= mg.SCALAR_ULPS_BAR and err["cov_rel"] <= mg.COV_REL_BAR, err
    return got, gmap


@pytest.mark.parametrize("sigma", (1.0, 0.65))
@pytest.mark.parametrize("level", (0, 3, 10))
@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257, 4099))
def test_fields_against_the_restatement(conv, n, level, sigma):
    rec = mg.gauss_records(n, n)
    merged = 0
    for max_group in (2, 5, 64):
        for dot in (-2.0, 0.5):
            got, m = check(conv, rec, level, max_group, dot, sigma)
            merged += conv.last_merge_counts()["merged"]
            # singletons and invalid records: byte for byte
            alone = np.flatnonzero(np.bincount(m, minlength=len(got))[m] == 1)
            assert np.array_equal(bits(got[m[alone]]), bits(rec[alone]))
            bad = np.flatnonzero(~mr.cr.valid_mask(rec))
            assert list(m[bad]) == list(range(len(got) - len(bad), len(got)))
    if n >= 63:
        assert merged > 0


def test_hand_derived_parents_on_the_device(conv):
    """tests/test_merge_gauss_ref.py's dyadic cases: every operation is exact, so the device's floats are the derived ones"""
    r = np.zeros((2, 24), F)
    r[:, 3], r[:, 16] = 1, 1
    r[:, 4:8] = (0.5, 0.25, 0.75, 0.25)
    for s, sigma, want in ((0.75, 1.0, (1.25, 0.75, 0.75)), (0.375, 2.0, (0.625, 0.375, 0.375))):
        r[:, 8:11] = s
        r[0, 0], r[1, 0] = -1.0, 1.0
        got, _ = check(conv, r, 10, 4, -2.0, sigma)
        assert len(got) == 1 and np.array_equal(got[0, 8:11], np.array(want, F)) and np.array_equal(got[0, 0:3], np.zeros(3, F))
    r[:, 0] = 0.5
    r[:, 8:11] = (0.5, 0.25, 0.125)
    got, _ = check(conv, r, 10, 4, -2.0, 1.0)
    assert np.array_equal(got[0, 8:11], r[0, 8:11]) and got[0, 7] == F(0.5) and np.array_equal(got[0, 16:20], np.array((1, 0, 0, 0), F))
    h, s = 2.0 ** -3, 2.0 ** -4
    b = np.repeat(r[:1], 4, 0)
    b[:, 8:11] = (s, s, 0)
    b[:, 0], b[:, 1] = (0, h, 0, h), (0, 0, h, h)
    got, _ = check(conv, b, 10, 4, 0.5, 1.0)
    assert len(got) == 1 and got[0, 8] == got[0, 9] == F(np.sqrt(2.0 ** -7)) and got[0, 10] == 0
    assert np.array_equal(got[0, 0:3], np.array((h / 2, h / 2, 0), F))


def test_the_run_rule_reads_the_row_of_the_smallest_scale(conv):
    r = np.zeros((2, 24), F)
    r[:, 3], r[:, 16] = 1, 1
    r[1, 16:20] = mr.quat_cast_wxyz((0, 1, 0), (-1, 0, 0), (0, 0, 1)).astype(F)      # the same r_3, r_1 and r_2 a quarter turn on
    for scale, after in (((0.01, 1, 1), 2), ((1, 0.01, 1), 2), ((1, 1, 0.01), 1), ((1, 1, 0), 1), ((1, 1, 1), 2)):
        r[:, 8:11] = scale
        check(conv, r, 10, 4, 0.5, 1.0)
        assert conv.num_stored == after, scale


def test_two_runs_agree_and_the_unsigned_flag_changes_nothing(conv):
    rec = mg.gauss_records(1000, 13)
    conv.set_merge_model("gaussian", 0.65)
    outs = []
    for unsigned in (False, False, True):
        conv.upload_records(rec)
        counts = conv.merge(3, 5, 0.5, unsigned_axis=unsigned)
        outs.append((counts, conv.download(), conv.download_merge_map()))
        assert conv.merge(10, 64, 0.5, dry_run=True, unsigned_axis=unsigned) == conv.merge(10, 64, 0.5, dry_run=True)
    for counts, got, m in outs[1:]:
        assert counts == outs[0][0] and np.array_equal(bits(got), bits(outs[0][1])) and np.array_equal(m, outs[0][2])
    assert outs[0][0]["merged"] > 50


def test_back_to_the_footprint_the_bytes_are_what_they_were(conv, hiplib):
    """the same context, after merges under the Gaussian model: FOOTPRINT gives what a context that never saw the switch gives, and
    that is merge_ref's (within its bars); sigma is not read"""
    rec = mr.crafted_records(1000, 21)
    fresh = Converter(0)
    try:
        assert fresh.merge_model == ("footprint", 1.0)
        fresh.upload_records(rec)
        fresh.merge(3, 5, 0.5)
        base, base_map = fresh.download(), fresh.download_merge_map()
    finally:
        fresh.close()
    conv.set_merge_model("gaussian", 0.65)
    conv.upload_records(rec)
    conv.merge(3, 5, 0.5)
    assert not np.array_equal(bits(conv.download()), bits(base))
    for sigma in (1.0, 0.3):
        conv.set_merge_model("footprint", sigma)
        assert conv.merge_model == ("footprint", float(F(sigma)))
        conv.upload_records(rec)
        conv.merge(3, 5, 0.5)
        got = conv.download()
        assert np.array_equal(bits(got), bits(base)) and np.array_equal(conv.download_merge_map(), base_map)
    want, wmap, _, info = mr.merge(rec, 3, 5, 0.5)
    err = mr.compare(got, want, info)
    assert np.array_equal(base_map, wmap) and err["scalar_ulps"] <= mr.SCALAR_ULPS_BAR and err["cov_rel"] <= mr.COV_REL_BAR


def test_errors_of_the_switch(hiplib):
    c = Converter(0)
    try:
        h = c._h
        assert hiplib.m2s_merge_model(h) == 0 and hiplib.m2s_merge_sigma(h) == 1.0
        for model, sigma in ((2, 1.0), (0xFFFFFFFF, 1.0), (1, float("nan")), (1, float("inf")), (1, float("-inf")), (1, 0.0), (1, -0.0), (1, -1.0),
                             (0, float("nan")), (0, 0.0)):
            assert hiplib.m2s_set_merge_model(h, model, sigma) == 1, (model, sigma)
            assert hiplib.m2s_merge_model(h) == 0 and hiplib.m2s_merge_sigma(h) == 1.0
        with pytest.raises(ValueError):
            c.set_merge_model("gauss")
        assert hiplib.m2s_set_merge_model(h, 1, 0.65) == 0 and c.merge_model == ("gaussian", float(F(0.65)))
        # no new flag bits: what m2s_merge refused it refuses, under either model
        c.upload_records(mg.gauss_records(20, 1))
        for flags in (2, 3, 6, 7, 8, 16, 0x80000004):
            p = MergeParamsC(0, 4, 0.5, flags)
            assert hiplib.m2s_merge(h, C.byref(p), None) == 1, flags
        # conversions in flight: refused, the setting stays
        c.upload_scene(synth.cube_sphere(6, tex_size=16))
        c.submit(48)
        assert hiplib.m2s_set_merge_model(h, 0, 1.0) == 7 and b"in flight" in hiplib.m2s_last_error(h)
        assert c.merge_model == ("gaussian", float(F(0.65)))
        total = c.wait()
        assert c.merge(2, 4, 0.5)["before"] == total
        c.set_merge_model("footprint")
        assert c.merge_model == ("footprint", 1.0)
    finally:
        c.close()


def test_what_the_switch_and_a_merge_under_it_invalidate(conv):
    """the switch itself invalidates nothing; a merge under the Gaussian model invalidates what pin 7 says, a dry run nothing"""
    rec = mg.gauss_records(300, 11)
    conv.set_merge_model("footprint")
    conv.carry_sh = False
    conv.upload_records(rec)
    conv.merge(10, 4, 0.5)
    first_map = conv.download_merge_map()
    sh = ms.random_plane(conv.num_stored, 3)
    conv.upload_sh(sh)
    conv.contrib_begin()
    ptr, stored = conv.device_records, conv.num_stored
    conv.set_merge_model("gaussian", 0.65)
    assert conv.device_records == ptr and conv.num_stored == stored and conv.device_sh and conv.device_contrib(0)
    assert np.array_equal(conv.download_merge_map(), first_map)
    dry = conv.merge(10, 4, -2.0, dry_run=True)
    assert conv.device_records == ptr and conv.device_sh and conv.device_contrib(0) and np.array_equal(conv.download_merge_map(), first_map)
    real = conv.merge(10, 4, -2.0)
    assert real == dry and real["after"] < stored
    assert conv.device_sh == 0 and conv.device_contrib(0) == 0 and not conv.positions_ready
    assert conv.download_merge_map().size == stored
    with pytest.raises(M2SError):
        conv.sh_plane_info()


@pytest.mark.parametrize("n,level,max_group,dot", ((65, 10, 64, -2.0), (4099, 3, 5, 0.5), (4099, 10, 2, -2.0)))
def test_the_sh_plane_takes_the_weights_of_5sg(conv, n, level, max_group, dot):
    rec = mg.gauss_records(n, n + 1)
    sh = ms.random_plane(n, n)
    conv.set_merge_model("gaussian", 0.65)
    conv.carry_sh = True
    try:
        conv.upload_records(rec)
        conv.upload_sh(sh, degree=2)
        counts = conv.merge(level, max_group, dot)
        perm, heads = mg.segment_heads(rec, level, max_group, dot)
        wplane, pinfo = mg.merge_plane(rec, sh, perm, heads)
        assert conv.sh_plane_info() == {"rows": counts["after"], "degree": 2} and len(wplane) == counts["after"]
        ulps = ms.compare(conv.download_sh(), wplane, pinfo)
        print(f"gauss merge+sh n={n} level={level} group={max_group}: {counts}, plane within {ulps:.4f} ulp of max|sh|; unit segments {int(pinfo['unit'].sum())}")
        assert ulps <= ms.PLANE_ULPS_BAR
        # ... and they are not the footprint's weights: the same segments, sx sy in place of the area
        fplane, _ = ms.merge_plane(rec, sh, perm, heads)
        assert not np.array_equal(bits(fplane), bits(wplane))
    finally:
        conv.carry_sh = False


def test_more_than_one_trip(conv):
    """300 003 records: 1 172 workgroups of 256 in the per-record kernels and a partial last wave, 19 workgroups of the reduction"""
    n = 300003
    rng = np.random.default_rng(5)
    base = mg.gauss_records(4099, 77)
    rec = base[rng.integers(0, len(base), n)]
    rec[:, 0:3] = rng.normal(0, 1, (n, 3)).astype(F)
    valid = int(mr.cr.valid_mask(rec).sum())
    assert 0 < n - valid < 1000
    first, m1 = check(conv, rec, 10, 64, -2.0, 0.65)
    assert len(first) == (valid + 63) // 64 + (n - valid)


def test_zz_achieved_errors_stay_within_four_times_the_measured(conv):
    """Runs last in this module: the largest errors of every comparison above, against the guards at 4 x what the MI355X measured."""
    conv.set_merge_model("footprint")
    print(f"gauss merge, achieved over the module: scalar {WORST['scalar_ulps']:.3f} ulp (guard {mg.SCALAR_ULPS_GUARD}), "
          f"covariance {WORST['cov_rel']:.3e} of l1 (guard {mg.COV_REL_GUARD:.1e})")
    assert WORST["scalar_ulps"] <= mg.SCALAR_ULPS_GUARD and WORST["cov_rel"] <= mg.COV_REL_GUARD
